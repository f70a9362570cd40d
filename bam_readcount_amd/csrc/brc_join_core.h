// brc_join_core.h — per-lane functions of the device-side join of computed regions (include/brc_join.h), written once for the gfx950
// kernels (brc_join.hip) and for the CPU build the tests run (tests/sim_join).
//
//   planes_lane   lane = (row of the 29 * L joined rows, group of destination elements): group 0 is the 0 .. 3 elements in front of the
//                 row's first 16-byte boundary, group g >= 1 the four elements behind it — ONE 16-byte store where all four lie in the
//                 window, single stores at the row's end.  The source is looked up once per row (uniform over a workgroup).
//   xagg_lane     lane = joined third-allele record: 64 bytes in, k rebased, the library renumbered, 64 bytes out
//   slots_lane    lane = joined indel record: 72 bytes in, kept or not, 72 bytes out, its synthetic read's length, its bytes into the
//                 scratch, the kept count                                                                   (atomic)
//   [scan]        bytes[] -> offs[], total -> counts[1]
//   reads_lane    lane = joined indel record: seq_off, and — when the total fits seq_cap — its nibbles out of the source's read
//   ref_lane      lane = byte of the joined reference slice: the first source that has a character there
// The scan is cooperative on the device (brc_side_scan.h) and a serial loop in the CPU build; everything else is the same code.
#ifndef BRC_JOIN_CORE_H
#define BRC_JOIN_CORE_H

#include <stdint.h>
#include <string.h>

#include "../../include/brc_join.h"

#if defined(__HIPCC__)
#define BRCJ_HD __host__ __device__ inline
#else
#define BRCJ_HD inline
#endif

namespace brcjoin {

enum { BLOCK = 256, KMAX = BRC_JOIN_MAX_SOURCES, ROWS = 29, NI = BRC_NI, NF = BRC_NF };
static const uint32_t NONE32 = 0xFFFFFFFFu;
static const uint32_t EMPTY_SLOT = 1u | (7u << 8);           // lane2_store's slot word of a dead lane: bucket 1, no alternate (NB_NONE)

struct Rec { uint32_t w[16]; };                              // struct XAgg: k, library << 8 | bucket, 9 integers, 4 floats, a pad word
struct Slot { int32_t pos, lib, len; uint32_t rep_read; int32_t rep_qpos; uint32_t i[NI]; uint32_t f[NF]; };      // struct IndelOut; the floats as bit patterns
static_assert(sizeof(Rec) == 64 && sizeof(Slot) == 72, "record sizes of include/brc.h");

// One source, as the kernels see it.  plane[]: ncol, depth, slotid, si, sf as 32-bit words, PS elements between rows.
struct Src {
    const uint32_t* plane[5];
    int64_t d, P, PS;                                        // pos0 - pos0_s; n_pos_s; stride_s
    int32_t L, pos0;
    const Rec* xagg; const Slot* slots;
    const uint8_t* seq4; const uint64_t* seq_off; const int32_t* l_qseq; int64_t n_reads;
    const char* ref; int64_t ref_lo, ref_hi;
};

// One call's work, BY VALUE in the kernel arguments.
struct Job {
    int32_t K, L; int64_t pos0, n, DS;                       // the window [pos0, pos0 + n), destination rows DS elements apart
    Src s[KMAX];
    int32_t base[KMAX + 1];                                  // joined library of a source's library 0
    uint64_t xbase[KMAX + 1], sbase[KMAX + 1];               // joined record of a source's record 0
    uint32_t* o_plane[5];
    Rec* o_xagg; Slot* o_slots; uint64_t* o_seq_off; int32_t* o_l_qseq; uint8_t* o_seq4; int64_t seq_cap;
    char* o_ref; int64_t ref_lo, ref_hi, ref_len;
    uint32_t *bytes, *offs, *part, *tot;                     // scratch: bytes [S], offs [S + 1], the scan's partials, its total
    uint32_t *o_counts, *status;
};

inline uint64_t scan_blocks(uint64_t n) { return (n + BLOCK - 1) / BLOCK; }
inline uint64_t workspace_words(uint64_t S) { return S + (S + 1) + scan_blocks(S) + 1 + 1; }
inline size_t workspace_bytes(uint64_t S) { return S ? (size_t)(workspace_words(S) * 4u) : 0; }
inline void carve(Job& J, void* ws) {
    uint32_t* w = (uint32_t*)ws; const uint64_t S = J.sbase[J.K];
    J.bytes = w; w += S; J.offs = w; w += S + 1; J.part = w; w += scan_blocks(S) + 1; J.tot = w;
}

// A destination store: written once and not read again by this library — on the device past the caches' retention (non-temporal).
BRCJ_HD void put(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_nontemporal_store(v, p);
#else
    *p = v;
#endif
}
// four words at a 16-byte boundary: one store on the device
BRCJ_HD void put4(uint32_t* p, const uint32_t* v) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    u32x4 x; x.x = v[0]; x.y = v[1]; x.z = v[2]; x.w = v[3];
    __builtin_nontemporal_store(x, (u32x4*)p);
#else
    p[0] = v[0]; p[1] = v[1]; p[2] = v[2]; p[3] = v[3];
#endif
}
// a source word: read once by this library
BRCJ_HD uint32_t get(const uint32_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_nontemporal_load(p);
#else
    return *p;
#endif
}
// four source words: one 16-byte load on the device where the address allows it, four loads otherwise (the source's offset
// pos0 - pos0_s is arbitrary: a row's loads cannot all be aligned with its stores)
BRCJ_HD void get4(const uint32_t* p, uint32_t* v) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    if (((uintptr_t)p & 15u) == 0) {
        const u32x4 x = __builtin_nontemporal_load((const u32x4*)p);
        v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
        return;
    }
#endif
    v[0] = get(p); v[1] = get(p + 1); v[2] = get(p + 2); v[3] = get(p + 3);
}
BRCJ_HD void count_up(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(p, v);
#else
    *p += v;
#endif
}
BRCJ_HD void or_bits(uint32_t* p, uint32_t bits) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicOr(p, bits);
#else
    *p |= bits;
#endif
}

// the source a joined index belongs to: the last s whose base is not above it (K <= 16: a handful of compares)
template <class T> BRCJ_HD int source_of(const T* base, int K, T x) {
    int s = 0;
    while (s + 1 < K && x >= base[s + 1]) ++s;
    return s;
}

// elements in front of a row's first 16-byte boundary (rows are 4-byte aligned), and the groups that cover [0, n)
BRCJ_HD int64_t row_head(const uint32_t* row, int64_t n) {
    const int64_t h = (int64_t)(((16u - (uint32_t)((uintptr_t)row & 15u)) & 15u) >> 2);
    return h < n ? h : n;
}
BRCJ_HD int64_t row_groups(int64_t n) { return 1 + (n + 3) / 4; }      // enough for every alignment: group 0 and ceil((n - head) / 4) <= (n + 3) / 4

// Lane = (row y of the 29 * L joined rows, group g).  y = (joined library) * 29 + r; r: 0 ncol, 1 depth, 2 slotid, 3 .. 20 si, 21 .. 28 sf.
BRCJ_HD void planes_lane(const Job& J, int64_t y, int64_t g) {
    const int32_t lj = (int32_t)(y / ROWS), r = (int32_t)(y % ROWS);
    const int a = r < 3 ? r : (r < 21 ? 3 : 4), sub = r < 3 ? 0 : (r < 21 ? r - 3 : r - 21), per = a == 3 ? 18 : (a == 4 ? 8 : 1);
    uint32_t* dst = J.o_plane[a] + ((int64_t)lj * per + sub) * J.DS;
    const int64_t head = row_head(dst, J.n);
    const int64_t e0 = g == 0 ? 0 : head + 4 * (g - 1), e1 = g == 0 ? head : (e0 + 4 < J.n ? e0 + 4 : J.n);
    if (e0 >= e1) return;
    const int s = source_of(J.base, J.K, lj);
    const Src& S = J.s[s];
    const uint32_t* src = S.plane[a] + ((int64_t)(lj - J.base[s]) * per + sub) * S.PS;
    const uint32_t empty = r == 2 ? EMPTY_SLOT : 0u;
    const int64_t k0 = e0 + S.d;                             // the source element of e0
    if (e1 - e0 == 4 && g != 0) {
        uint32_t v[4];
        if (k0 >= 0 && k0 + 4 <= S.P) get4(src + k0, v);
        else for (int j = 0; j < 4; ++j) v[j] = (k0 + j >= 0 && k0 + j < S.P) ? get(src + k0 + j) : empty;
        put4(dst + e0, v);
        return;
    }
    for (int64_t e = e0; e < e1; ++e) {
        const int64_t k = e + S.d;
        put(dst + e, (k >= 0 && k < S.P) ? get(src + k) : empty);
    }
}

// Lane = joined third-allele record t: the record goes word by word from the source to its place (no copy of it lives in the lane).
BRCJ_HD void xagg_lane(const Job& J, uint64_t t) {
    const int s = source_of(J.xbase, J.K, t);
    const Src& S = J.s[s];
    const uint32_t* in = S.xagg[t - J.xbase[s]].w; uint32_t* out = J.o_xagg[t].w;
    const uint32_t k = in[0], lb = in[1], lib = lb >> 8;
    const int64_t kj = (int64_t)k - S.d;
    const bool used = k != NONE32 && (int64_t)k < S.P && lib < (uint32_t)S.L && kj >= 0 && kj < J.n;
    out[0] = used ? (uint32_t)kj : NONE32;
    out[1] = used ? ((lib + (uint32_t)J.base[s]) << 8) | (lb & 0xffu) : lb;
#pragma unroll
    for (int f = 2; f < 16; ++f) out[f] = in[f];
}

// a source record that the join keeps
BRCJ_HD bool kept(const Job& J, const Src& S, int32_t pos, int32_t lib, int32_t len) {
    const int64_t p = pos;
    return len != 0 && p >= J.pos0 && p < J.pos0 + J.n && p >= S.pos0 && p < (int64_t)S.pos0 + S.P && lib >= 0 && lib < S.L;
}

// Lane = joined indel record t.  With no destinations (a call for the counts alone) only the scratch and the count are written.
BRCJ_HD void slots_lane(const Job& J, uint64_t t) {
    const int s = source_of(J.sbase, J.K, t);
    const Src& S = J.s[s];
    const Slot* in = S.slots + (t - J.sbase[s]);
    const int32_t pos = in->pos, lib = in->lib, len = in->len;
    const bool keep = kept(J, S, pos, lib, len);
    const int32_t lq = keep && len > 0 ? len : 0;
    J.bytes[t] = ((uint32_t)lq + 1u) >> 1;
    if (keep && J.o_counts) count_up(J.o_counts, 1u);
    if (!J.o_slots) return;
    Slot* out = J.o_slots + t;
    out->pos = pos; out->lib = keep ? lib + J.base[s] : lib; out->len = keep ? len : 0;
    out->rep_read = (uint32_t)t; out->rep_qpos = -1;
#pragma unroll
    for (int f = 0; f < NI; ++f) out->i[f] = in->i[f];
#pragma unroll
    for (int f = 0; f < NF; ++f) out->f[f] = in->f[f];
    J.o_l_qseq[t] = lq;
}

// the source's raw 4-bit code at offset q of read rr, 15 where include/brc.h spells N
BRCJ_HD uint32_t nibble(const Src& S, uint32_t rr, int64_t q) {
    if ((int64_t)rr >= S.n_reads || q < 0 || q >= (int64_t)S.l_qseq[rr]) return 15u;
    const uint8_t b = S.seq4[S.seq_off[rr] + (uint64_t)(q >> 1)];
    return (q & 1) ? (b & 15u) : (uint32_t)(b >> 4);
}

// Lane = joined indel record t (after the scan): its read's offset, and its bytes when the whole arena fits.
BRCJ_HD void reads_lane(const Job& J, uint64_t t) {
    const uint32_t off = J.offs[t];
    J.o_seq_off[t] = off;
    const int64_t lq = J.o_l_qseq[t];
    if (lq <= 0 || !J.o_seq4 || (int64_t)J.tot[0] > J.seq_cap) return;
    const int s = source_of(J.sbase, J.K, t);
    const Src& S = J.s[s];
    const Slot* o = S.slots + (t - J.sbase[s]);
    const uint32_t rr = o->rep_read; const int64_t q0 = (int64_t)o->rep_qpos + 1;
    for (int64_t j = 0; j < lq; j += 2) {
        const uint32_t hi = nibble(S, rr, q0 + j), lo = j + 1 < lq ? nibble(S, rr, q0 + j + 1) : 0u;
        J.o_seq4[(uint64_t)off + (uint64_t)(j >> 1)] = (uint8_t)((hi << 4) | lo);
    }
}

// Lane = byte x of the joined reference slice.
BRCJ_HD void ref_lane(const Job& J, int64_t x) {
    const int64_t p = J.ref_lo + x;
    char c = 0; bool differs = false;
    for (int s = 0; s < J.K; ++s) {
        const Src& S = J.s[s];
        if (!S.ref || p < S.ref_lo || p >= S.ref_hi || p >= J.ref_len || p < 0) continue;
        const char q = S.ref[p - S.ref_lo];
        if (!q) continue;
        if (!c) c = q; else if (q != c) differs = true;
    }
    J.o_ref[x] = c;
    if (differs && J.status) or_bits(J.status, BRC_JOIN_REF_DIFFERS);
}

// ---------------------------------------------------------------------------------------------- the host's side of a call

struct Range { const char* lo; const char* hi; };
inline Range range_of(const void* p, uint64_t bytes) { Range r; r.lo = (const char*)p; r.hi = (const char*)p + (p ? bytes : 0); return r; }
inline bool overlap(const Range& a, const Range& b) { return a.lo < a.hi && b.lo < b.hi && a.lo < b.hi && b.lo < a.hi; }

inline uint64_t plane_bytes(uint64_t rows, int64_t stride, int64_t n) { return n > 0 && rows ? ((rows - 1) * (uint64_t)stride + (uint64_t)n) * 4u : 0; }

// K, the sources and the window: what brc_join_sizes_of and brc_join_views both refuse, and the host-known sizes.  `memory` / `device`
// come back as the sources' common ones.
inline int check_sources(int32_t K, const brc_join_source* src, int32_t pos0, int64_t n, int64_t stride, brc_join_sizes* z, int32_t* memory, int32_t* device,
                         const char** why) {
    memset(z, 0, sizeof *z);
    if (!src) { *why = "no sources"; return BRC_E_ARG; }
    if (K < 1 || K > KMAX) { *why = "K outside 1 .. BRC_JOIN_MAX_SOURCES"; return BRC_E_ARG; }
    if (n < 0 || stride < n) { *why = "n_pos below 0 or stride below n_pos"; return BRC_E_ARG; }
    if ((uint64_t)n >= 0x7ffffff0ull || (int64_t)pos0 + n > 0x7fffffffll) { *why = "window too large: positions are indexed with 32 bits"; return BRC_E_ARG; }
    int64_t L = 0, ref_len = -1, lo = 0, hi = 0; uint64_t nx = 0, ns = 0;
    for (int s = 0; s < K; ++s) {
        const brc_device_view* v = src[s].view; const brc_device_indels* d = src[s].indels;
        if (!v) { *why = "a source without a view"; return BRC_E_ARG; }
        if (v->n_lib < 1 || v->n_pos < 0 || v->stride < v->n_pos) { *why = "not a view of a computed region"; return BRC_E_ARG; }
        if (v->n_pos > 0 && (!v->ncol || !v->depth || !v->slotid || !v->si || !v->sf)) { *why = "a view without planes"; return BRC_E_ARG; }
        if (v->n_xagg && !v->xagg) { *why = "a view without its third-allele records"; return BRC_E_ARG; }
        if (s == 0) { *memory = v->memory; *device = v->device; }
        if (v->memory != *memory || v->device != *device) { *why = "views of mixed memory kind or device"; return BRC_E_ARG; }
        if (d) {
            if (d->memory != v->memory || d->device != v->device || d->n_lib != v->n_lib || d->pos0 != v->pos0 || d->n_pos != v->n_pos) {
                *why = "a source whose view and indels view disagree"; return BRC_E_ARG;
            }
            if ((d->n_slots && !d->slots) || d->n_reads < 0 || (d->n_reads > 0 && (!d->seq4 || !d->seq_off || !d->l_qseq))) {
                *why = "an indels view without its arrays"; return BRC_E_ARG;
            }
            ns += d->n_slots;
            if (d->ref) {
                if (d->ref_hi < d->ref_lo) { *why = "a reference slice that ends before it starts"; return BRC_E_ARG; }
                if (ref_len >= 0 && d->ref_len != ref_len) { *why = "sources whose ref_len differ"; return BRC_E_ARG; }
                if (ref_len < 0) { lo = d->ref_lo; hi = d->ref_hi; } else { lo = d->ref_lo < lo ? d->ref_lo : lo; hi = d->ref_hi > hi ? d->ref_hi : hi; }
                ref_len = d->ref_len;
            }
        }
        L += v->n_lib; nx += v->n_xagg;
        if (L > BRC_JOIN_MAX_LIB) { *why = "more than BRC_JOIN_MAX_LIB joined libraries"; return BRC_E_ARG; }
        if (nx >= 0x7ffffff0ull || ns >= 0x7ffffff0ull) { *why = "too many records: they are indexed with 32 bits"; return BRC_E_ARG; }
    }
    if (ref_len >= 0 && (uint64_t)(hi - lo) >= 0x7ffffff0ull) { *why = "reference slice too large"; return BRC_E_ARG; }
    z->n_lib = (int32_t)L;
    if (n == 0) return BRC_OK;                               // (an empty window joins nothing)
    z->n_xagg = nx; z->n_slots = ns;
    z->has_ref = ref_len >= 0; z->ref_lo = lo; z->ref_hi = hi; z->ref_len = ref_len >= 0 ? ref_len : 0;
    z->ncol_bytes = z->depth_bytes = z->slotid_bytes = plane_bytes((uint64_t)L, stride, n);
    z->si_bytes = plane_bytes((uint64_t)L * 18u, stride, n); z->sf_bytes = plane_bytes((uint64_t)L * 8u, stride, n);
    z->xagg_bytes = nx * 64u; z->slots_bytes = ns * 72u; z->seq_off_bytes = ns * 8u; z->l_qseq_bytes = ns * 4u;
    z->ref_bytes = (uint64_t)(hi - lo); z->workspace_bytes = workspace_bytes(ns);
    return BRC_OK;
}

// The argument checks of brc_join_views (everything but the kind of memory, which the two libraries check themselves): 0 = fine.
inline int check_job(int32_t K, const brc_join_source* src, int32_t pos0, int64_t n, int64_t stride, const brc_join_dest* dst, const brc_device_view* ov,
                     const brc_device_indels* oi, const uint32_t* counts, int64_t seq_cap, const uint32_t* status, const void* ws, size_t ws_bytes,
                     brc_join_sizes* z, int32_t* memory, int32_t* device, const char** why) {
    if (int rc = check_sources(K, src, pos0, n, stride, z, memory, device, why)) return rc;
    if (seq_cap < 0) { *why = "seq_cap below 0"; return BRC_E_ARG; }
    if (!dst && !counts) { *why = "neither destinations nor counts"; return BRC_E_ARG; }
    if (dst && !ov && !oi) { *why = "neither out_view nor out_indels"; return BRC_E_ARG; }
    if (n == 0) return BRC_OK;
    const bool planes = dst && ov, indels = !dst || oi;
    if (planes && (!dst->ncol || !dst->depth || !dst->slotid || !dst->si || !dst->sf || (z->n_xagg && !dst->xagg))) { *why = "a plane or record buffer of dst is NULL"; return BRC_E_ARG; }
    if (dst && oi && ((z->n_slots && (!dst->slots || !dst->seq_off || !dst->l_qseq)) || (seq_cap > 0 && !dst->seq4) || (z->ref_bytes && !dst->ref))) {
        *why = "an indel, read or reference buffer of dst is NULL"; return BRC_E_ARG;
    }
    if (indels && z->n_slots && (!ws || ws_bytes < z->workspace_bytes)) { *why = "workspace missing or smaller than brc_join_workspace"; return BRC_E_ARG; }
    // destinations against the sources' arrays of host-known extent
    Range D[16]; int nd = 0;
    if (planes) {
        D[nd++] = range_of(dst->ncol, z->ncol_bytes); D[nd++] = range_of(dst->depth, z->depth_bytes); D[nd++] = range_of(dst->slotid, z->slotid_bytes);
        D[nd++] = range_of(dst->si, z->si_bytes); D[nd++] = range_of(dst->sf, z->sf_bytes); D[nd++] = range_of(dst->xagg, z->xagg_bytes);
    }
    if (dst && oi) {
        D[nd++] = range_of(dst->slots, z->slots_bytes); D[nd++] = range_of(dst->seq_off, z->seq_off_bytes); D[nd++] = range_of(dst->l_qseq, z->l_qseq_bytes);
        D[nd++] = range_of(dst->seq4, (uint64_t)seq_cap); D[nd++] = range_of(dst->ref, z->ref_bytes);
    }
    if (indels) { D[nd++] = range_of(ws, z->n_slots ? z->workspace_bytes : 0); D[nd++] = range_of(counts, 8); }
    D[nd++] = range_of(status, 4);
    for (int s = 0; s < K; ++s) {
        const brc_device_view* v = src[s].view; const brc_device_indels* d = src[s].indels;
        const uint64_t row = (uint64_t)v->stride * 4u, Ls = (uint64_t)v->n_lib;
        Range R[12]; int nr = 0;
        if (v->n_pos > 0) {
            R[nr++] = range_of(v->ncol, Ls * row); R[nr++] = range_of(v->depth, Ls * row); R[nr++] = range_of(v->slotid, Ls * row);
            R[nr++] = range_of(v->si, Ls * 18u * row); R[nr++] = range_of(v->sf, Ls * 8u * row);
        }
        R[nr++] = range_of(v->xagg, v->n_xagg * 64u);
        if (d) {
            R[nr++] = range_of(d->slots, d->n_slots * 72u); R[nr++] = range_of(d->seq_off, (uint64_t)d->n_reads * 8u); R[nr++] = range_of(d->l_qseq, (uint64_t)d->n_reads * 4u);
            if (d->ref) R[nr++] = range_of(d->ref, (uint64_t)(d->ref_hi - d->ref_lo));
        }
        for (int a = 0; a < nd; ++a) for (int b = 0; b < nr; ++b) if (overlap(D[a], R[b])) { *why = "a destination overlaps a source"; return BRC_E_ARG; }
    }
    return BRC_OK;
}

inline Job make_job(int32_t K, const brc_join_source* src, int32_t pos0, int64_t n, int64_t stride, const brc_join_dest* dst, bool planes, bool indels,
                    uint32_t* counts, int64_t seq_cap, uint32_t* status, void* ws, const brc_join_sizes& z) {
    Job J; memset(&J, 0, sizeof J);
    J.K = K; J.L = z.n_lib; J.pos0 = pos0; J.n = n; J.DS = stride;
    for (int s = 0; s < K; ++s) {
        const brc_device_view* v = src[s].view; const brc_device_indels* d = src[s].indels;
        Src& S = J.s[s];
        S.plane[0] = v->ncol; S.plane[1] = v->depth; S.plane[2] = v->slotid; S.plane[3] = v->si; S.plane[4] = (const uint32_t*)v->sf;
        S.d = (int64_t)pos0 - v->pos0; S.P = v->n_pos; S.PS = v->stride; S.L = v->n_lib; S.pos0 = v->pos0;
        S.xagg = (const Rec*)v->xagg;
        J.base[s + 1] = J.base[s] + v->n_lib; J.xbase[s + 1] = J.xbase[s] + v->n_xagg; J.sbase[s + 1] = J.sbase[s] + (d ? d->n_slots : 0);
        if (d) {
            S.slots = (const Slot*)d->slots; S.seq4 = d->seq4; S.seq_off = d->seq_off; S.l_qseq = d->l_qseq; S.n_reads = d->n_reads;
            S.ref = d->ref; S.ref_lo = d->ref_lo; S.ref_hi = d->ref_hi;
        }
    }
    if (planes) {
        J.o_plane[0] = dst->ncol; J.o_plane[1] = dst->depth; J.o_plane[2] = dst->slotid; J.o_plane[3] = dst->si; J.o_plane[4] = (uint32_t*)dst->sf;
        J.o_xagg = (Rec*)dst->xagg;
    }
    if (indels) {
        if (dst) { J.o_slots = (Slot*)dst->slots; J.o_seq_off = dst->seq_off; J.o_l_qseq = dst->l_qseq; J.o_seq4 = dst->seq4; J.o_ref = dst->ref; }
        J.seq_cap = seq_cap; J.o_counts = counts;
        if (z.n_slots) carve(J, ws);
    }
    J.ref_lo = z.ref_lo; J.ref_hi = z.ref_hi; J.ref_len = z.ref_len; J.status = status;
    return J;
}

// the host structs of a joined region
inline void fill_views(const Job& J, const brc_join_sizes& z, int32_t memory, int32_t device, brc_device_view* ov, brc_device_indels* oi) {
    if (ov) {
        memset(ov, 0, sizeof *ov);
        ov->memory = memory; ov->device = device; ov->n_lib = J.L; ov->pos0 = (int32_t)J.pos0; ov->n_pos = J.n; ov->stride = J.n ? J.DS : 0;
        if (J.n) {
            ov->ncol = J.o_plane[0]; ov->depth = J.o_plane[1]; ov->slotid = J.o_plane[2]; ov->si = J.o_plane[3]; ov->sf = (const float*)J.o_plane[4];
            ov->xagg = z.n_xagg ? J.o_xagg : nullptr; ov->n_xagg = z.n_xagg;
        }
    }
    if (oi) {
        memset(oi, 0, sizeof *oi);
        oi->memory = memory; oi->device = device; oi->n_lib = J.L; oi->pos0 = (int32_t)J.pos0; oi->n_pos = J.n;
        if (J.n) {
            oi->n_slots = z.n_slots; oi->n_reads = (int64_t)z.n_slots;
            if (z.n_slots) { oi->slots = J.o_slots; oi->seq4 = J.o_seq4; oi->seq_off = J.o_seq_off; oi->l_qseq = J.o_l_qseq; }
            if (z.has_ref) { oi->ref = z.ref_bytes ? J.o_ref : nullptr; oi->ref_lo = z.ref_lo; oi->ref_hi = z.ref_hi; oi->ref_len = z.ref_len; }
        }
    }
}

// bytes the host can count (brc_join_last_timing)
inline void job_bytes(const Job& J, uint64_t* rd, uint64_t* wr) {
    uint64_t r = 0, w = 0;
    if (J.o_plane[0]) {
        for (int s = 0; s < J.K; ++s) {
            const int64_t lo = J.s[s].d > 0 ? J.s[s].d : 0, hi = J.s[s].d + J.n < J.s[s].P ? J.s[s].d + J.n : J.s[s].P;
            if (hi > lo) r += 116u * (uint64_t)(hi - lo) * (uint64_t)J.s[s].L;
        }
        w += 116u * (uint64_t)J.n * (uint64_t)J.L;
        r += 64u * J.xbase[J.K]; w += 64u * J.xbase[J.K];
    }
    if (J.bytes) { r += 72u * J.sbase[J.K]; if (J.o_slots) w += (72u + 12u) * J.sbase[J.K]; }
    if (J.o_ref) {
        for (int s = 0; s < J.K; ++s) if (J.s[s].ref) r += (uint64_t)(J.s[s].ref_hi - J.s[s].ref_lo);
        w += (uint64_t)(J.ref_hi - J.ref_lo);
    }
    *rd = r; *wr = w;
}

}  // namespace brcjoin
#endif
