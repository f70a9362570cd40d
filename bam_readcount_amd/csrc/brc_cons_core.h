// brc_cons_core.h — per-lane functions of the device-side consensus caller (include/brc_cons.h), written once for the gfx950 kernels
// (brc_cons.hip) and for the CPU build the tests run (tests/cpu_cons).
//
//   link_lane     lane = third-allele record: a used record of a base bucket inside the window is pushed onto its position's list
//                 (brc_select_core.h's link_lane): a third allele's count sits only in such a record
//   record_lane   lane = table record r: ONE load of pos, lib, len, count -> the status bits; a deletion adds its count into a 32-bit
//                 difference array at the two ends of its cover, clipped to the window (O(1) whatever its length); the first record
//                 of a run puts itself into its position's run word (a minimum); an insertion inside the window walks its run, left
//                 and right, with the allele text compared bytewise, and leaves its support in the scratch
//   [scan]        the difference array -> d per position (brc_side_scan.h on the device, a serial loop in the CPU build)
//   site_lane     lane = position: ONE loop over the counted libraries — slotid and the two slots' read counts, the position's records
//                 on top (expand_lane's precedence, brc_dense_core.h) —, d from the scan, the call, the walk over the position's run
//                 for the insertion, the per-position stores
//   [scan]        the per-position lengths -> the offsets and the total
//   emit_lane     lane = position: its pieces of the sequence, each only where it fits whole
// The atomics link records, add 32-bit counts, take a minimum and OR bits: the result is a pure function of the inputs.
//
// Rec is brc_dense_core.h's restatement of the engine's record; nothing of the engine is included.
#ifndef BRC_CONS_CORE_H
#define BRC_CONS_CORE_H

#include <stdint.h>

#include "../../include/brc_cons.h"
#include "brc_dense_core.h"

namespace brccons {

using brcdense::NI;
using brcdense::NONE32;
using brcdense::put;
using brcdense::Rec;

enum { BLOCK = 256, WAVE = 64 };                           // lanes of a workgroup of every kernel = positions of a scan tile
enum { ON_WORDS = 8 };                                     // 256 bits: BRC_CONS_MAX_LIB libraries fit
enum { NCNT = BRC_CONS_NCNT };

// One call's work.  It travels BY VALUE in the kernel arguments, lib_on included: whether a library counts is a scalar test.
struct Job {
    const uint32_t *slotid, *si;                           // the view's planes, PS elements apart
    const Rec* xagg; uint64_t n_xagg;
    const char* ref; int64_t ref_lo, ref_hi, ref_len;
    int32_t Lp, pos0; int64_t PS;
    int64_t k0, n, DS, cap;                                // window [k0, k0 + n) of the planes; cnt planes DS apart; seq_cap
    int64_t m, A;                                          // table records; alleles_len
    const int32_t *pos, *lib, *len; const uint32_t *count, *aoff; const uint8_t* text;
    uint32_t flags, min_depth, min_count, num, den, ins_min_count, ins_num, ins_den, fill, gap;
    uint32_t on[ON_WORDS];
    // scratch (32-bit words): diff [n] the deletions' difference array, dcov [n + 1] its exclusive scan (d of element j = dcov[j + 1]),
    // run [n] the first record of a position's run (NONE32: none), sup [2 m] a candidate's support (low, high) — these four only with a
    // table; head [n], next [n_xagg] the positions' third-allele lists (only when the view has records); lens [n], offs [n + 1] the
    // pieces' lengths and their exclusive scan, wins [n], wcall [(n + 3) / 4] the accepted record and the call byte for emit_lane —
    // these four only without BRC_CONS_ALIGNED; part [blocks] the scans' workgroup sums; tot [1]
    uint32_t *diff, *dcov, *run, *sup, *head, *next, *lens, *offs, *wins, *part, *tot; uint8_t* wcall;
    uint32_t *o_counts, *o_cnt, *o_ins, *o_off, *status; uint8_t *o_call, *o_seq;
};

inline uint64_t blocks_of(uint64_t n) { return (n + BLOCK - 1) / BLOCK; }
inline uint64_t workspace_words(uint64_t n, uint64_t m, uint64_t X) {
    return (m ? 3 * n + 1 + 2 * m : 0) + (X ? n + X : 0) + 3 * n + 1 + (n + 3) / 4 + blocks_of(n) + 1;
}
inline int64_t workspace_bytes(const brc_device_view* v, int64_t n, int64_t m) {
    if (!v || n <= 0) return 0;
    return (int64_t)(workspace_words((uint64_t)n, m > 0 ? (uint64_t)m : 0, v->n_xagg) * 4u);
}
inline void carve(Job& J, void* ws) {
    uint32_t* w = (uint32_t*)ws; const uint64_t n = (uint64_t)J.n, m = (uint64_t)J.m, X = J.n_xagg;
    J.diff = J.dcov = J.run = J.sup = J.head = J.next = nullptr;
    if (m) { J.diff = w; w += n; J.dcov = w; w += n + 1; J.run = w; w += n; J.sup = w; w += 2 * m; }
    if (X) { J.head = w; w += n; J.next = w; w += X; }
    J.lens = w; w += n; J.offs = w; w += n + 1; J.wins = w; w += n; J.wcall = (uint8_t*)w; w += (n + 3) / 4;
    J.part = w; w += blocks_of(n); J.tot = w;
}

BRCD_HD bool counted(const Job& J, int64_t l) { return (J.on[l >> 5] >> (l & 31)) & 1u; }
BRCD_HD bool aligned(const Job& J) { return (J.flags & BRC_CONS_ALIGNED) != 0u; }

BRCD_HD uint32_t exchange(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicExch(p, v);
#else
    const uint32_t o = *p; *p = v; return o;
#endif
}
BRCD_HD void fetch_or(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicOr(p, v);
#else
    *p |= v;
#endif
}
BRCD_HD void fetch_add(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(p, v);
#else
    *p += v;
#endif
}
BRCD_HD void fetch_min(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMin(p, v);
#else
    if (v < *p) *p = v;
#endif
}

// Lane = third-allele record r (head preset to NONE32): overlay_lane's bounds (brc_dense_core.h), and a base bucket only.
BRCD_HD void link_lane(const Job& J, uint64_t r) {
    const uint32_t k = J.xagg[r].k, lb = J.xagg[r].lib_b;
    if (k == NONE32) return;
    const int64_t l = lb >> 8, j = (int64_t)k - J.k0; const uint32_t b = lb & 0xffu;
    if (l >= J.Lp || b < 1u || b > 4u || j < 0 || j >= J.n) return;
    J.next[r] = exchange(J.head + j, (uint32_t)r);
}

// text(x) of include/brc_cons.h: [*a, *a + return) inside alleles whatever allele_off holds
BRCD_HD int64_t text_of(const Job& J, int64_t x, int64_t* a) {
    int64_t a0 = J.aoff[x], a1 = J.aoff[x + 1];
    if (a0 > J.A) a0 = J.A;
    if (a1 > J.A) a1 = J.A;
    *a = a0;
    return a1 > a0 ? a1 - a0 : 0;
}
BRCD_HD bool lib_counts(const Job& J, int64_t l) { return l >= 0 && l < J.Lp && counted(J, l); }

// record x of r's run: its count where it spells r's allele (length ln, text [a, a + na)) in a counted library
BRCD_HD uint64_t same_allele(const Job& J, int64_t x, int32_t ln, int64_t a, int64_t na) {
    if (J.len[x] != ln || !lib_counts(J, J.lib[x])) return 0u;
    int64_t b;
    if (text_of(J, x, &b) != na) return 0u;
    for (int64_t i = 0; i < na; ++i) if (J.text[a + i] != J.text[b + i]) return 0u;
    return J.count[x];
}

// Lane = table record r (diff preset to 0, run to NONE32).
BRCD_HD void record_lane(const Job& J, int64_t r) {
    const int64_t p = J.pos[r], l = J.lib[r]; const int32_t ln = J.len[r];
    const bool in_lib = l >= 0 && l < J.Lp;
    const bool head = r == 0 || (int64_t)J.pos[r - 1] != p;
    if (J.status) {
        uint32_t bits = (ln != 0 && !in_lib) ? BRC_CONS_TABLE_OUT_OF_RANGE : 0u;
        if (r > 0 && (int64_t)J.pos[r - 1] > p) bits |= BRC_CONS_TABLE_NOT_ASCENDING;
        if (bits) fetch_or(J.status, bits);
    }
    const int64_t j = p - (int64_t)J.pos0 - J.k0;              // the anchor's window element
    if (head && j >= 0 && j < J.n) fetch_min(J.run + j, (uint32_t)r);
    if (ln == 0 || !in_lib || !counted(J, l)) return;
    if (ln < 0) {                                              // covers the window elements [j + 1, j + 1 + |ln|)
        int64_t lo = j + 1, hi = j + 1 - (int64_t)ln;
        if (lo < 0) lo = 0;
        if (hi > J.n) hi = J.n;
        if (lo >= hi) return;
        const uint32_t c = J.count[r];
        fetch_add(J.diff + lo, c);
        if (hi < J.n) fetch_add(J.diff + hi, 0u - c);
        return;
    }
    if (j < 0 || j >= J.n) return;
    int64_t a; const int64_t na = text_of(J, r, &a);
    uint64_t s = J.count[r];
    for (int64_t x = r - 1; x >= 0 && (int64_t)J.pos[x] == p; --x) s += same_allele(J, x, ln, a, na);
    for (int64_t x = r + 1; x < J.m && (int64_t)J.pos[x] == p; ++x) s += same_allele(J, x, ln, a, na);
    J.sup[2 * r] = (uint32_t)s; J.sup[2 * r + 1] = (uint32_t)(s >> 32);
}

// the raw reference character of plane index k by brc_select.h's rule
BRCD_HD uint32_t ref_char(const Job& J, int64_t k) {
    const int64_t p = (int64_t)J.pos0 + k;
    if (!J.ref || p < 0 || p >= J.ref_len || p < J.ref_lo || p >= J.ref_hi) return 'N';
    const uint32_t ch = (uint8_t)J.ref[p - J.ref_lo];
    return ch ? ch : (uint32_t)'N';
}

BRCD_HD bool q_ok(const Job& J, uint64_t x, uint64_t T) { return x >= J.min_count && x * J.den >= (uint64_t)J.num * T; }

// bytes the accepted record `ins` emits: its text behind the sign
BRCD_HD int64_t emitted_of(const Job& J, uint32_t ins, int64_t* a) {
    if (ins == NONE32) { *a = 0; return 0; }
    const int64_t na = text_of(J, ins, a);
    *a += 1;
    return na > 0 ? na - 1 : 0;
}

// Lane = window element j (after every link_lane and record_lane of the call and the scan of diff): the call byte.  Neighbouring
// lanes load neighbouring words of every plane — three loads per counted library, the position's records only where it has any —
// and store neighbouring words of every destination.  The byte itself is stored by the caller (packed, brc_cons.hip).
BRCD_HD uint32_t site_lane(const Job& J, int64_t j) {
    const int64_t k = J.k0 + j;
    const uint32_t first = J.head ? J.head[j] : NONE32;
    uint64_t c[4] = {0u, 0u, 0u, 0u};
    for (int l = 0; l < J.Lp; ++l) {
        if (!counted(J, l)) continue;                       // (uniform over the wave)
        const uint32_t sid = J.slotid[(int64_t)l * J.PS + k], b0 = sid & 0xffu, b1 = (sid >> 8) & 0xffu;
        const uint32_t n0 = J.si[(((int64_t)l * 2 + 0) * NI) * J.PS + k], n1 = J.si[(((int64_t)l * 2 + 1) * NI) * J.PS + k];
        uint32_t v[4];
#pragma unroll
        for (uint32_t b = 0; b < 4u; ++b) {
            uint32_t x = 0u;
            if (b0 == b + 1u && n0) x = n0;
            if (b1 == b + 1u && n1) x = n1;
            v[b] = x;
        }
        for (uint32_t r = first; r != NONE32; r = J.next[r]) {
            const uint32_t lb = J.xagg[r].lib_b;
            if ((int)(lb >> 8) != l) continue;
            const uint32_t x = J.xagg[r].i[0];
#pragma unroll
            for (uint32_t b = 0; b < 4u; ++b) if ((lb & 0xffu) == b + 1u) v[b] = x;
        }
#pragma unroll
        for (uint32_t b = 0; b < 4u; ++b) c[b] += v[b];
    }
    const uint64_t d = J.dcov ? J.dcov[j + 1] : 0u;
    const uint64_t T = c[0] + c[1] + c[2] + c[3] + d;
    uint32_t ch; bool deleted = false;
    if (T < J.min_depth) ch = NONE32;
    else if (q_ok(J, d, T) && d > c[0] && d > c[1] && d > c[2] && d > c[3]) { ch = J.gap; deleted = true; }
    else {
        uint32_t mask = 0u;
#pragma unroll
        for (uint32_t b = 0; b < 4u; ++b) if (q_ok(J, c[b], T)) mask |= 1u << b;
        ch = mask ? (uint32_t)(uint8_t)"=ACMGRSVTWYHKDBN"[mask] : NONE32;
    }
    if (ch == NONE32) ch = (J.flags & BRC_CONS_FILL_REF) ? ref_char(J, k) : J.fill;
    // the insertion behind k: one walk over the position's run
    uint32_t best = NONE32, ins = NONE32; uint64_t sbest = 0u;
    const uint32_t r0 = J.run ? J.run[j] : NONE32;
    if (r0 != NONE32) {
        const int64_t p = J.pos[r0];
        uint64_t I = 0u;
        for (int64_t x = r0; x < J.m && (int64_t)J.pos[x] == p; ++x) {
            if (J.len[x] <= 0 || !lib_counts(J, J.lib[x])) continue;
            I += J.count[x];
            const uint64_t s = (uint64_t)J.sup[2 * x] | ((uint64_t)J.sup[2 * x + 1] << 32);
            if (best == NONE32 || s > sbest) { best = (uint32_t)x; sbest = s; }
        }
        const uint64_t T2 = T + ((J.flags & BRC_CONS_INS_CENTRIC) ? I : 0u);
        if (best != NONE32 && T2 >= J.min_depth && sbest >= J.ins_min_count && sbest * J.ins_den >= (uint64_t)J.ins_num * T2) ins = best;
    }
    if (J.o_cnt) {
#pragma unroll
        for (int b = 0; b < 4; ++b) put(J.o_cnt + (int64_t)b * J.DS + j, (uint32_t)c[b]);
        put(J.o_cnt + (int64_t)BRC_CONS_C_DEL * J.DS + j, (uint32_t)d);
        put(J.o_cnt + (int64_t)BRC_CONS_C_INS * J.DS + j, (uint32_t)sbest);
    }
    if (J.o_ins) put(J.o_ins + j, ins);
    if (aligned(J)) {
        if (J.o_off) { put(J.o_off + j, (uint32_t)j); if (j + 1 == J.n) put(J.o_off + J.n, (uint32_t)J.n); }
        if (J.o_counts && j == 0) *J.o_counts = (uint32_t)J.n;
    } else {
        int64_t a;
        J.lens[j] = (deleted ? 0u : 1u) + (uint32_t)emitted_of(J, ins, &a);
        J.wins[j] = ins;
    }
    return ch;
}

// Lane = window element j (after the scan of lens): its offset and its pieces of the sequence.
BRCD_HD void emit_lane(const Job& J, int64_t j) {
    const uint64_t at = J.offs[j], total = *J.tot;
    if (J.o_off) { put(J.o_off + j, (uint32_t)at); if (j + 1 == J.n) put(J.o_off + J.n, (uint32_t)total); }
    if (!J.o_seq) return;
    const uint64_t lim = (uint64_t)J.cap < total ? (uint64_t)J.cap : total;
    int64_t a; const int64_t ne = emitted_of(J, J.wins[j], &a);
    uint64_t o = at;
    if (J.lens[j] != (uint32_t)ne) {                        // (a call byte: the position is not DELETED)
        if (o + 1u <= lim) J.o_seq[o] = J.wcall[j];
        o += 1u;
    }
    if (ne > 0 && o + (uint64_t)ne <= lim) for (int64_t i = 0; i < ne; ++i) J.o_seq[o + (uint64_t)i] = J.text[a + i];
}

// The argument checks of brc_cons_call (everything but the kind of memory, which the two libraries check themselves): 0 = fine.
inline int check_job(const brc_device_view* v, const brc_device_indels* d, const brc_cons_params* p, const brc_cons_table* t, int64_t k0, int64_t n,
                     int64_t dst_stride, int64_t seq_cap, const void* ws, const char** why) {
    if (!v || !d) { *why = "no view"; return BRC_E_ARG; }
    if (!p) { *why = "no parameters"; return BRC_E_ARG; }
    if (!t) { *why = "no table"; return BRC_E_ARG; }
    if (v->n_lib < 1 || v->n_pos < 0 || v->stride < v->n_pos || d->n_lib < 1 || d->n_pos < 0) { *why = "not a view of a computed region"; return BRC_E_ARG; }
    if (v->memory != d->memory || v->device != d->device || v->n_lib != d->n_lib || v->pos0 != d->pos0 || v->n_pos != d->n_pos) {
        *why = "the two views are not of one region"; return BRC_E_ARG;
    }
    if (v->n_lib > BRC_CONS_MAX_LIB) { *why = "more libraries than BRC_CONS_MAX_LIB"; return BRC_E_ARG; }
    if (k0 < 0 || n < 0 || k0 > v->n_pos || n > v->n_pos - k0) { *why = "the window must lie inside the view's planes"; return BRC_E_ARG; }
    if (n > 0 && (!v->ncol || !v->depth || !v->slotid || !v->si || !v->sf)) { *why = "a view without planes"; return BRC_E_ARG; }
    if (v->n_xagg && !v->xagg) { *why = "a view without its third-allele records"; return BRC_E_ARG; }
    if (d->n_slots && (!d->slots || !d->seq4 || !d->seq_off || !d->l_qseq || d->n_reads < 0)) { *why = "a view with records but without its arrays"; return BRC_E_ARG; }
    if (dst_stride < n) { *why = "dst_stride below n"; return BRC_E_ARG; }
    if (seq_cap < 0) { *why = "negative capacity"; return BRC_E_ARG; }
    if (t->m < 0 || t->stride < t->m) { *why = "a table with m below 0 or stride below m"; return BRC_E_ARG; }
    if (t->alleles_len < 0) { *why = "alleles_len below 0"; return BRC_E_ARG; }
    if (t->m > 0 && (!t->pos || !t->lib || !t->len || !t->count || !t->allele_off || !t->alleles)) { *why = "a table without its arrays"; return BRC_E_ARG; }
    if ((uint64_t)t->m >= 0x7ffffff0ull || v->n_xagg >= 0xfffffff0ull || (uint64_t)n >= 0x7ffffff0ull || (uint64_t)n + (uint64_t)t->alleles_len >= 0xfffffff0ull) {
        *why = "window or table too large: records, positions and sequence bytes are indexed with 32 bits"; return BRC_E_ARG;
    }
    if (p->flags & ~(BRC_CONS_ALIGNED | BRC_CONS_FILL_REF | BRC_CONS_INS_CENTRIC)) { *why = "flags: BRC_CONS_ALIGNED | BRC_CONS_FILL_REF | BRC_CONS_INS_CENTRIC"; return BRC_E_ARG; }
    if (p->den < 1u || p->den > 65535u || p->ins_den < 1u || p->ins_den > 65535u) { *why = "den and ins_den must lie in [1, 65535]"; return BRC_E_ARG; }
    if (p->num > p->den || p->ins_num > p->ins_den) { *why = "a fraction above 1"; return BRC_E_ARG; }
    if (p->fill > 255u || p->gap > 255u) { *why = "fill and gap are characters: 0 .. 255"; return BRC_E_ARG; }
    bool any = !p->lib_on;
    for (int l = 0; p->lib_on && l < v->n_lib; ++l) {
        if (p->lib_on[l] > 1) { *why = "a lib_on byte above 1"; return BRC_E_ARG; }
        any = any || p->lib_on[l];
    }
    if (!any) { *why = "no counted library"; return BRC_E_ARG; }
    if (n > 0 && !ws) { *why = "no workspace"; return BRC_E_ARG; }
    return BRC_OK;
}
inline Job make_job(const brc_device_view* v, const brc_device_indels* d, const brc_cons_params* p, const brc_cons_table* t, int64_t k0, int64_t n,
                    int64_t dst_stride, int64_t seq_cap, uint32_t* counts, uint8_t* call, uint32_t* cnt, uint32_t* ins_rec, uint32_t* off, uint8_t* seq,
                    uint32_t* status, void* ws) {
    Job J;
    J.slotid = v->slotid; J.si = v->si; J.xagg = (const Rec*)v->xagg; J.n_xagg = v->n_xagg;
    J.ref = d->ref; J.ref_lo = d->ref_lo; J.ref_hi = d->ref_hi; J.ref_len = d->ref_len;
    J.Lp = v->n_lib; J.pos0 = v->pos0; J.PS = v->stride; J.k0 = k0; J.n = n; J.DS = dst_stride; J.cap = seq_cap;
    J.m = t->m; J.A = t->alleles_len;
    J.pos = t->pos; J.lib = t->lib; J.len = t->len; J.count = t->count; J.aoff = t->allele_off; J.text = t->alleles;
    J.flags = p->flags; J.min_depth = p->min_depth; J.min_count = p->min_count; J.num = p->num; J.den = p->den;
    J.ins_min_count = p->ins_min_count; J.ins_num = p->ins_num; J.ins_den = p->ins_den; J.fill = p->fill; J.gap = p->gap;
    for (int w = 0; w < ON_WORDS; ++w) J.on[w] = 0u;
    for (int l = 0; l < v->n_lib; ++l) if (!p->lib_on || p->lib_on[l]) J.on[l >> 5] |= 1u << (l & 31);
    carve(J, ws);
    J.o_counts = counts; J.o_call = call; J.o_cnt = cnt; J.o_ins = ins_rec; J.o_off = off; J.o_seq = seq; J.status = status;
    return J;
}
inline bool walks_records(const Job& J) { return J.head != nullptr; }
inline bool walks_table(const Job& J) { return J.m > 0; }
// the per-position sweep runs for every destination but a status word alone
inline bool wants_sites(const Job& J) { return J.o_counts || J.o_call || J.o_cnt || J.o_ins || J.o_off || J.o_seq; }
// (without BRC_CONS_ALIGNED) the lengths are scanned for counts, off and seq; the emit runs for the last two
inline bool wants_scan(const Job& J) { return !aligned(J) && (J.o_counts || J.o_off || J.o_seq); }
inline bool wants_emit(const Job& J) { return !aligned(J) && (J.o_off || J.o_seq); }
// bytes the sweeps ask for / write (brc_cons_last_timing): functions of n, m, the libraries and the destinations alone
inline void job_bytes(const Job& J, uint64_t* rd, uint64_t* wr) {
    const uint64_t n = (uint64_t)J.n, m = (uint64_t)J.m, chain = walks_records(J) ? 1u : 0u, tab = m ? 1u : 0u, al = aligned(J) ? 1u : 0u;
    const uint64_t scan = wants_scan(J) ? 1u : 0u, emit = wants_emit(J) ? 1u : 0u;
    uint64_t L = 0;
    for (int l = 0; l < J.Lp; ++l) L += counted(J, l);
    *rd = 4u * n * (3u * L + chain + 4u * tab + 2u * scan + 3u * emit) + n * ((J.flags & BRC_CONS_FILL_REF) ? 1u : 0u) + n * emit + 64u * J.n_xagg * chain + 24u * m;
    *wr = 4u * n * (chain + 2u * tab + (1u - al) * 2u + scan + (J.o_cnt ? (uint64_t)NCNT : 0u) + (J.o_ins ? 1u : 0u) + (J.o_off ? 1u : 0u)) +
          n * ((J.o_call ? 1u : 0u) + (1u - al) + (J.o_seq ? 1u : 0u)) + 4u * (J.n_xagg * chain + 2u * m + 2u * blocks_of(n) + 2u);
}

}  // namespace brccons
#endif
