// brc_indels_core.h — per-lane functions of the device-resident indel table (include/brc_indels.h), written once for the gfx950 kernels
// (brc_indels.hip) and for the CPU build the tests run (tests/sim_indels): what assemble_indels (brc_host.cpp) does on the host — spell
// every allele, sort by (position, library, allele text) — as a counting sort by position followed by a rank inside each position's run.
//
//   count_lane   lane = slot: a live record inside the window counts itself at its position             (atomic)
//   [scan]       cnt[] -> run starts off[], total -> counts[0]
//   place_lane   lane = slot: the slot index goes into its position's run, anywhere in it                (atomic cursor)
//   rank_lane    lane = placed record: how many peers of its run come before it by (library, allele text, slot index) -> its final
//                index off[p] + rank: unique and independent of where place_lane put anything
//   [scan]       |len| + 1 in final order -> allele_off[], total -> counts[1]
//   emit_lane    lane = final record: the structure-of-arrays stores (neighbouring lanes store neighbouring elements), the thirteen
//                columns, the allele bytes
// The two scans are cooperative on the device (brc_indels.hip: reduce, scan of the partials, apply — three launches each) and a
// serial loop in the CPU build; everything else is the same code.
//
// The record layout is struct IndelOut of brc_core.h, restated here so that this header includes nothing of the engine: the view
// (brc_device_indels, include/brc.h) is plain data.
#ifndef BRC_INDELS_CORE_H
#define BRC_INDELS_CORE_H

#include <stdint.h>

#include "../../include/brc_indels.h"
#include "brc_dense_core.h"      // metrics13, put

#if defined(__HIPCC__)
#define BRC_HD __host__ __device__ inline
#else
#define BRC_HD inline
#endif

namespace brcindels {

using brcdense::NI; using brcdense::NF; using brcdense::NM;

struct Slot { int32_t pos, lib, len; uint32_t rep_read; int32_t rep_qpos; uint32_t i[NI]; float f[NF]; };
static_assert(sizeof(Slot) == 72, "an indel record is 72 bytes");

enum { SCAN_TILE = 256 };        // elements per workgroup of a scan = the block size of every kernel

// One call's work: the view, the window, the scratch, the destinations (any of them nullptr: not wanted).
struct Job {
    const Slot* slots; uint64_t n_slots;
    const uint8_t* seq4; const uint64_t* seq_off; const int32_t* l_qseq; int64_t n_reads;
    const char* ref; int64_t ref_lo, ref_hi, ref_len;
    int64_t first, n;                // the window: reference positions [first, first + n)
    int64_t cap, acap;
    // scratch (32-bit words): cnt [n] records per position (counted up by count_lane, down again by place_lane), off [n + 1] run starts,
    // placed [S] slot indices grouped by position, order [S] slot index of final record r, alen [S] its text length, aoff [S + 1] the
    // text offsets, part [.] the scans' workgroup partials, tot [2] = counts
    uint32_t *cnt, *off, *placed, *order, *alen, *aoff, *part, *tot;
    uint32_t* o_counts;
    int32_t *o_pos, *o_lib, *o_len; uint32_t* o_rep_read; int32_t* o_rep_qpos;
    uint32_t* o_istat; float *o_fstat, *o_metrics;
    uint32_t* o_aoff; uint8_t* o_alleles;
};

inline uint64_t scan_blocks(uint64_t n) { return (n + SCAN_TILE - 1) / SCAN_TILE; }
// words of scratch for a window of n positions of a view with S slots
inline uint64_t workspace_words(uint64_t n, uint64_t S) {
    const uint64_t nb = scan_blocks(n > S ? n : S) + 1;
    return n + (n + 1) + S + S + S + (S + 1) + nb + 2;
}
inline size_t workspace_bytes(const brc_device_indels* v, int64_t n) {
    if (!v || n <= 0 || v->n_slots == 0) return 0;
    return (size_t)(workspace_words((uint64_t)n, v->n_slots) * 4u);
}
inline void carve(Job& J, void* ws) {
    uint32_t* w = (uint32_t*)ws; const uint64_t n = (uint64_t)J.n, S = J.n_slots;
    J.cnt = w; w += n; J.off = w; w += n + 1; J.placed = w; w += S; J.order = w; w += S; J.alen = w; w += S; J.aoff = w; w += S + 1;
    J.part = w; w += scan_blocks(n > S ? n : S) + 1; J.tot = w;
}

// fetch-and-add / fetch-and-subtract on a scratch word: device-scope atomics in the kernels, plain arithmetic in the serial CPU build
BRC_HD uint32_t fetch_add(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicAdd(p, v);
#else
    const uint32_t o = *p; *p = o + v; return o;
#endif
}
BRC_HD uint32_t fetch_sub(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicSub(p, v);
#else
    const uint32_t o = *p; *p = o - v; return o;
#endif
}

// window element of a slot, or -1: unused (len == 0) or outside the window
BRC_HD int64_t window_index(const Job& J, uint64_t s) {
    const Slot& o = J.slots[s];
    if (o.len == 0) return -1;
    const int64_t d = (int64_t)o.pos - J.first;
    return (d >= 0 && d < J.n) ? d : -1;
}

BRC_HD void count_lane(const Job& J, uint64_t s) {
    const int64_t d = window_index(J, s);
    if (d >= 0) (void)fetch_add(J.cnt + d, 1u);
}

// (after the scan of cnt: off[d] is the start of position d's run, cnt[d] its length — counted down here, so the scratch ends as zeros)
BRC_HD void place_lane(const Job& J, uint64_t s) {
    const int64_t d = window_index(J, s);
    if (d < 0) return;
    const uint32_t k = fetch_sub(J.cnt + d, 1u) - 1u;
    J.placed[J.off[d] + k] = (uint32_t)s;
}

// character j of a record's allele text behind its sign (bamreadcount.cpp:324-338; allele_char of brc_core.h, from the uploaded SEQ
// instead of the engine's event bytes): an inserted base as "=ACGTN"[canonical code] ('N' past the read's end), a deleted one as the
// reference's raw character ('N' where there is none)
BRC_HD char allele_char(const Job& J, const Slot& o, int j) {
    if (o.len > 0) {
        if ((int64_t)o.rep_read >= J.n_reads) return 'N';
        const int64_t q = (int64_t)o.rep_qpos + 1 + j;
        if (q < 0 || q >= (int64_t)J.l_qseq[o.rep_read]) return 'N';
        const uint8_t* seq = J.seq4 + J.seq_off[o.rep_read];
        const uint32_t b4 = (seq[q >> 1] >> ((~q & 1) << 2)) & 0xfu;
        const char bases[] = "=ACGTN";
        return bases[(0x5555555455535210ull >> (b4 * 4)) & 15u];            // canon_bucket of brc_core.h
    }
    const int64_t p = (int64_t)o.pos + 1 + j;
    const char rc = (J.ref && p >= 0 && p < J.ref_len && p >= J.ref_lo && p < J.ref_hi) ? J.ref[p - J.ref_lo] : (char)0;
    return rc ? rc : 'N';
}

BRC_HD int abs_len(const Slot& o) { return o.len < 0 ? -o.len : o.len; }

// order of two records of ONE position: library, then the allele texts as std::string compares them ('+' before '-', bytewise, a
// prefix before the longer text; deletions at one position are prefixes of one another: the shorter first).  < 0: a first.
BRC_HD int compare(const Job& J, const Slot& a, const Slot& b) {
    if (a.lib != b.lib) return a.lib < b.lib ? -1 : 1;
    if ((a.len > 0) != (b.len > 0)) return a.len > 0 ? -1 : 1;
    const int la = abs_len(a), lb = abs_len(b);
    if (a.len > 0) {
        const int n = la < lb ? la : lb;
        for (int j = 0; j < n; ++j) {
            const unsigned char ca = (unsigned char)allele_char(J, a, j), cb = (unsigned char)allele_char(J, b, j);
            if (ca != cb) return ca < cb ? -1 : 1;
        }
    }
    return la < lb ? -1 : (la > lb ? 1 : 0);
}

// Lane = placed record j: its rank among the records of its position's run.  The alleles of one (position, library) are distinct, so
// `compare` alone orders a run; the slot index breaks a tie all the same, so that the final indices are a permutation whatever the
// records hold.  Quadratic in the run's length: a run is the handful of alleles of one position.
BRC_HD void rank_lane(const Job& J, uint64_t j) {
    if (j >= (uint64_t)J.tot[0]) return;
    const uint32_t s = J.placed[j];
    const Slot& o = J.slots[s];
    const int64_t d = (int64_t)o.pos - J.first;
    const uint32_t lo = J.off[d], hi = J.off[d + 1];
    uint32_t rank = 0;
    for (uint32_t t = lo; t < hi; ++t) {
        if (t == (uint32_t)j) continue;
        const uint32_t st = J.placed[t];
        const int c = compare(J, J.slots[st], o);
        if (c < 0 || (c == 0 && st < s)) ++rank;
    }
    J.order[lo + rank] = s;
    J.alen[lo + rank] = (uint32_t)abs_len(o) + 1u;
}

// Lane = final index r in [0, M]: lane M only closes the offsets; a record at or behind `cap` stores nothing, its text included.
BRC_HD void emit_lane(const Job& J, uint64_t r) {
    const uint64_t M = J.tot[0];
    if (r > M) return;
    const uint32_t a0 = J.aoff[r];
    if (J.o_aoff && (int64_t)r <= J.cap) brcdense::put(J.o_aoff + r, a0);
    if (r == M || (int64_t)r >= J.cap) return;
    const Slot o = J.slots[J.order[r]];
    if (J.o_pos) brcdense::put(J.o_pos + r, o.pos);
    if (J.o_lib) brcdense::put(J.o_lib + r, o.lib);
    if (J.o_len) brcdense::put(J.o_len + r, o.len);
    if (J.o_rep_read) brcdense::put(J.o_rep_read + r, o.rep_read);
    if (J.o_rep_qpos) brcdense::put(J.o_rep_qpos + r, o.rep_qpos);
    if (J.o_istat) for (int f = 0; f < NI; ++f) brcdense::put(J.o_istat + (int64_t)f * J.cap + (int64_t)r, o.i[f]);
    if (J.o_fstat) for (int f = 0; f < NF; ++f) brcdense::put(J.o_fstat + (int64_t)f * J.cap + (int64_t)r, o.f[f]);
    if (J.o_metrics) {
        float m[NM];
        brcdense::metrics13(o.i, o.f, m);
        for (int f = 0; f < NM; ++f) brcdense::put(J.o_metrics + (int64_t)f * J.cap + (int64_t)r, m[f]);
    }
    const uint32_t n = (uint32_t)abs_len(o);
    if (J.o_alleles && (uint64_t)a0 + n + 1u <= (uint64_t)J.acap) {
        uint8_t* w = J.o_alleles + a0;
        w[0] = (uint8_t)(o.len > 0 ? '+' : '-');
        for (uint32_t j = 0; j < n; ++j) w[1 + j] = (uint8_t)allele_char(J, o, (int)j);
    }
}

// The argument checks of brc_indels_gather (everything but the kind of memory, which the two libraries check themselves): 0 = fine.
inline int check_job(const brc_device_indels* v, int64_t k0, int64_t n, int64_t cap, int64_t acap, const void* ws, size_t ws_bytes, const char** why) {
    if (!v) { *why = "no view"; return BRC_E_ARG; }
    if (v->n_lib < 1 || v->n_pos < 0) { *why = "not a view of a computed region"; return BRC_E_ARG; }
    if (k0 < 0 || n < 0 || k0 > v->n_pos || n > v->n_pos - k0) { *why = "the window must lie inside the view's positions"; return BRC_E_ARG; }
    if (cap < 0 || acap < 0) { *why = "negative capacity"; return BRC_E_ARG; }
    if (v->n_slots && (!v->slots || !v->seq4 || !v->seq_off || !v->l_qseq || v->n_reads < 0)) { *why = "a view with records but without its arrays"; return BRC_E_ARG; }
    if (v->n_slots >= 0xfffffff0ull || (uint64_t)n >= 0xfffffff0ull) { *why = "window too large: records and positions are indexed with 32 bits"; return BRC_E_ARG; }
    const size_t need = workspace_bytes(v, n);
    if (need && (!ws || ws_bytes < need)) { *why = "workspace missing or smaller than brc_indels_workspace"; return BRC_E_ARG; }
    return BRC_OK;
}
inline Job make_job(const brc_device_indels* v, int64_t k0, int64_t n, void* ws, uint32_t* counts, int64_t cap, int64_t acap, int32_t* pos, int32_t* lib,
                    int32_t* len, uint32_t* rep_read, int32_t* rep_qpos, uint32_t* istat, float* fstat, float* metrics, uint32_t* allele_off, uint8_t* alleles) {
    Job J;
    J.slots = (const Slot*)v->slots; J.n_slots = v->n_slots;
    J.seq4 = v->seq4; J.seq_off = v->seq_off; J.l_qseq = v->l_qseq; J.n_reads = v->n_reads;
    J.ref = v->ref; J.ref_lo = v->ref_lo; J.ref_hi = v->ref_hi; J.ref_len = v->ref_len;
    J.first = (int64_t)v->pos0 + k0; J.n = n; J.cap = cap; J.acap = acap;
    carve(J, ws);
    J.o_counts = counts; J.o_pos = pos; J.o_lib = lib; J.o_len = len; J.o_rep_read = rep_read; J.o_rep_qpos = rep_qpos;
    J.o_istat = istat; J.o_fstat = fstat; J.o_metrics = metrics; J.o_aoff = allele_off; J.o_alleles = alleles;
    return J;
}
inline bool wants_records(const Job& J) {
    return J.o_pos || J.o_lib || J.o_len || J.o_rep_read || J.o_rep_qpos || J.o_istat || J.o_fstat || J.o_metrics || J.o_aoff || J.o_alleles;
}
// bytes the two sweeps over the slots read / the scratch bytes every call writes (brc_indels_last_timing)
inline void job_bytes(const Job& J, uint64_t* rd, uint64_t* wr) {
    *rd = 2u * 72u * J.n_slots + 4u * 3u * (uint64_t)J.n;
    *wr = 4u * (3u * (uint64_t)J.n + 1u);
}

}  // namespace brcindels
#endif
