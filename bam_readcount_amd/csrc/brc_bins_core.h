// brc_bins_core.h — per-lane functions of the device-side window summaries (include/brc_bins.h), written once for the gfx950 kernels
// (brc_bins.hip) and for the CPU build the tests run (tests/sim_bins).
//
//   clear_lane   lane = destination element: the n_bins elements of every wanted row, the histogram, the status word -> 0
//   edge_lane    lane = edge of an edge list: an edge outside the window, a neighbour that descends -> a bit of the status word
//   plane_lane   lane = (window element, library): the bin of the position and what it adds to it — depth, ncol, the six buckets' read
//                counts from the two slots (expand_lane's precedence), the non-reference reads (brcselect::ref_bucket: the selector's
//                reference rule)
//   commit_lane  lane = the same: its values into its bin, one 64-bit atomic per non-zero value.  On the device a wave whose 64
//                positions share one bin reduces across its lanes first (brc_bins.hip: wave_commit) and adds once per value
//   record_lane  lane = third-allele record: a used record inside the window adds (its count - the slots' count of its bucket) to its
//                bin — modulo 2^64, so the sum ends as if the record had taken the bucket's place, whatever ran first
//   indel_lane   lane = indel record: a live record inside the window adds its reads to its library's insertion or deletion sum
// Every store is an integer add, an integer maximum or an OR: their order changes nothing, the result is a pure function of the inputs.
//
// Rec and Slot are brc_dense_core.h's and brc_indels_core.h's restatements of the engine's records; nothing of the engine is included.
#ifndef BRC_BINS_CORE_H
#define BRC_BINS_CORE_H

#include <stdint.h>

#include "../../include/brc_bins.h"
#include "brc_select_core.h"

namespace brcbins {

using brcdense::NB;
using brcdense::NI;
using brcdense::NONE32;
using brcdense::Rec;
using brcindels::Slot;

enum { BLOCK = 256, WAVE = 64 };                           // lanes of a workgroup of every kernel; a wave = 64 consecutive positions
enum { NSUM = BRC_BINS_NSUM, NADD = 9, MAX_THR = BRC_BINS_MAX_THR };      // sums 0..8 are what a position adds; 9, 10 come from records

// One call's work.  It travels BY VALUE in the kernel arguments, the thresholds included.
struct Job {
    const uint32_t *ncol, *depth, *slotid, *si;            // the view's planes, PS elements apart
    const Rec* xagg; uint64_t n_xagg;
    const Slot* slots; uint64_t n_slots;
    const char* ref; int64_t ref_lo, ref_hi, ref_len;
    int32_t Lp, pos0; int64_t P, PS;
    int64_t k0, n;                                         // window [k0, k0 + n) of the planes
    const int32_t* edges; uint32_t width; int64_t n_bins, DS;            // edges == nullptr: uniform bins of `width` positions
    int32_t n_thr, n_hist; uint32_t thr[MAX_THR];
    uint64_t *o_sums, *o_cov, *o_hist; uint32_t* o_status;
};

inline uint64_t blocks_of(uint64_t n) { return (n + BLOCK - 1) / BLOCK; }

BRCD_HD void add64(uint64_t* p, uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd((unsigned long long*)p, (unsigned long long)v);
#else
    *p += v;
#endif
}
BRCD_HD void max64(uint64_t* p, uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMax((unsigned long long*)p, (unsigned long long)v);
#else
    if (*p < v) *p = v;
#endif
}

BRCD_HD bool wants_sums(const Job& J) { return J.o_sums != nullptr; }
BRCD_HD bool wants_cov(const Job& J) { return J.o_cov != nullptr && J.n_thr > 0; }
BRCD_HD bool wants_hist(const Job& J) { return J.o_hist != nullptr && J.n_hist > 0; }

// destination elements a call clears: the rows' first n_bins elements, the histogram, the status word
BRCD_HD uint64_t clear_total(const Job& J) {
    const uint64_t nb = (uint64_t)J.n_bins, L = (uint64_t)J.Lp;
    return (wants_sums(J) ? L * NSUM * nb : 0u) + (wants_cov(J) ? L * (uint64_t)J.n_thr * nb : 0u) + (wants_hist(J) ? L * (uint64_t)J.n_hist : 0u) + 1u;
}
BRCD_HD void clear_lane(const Job& J, uint64_t i) {
    const uint64_t nb = (uint64_t)J.n_bins, L = (uint64_t)J.Lp;
    const uint64_t a = wants_sums(J) ? L * NSUM * nb : 0u, c = wants_cov(J) ? L * (uint64_t)J.n_thr * nb : 0u, h = wants_hist(J) ? L * (uint64_t)J.n_hist : 0u;
    if (i < a) { J.o_sums[(i / nb) * (uint64_t)J.DS + i % nb] = 0u; return; }
    i -= a;
    if (i < c) { J.o_cov[(i / nb) * (uint64_t)J.DS + i % nb] = 0u; return; }
    i -= c;
    if (i < h) { J.o_hist[i] = 0u; return; }
    if (i == h && J.o_status) *J.o_status = 0u;
}

// Lane = edge i in [0, n_bins] (after the status word's clear_lane)
BRCD_HD void edge_lane(const Job& J, uint64_t i) {
    const int64_t e = J.edges[i];
    uint32_t bits = 0u;
    if (e < J.k0 || e > J.k0 + J.n) bits |= BRC_BINS_OUTSIDE;
    if ((int64_t)i < J.n_bins && (int64_t)J.edges[i + 1] < e) bits |= BRC_BINS_DESCENDS;
    if (bits && J.o_status) brcselect::fetch_or(J.o_status, bits);
}

// bin of plane index k of the window (k0 <= k < k0 + n, n_bins > 0), or -1.  An edge list is searched for the number of
// edges[1 .. n_bins] that are <= k: at most 32 steps and only elements of the list are read, whatever the list holds; an edge outside
// the window needs no clipping here — below k0 it is <= every k of the window, above k0 + n it is > every k — and a descending
// list gives some b in [0, n_bins], of which n_bins means none.
BRCD_HD int64_t bin_of(const Job& J, int64_t k) {
    if (!J.edges) return (int64_t)((uint32_t)(k - J.k0) / J.width);
    const uint32_t nb = (uint32_t)J.n_bins;
    if (k < (int64_t)J.edges[0] || k >= (int64_t)J.edges[nb]) return -1;
    uint32_t lo = 0u, hi = nb;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if ((int64_t)J.edges[mid + 1u] <= k) lo = mid + 1u; else hi = mid;
    }
    return lo < nb ? (int64_t)lo : -1;
}

// The selector's reference rule itself (brcselect::ref_bucket), given the five fields it reads: base bucket 1..4 of the reference
// character of plane index k, 0: none of ACGTacgt.
BRCD_HD uint32_t ref_bucket(const Job& J, int64_t k) {
    brcselect::Job S;
    S.ref = J.ref; S.ref_lo = J.ref_lo; S.ref_hi = J.ref_hi; S.ref_len = J.ref_len; S.pos0 = J.pos0;
    return brcselect::ref_bucket(S, k);
}

// The read count of a bucket after expand_lane's writes (brc_dense_core.h: zero; slot 0 where it names the bucket and counts reads;
// slot 1 likewise, the later write winning).  expand_lane and the selector's why_lane spell this inside their loops; taking it out of
// them changes the register allocation of their kernels, whose objects the committed measurements name, so it stands here once for
// plane_lane and record_lane.
BRCD_HD uint32_t slot_value(bool in0, uint32_t s0, bool in1, uint32_t s1) {
    uint32_t v = 0u;
    if (in0 && s0) v = s0;
    if (in1 && s1) v = s1;
    return v;
}

// what one position of one library adds to its bin
struct Lane { int64_t bin; uint32_t depth; uint32_t add[NADD]; };

// Lane = window element j of library l.  Neighbouring lanes load neighbouring words of every plane: depth alone when only covered or
// hist is wanted, five words and the reference byte for the sums.
BRCD_HD Lane plane_lane(const Job& J, int l, int64_t j) {
    Lane o;
    const int64_t k = J.k0 + j, row = (int64_t)l * J.PS + k;
    o.bin = bin_of(J, k);
    o.depth = J.depth[row];
#pragma unroll
    for (int s = 0; s < NADD; ++s) o.add[s] = 0u;
    if (!wants_sums(J) || o.bin < 0) return o;
    o.add[BRC_BINS_S_DEPTH] = o.depth;
    o.add[BRC_BINS_S_NCOL] = J.ncol[row];
    const uint32_t sid = J.slotid[row], b0 = sid & 0xffu, b1 = (sid >> 8) & 0xffu;
    const uint32_t n0 = J.si[(((int64_t)l * 2 + 0) * NI) * J.PS + k], n1 = J.si[(((int64_t)l * 2 + 1) * NI) * J.PS + k];
    const uint32_t rb = ref_bucket(J, k);
    uint32_t nonref = 0u;
#pragma unroll
    for (uint32_t b = 0; b < (uint32_t)NB; ++b) {
        const uint32_t v = slot_value(b0 == b, n0, b1 == b, n1);
        o.add[BRC_BINS_S_BUCKET + b] = v;
        if (b >= 1u && b <= 4u && rb && b != rb) nonref += v;
    }
    o.add[BRC_BINS_S_NONREF] = nonref;
    return o;
}

BRCD_HD uint32_t hist_bar(const Job& J, uint32_t depth) { return depth < (uint32_t)J.n_hist ? depth : (uint32_t)J.n_hist - 1u; }

// Lane = the same (cleared destinations): its values into its bin
BRCD_HD void commit_lane(const Job& J, int l, const Lane& o) {
    if (o.bin < 0) return;
    if (wants_sums(J)) {
        uint64_t* base = J.o_sums + ((int64_t)l * NSUM) * J.DS + o.bin;
#pragma unroll
        for (int s = 0; s < NADD; ++s) if (o.add[s]) add64(base + (int64_t)s * J.DS, o.add[s]);
        if (o.depth) max64(base + (int64_t)BRC_BINS_S_MAXDEPTH * J.DS, o.depth);
    }
    if (wants_cov(J))
        for (int t = 0; t < J.n_thr; ++t) if (o.depth >= J.thr[t]) add64(J.o_cov + ((int64_t)l * J.n_thr + t) * J.DS + o.bin, 1u);
}

// Lane = third-allele record r: overlay_lane's bounds (brc_dense_core.h)
BRCD_HD void record_lane(const Job& J, uint64_t r) {
    const uint32_t k32 = J.xagg[r].k, lb = J.xagg[r].lib_b;
    if (k32 == NONE32) return;
    const int64_t l = lb >> 8, k = k32; const uint32_t b = lb & 0xffu;
    if (l >= J.Lp || b >= (uint32_t)NB || k >= J.P || k < J.k0 || k >= J.k0 + J.n) return;
    const int64_t bin = bin_of(J, k);
    if (bin < 0) return;
    const uint32_t sid = J.slotid[l * J.PS + k], b0 = sid & 0xffu, b1 = (sid >> 8) & 0xffu;
    const uint32_t n0 = J.si[((l * 2 + 0) * NI) * J.PS + k], n1 = J.si[((l * 2 + 1) * NI) * J.PS + k];
    const uint64_t delta = (uint64_t)J.xagg[r].i[0] - (uint64_t)slot_value(b0 == b, n0, b1 == b, n1);
    if (!delta) return;
    uint64_t* base = J.o_sums + (l * NSUM) * J.DS + bin;
    add64(base + (int64_t)(BRC_BINS_S_BUCKET + b) * J.DS, delta);
    if (b >= 1u && b <= 4u) {
        const uint32_t rb = ref_bucket(J, k);
        if (rb && rb != b) add64(base + (int64_t)BRC_BINS_S_NONREF * J.DS, delta);
    }
}

// Lane = indel record s
BRCD_HD void indel_lane(const Job& J, uint64_t s) {
    const Slot& o = J.slots[s];
    const int32_t len = o.len, lib = o.lib;
    if (len == 0 || lib < 0 || lib >= J.Lp) return;
    const int64_t k = (int64_t)o.pos - J.pos0;
    if (k < J.k0 || k >= J.k0 + J.n) return;
    const int64_t bin = bin_of(J, k);
    if (bin < 0 || !o.i[0]) return;
    add64(J.o_sums + ((int64_t)lib * NSUM + (len > 0 ? BRC_BINS_S_INS : BRC_BINS_S_DEL)) * J.DS + bin, o.i[0]);
}

BRCD_HD bool walks_records(const Job& J) { return wants_sums(J) && J.n_xagg; }
BRCD_HD bool walks_slots(const Job& J) { return wants_sums(J) && J.n_slots; }

inline int64_t bins_of(const brc_bins_params* p, int64_t n) { return p->edges ? p->n_bins : (n > 0 ? (n - 1) / p->width + 1 : 0); }

// The argument checks of brc_bins_reduce (everything but the kind of memory, which the two libraries check themselves): 0 = fine.
inline int check_job(const brc_device_view* v, const brc_device_indels* d, const brc_bins_params* p, int64_t k0, int64_t n, int64_t dst_stride,
                     const char** why) {
    if (!v || !d) { *why = "no view"; return BRC_E_ARG; }
    if (!p) { *why = "no parameters"; return BRC_E_ARG; }
    if (v->n_lib < 1 || v->n_pos < 0 || v->stride < v->n_pos || d->n_lib < 1 || d->n_pos < 0) { *why = "not a view of a computed region"; return BRC_E_ARG; }
    if (v->memory != d->memory || v->device != d->device || v->n_lib != d->n_lib || v->pos0 != d->pos0 || v->n_pos != d->n_pos) {
        *why = "the two views are not of one region"; return BRC_E_ARG;
    }
    if (v->n_lib > BRC_BINS_MAX_LIB) { *why = "more libraries than BRC_BINS_MAX_LIB"; return BRC_E_ARG; }
    if (k0 < 0 || n < 0 || k0 > v->n_pos || n > v->n_pos - k0) { *why = "the window must lie inside the view's planes"; return BRC_E_ARG; }
    if (n > 0 && (!v->ncol || !v->depth || !v->slotid || !v->si || !v->sf)) { *why = "a view without planes"; return BRC_E_ARG; }
    if (v->n_xagg && !v->xagg) { *why = "a view without its third-allele records"; return BRC_E_ARG; }
    if (d->n_slots && (!d->slots || !d->seq4 || !d->seq_off || !d->l_qseq || d->n_reads < 0)) { *why = "a view with records but without its arrays"; return BRC_E_ARG; }
    if (d->n_slots >= 0xfffffff0ull || v->n_xagg >= 0xfffffff0ull) { *why = "too many records: they are indexed with 32 bits"; return BRC_E_ARG; }
    if (k0 + n > (int64_t)INT32_MAX) { *why = "the window ends behind plane index 2^31 - 1: edges have 32 bits"; return BRC_E_ARG; }
    if (p->width < 0) { *why = "negative width"; return BRC_E_ARG; }
    if (p->width == 0 && !p->edges) { *why = "neither a width nor an edge list"; return BRC_E_ARG; }
    if (p->width > 0 && p->edges) { *why = "both a width and an edge list"; return BRC_E_ARG; }
    if (p->n_bins < 0 || p->n_bins > (int64_t)INT32_MAX - 1) { *why = "n_bins: 0 .. 2^31 - 2"; return BRC_E_ARG; }
    if (p->n_thr < 0 || p->n_thr > BRC_BINS_MAX_THR) { *why = "n_thr: 0 .. BRC_BINS_MAX_THR"; return BRC_E_ARG; }
    if (p->n_hist < 0 || p->n_hist > BRC_BINS_MAX_HIST) { *why = "n_hist: 0 .. BRC_BINS_MAX_HIST"; return BRC_E_ARG; }
    if (dst_stride < bins_of(p, n)) { *why = "dst_stride below n_bins"; return BRC_E_ARG; }
    return BRC_OK;
}
inline Job make_job(const brc_device_view* v, const brc_device_indels* d, const brc_bins_params* p, int64_t k0, int64_t n, int64_t dst_stride,
                    uint64_t* sums, uint64_t* covered, uint64_t* hist, uint32_t* status) {
    Job J;
    J.ncol = v->ncol; J.depth = v->depth; J.slotid = v->slotid; J.si = v->si; J.xagg = (const Rec*)v->xagg; J.n_xagg = v->n_xagg;
    J.slots = (const Slot*)d->slots; J.n_slots = d->n_slots;
    J.ref = d->ref; J.ref_lo = d->ref_lo; J.ref_hi = d->ref_hi; J.ref_len = d->ref_len;
    J.Lp = v->n_lib; J.pos0 = v->pos0; J.P = v->n_pos; J.PS = v->stride; J.k0 = k0; J.n = n;
    J.edges = p->edges; J.n_bins = bins_of(p, n); J.DS = dst_stride;
    J.width = (uint32_t)(p->width > n ? (n > 0 ? n : 1) : p->width);      // (a bin wider than the window is the window: n < 2^31)
    J.n_thr = p->n_thr; J.n_hist = p->n_hist;
    for (int t = 0; t < MAX_THR; ++t) J.thr[t] = t < p->n_thr ? p->thr[t] : 0u;
    J.o_sums = sums; J.o_cov = covered; J.o_hist = hist; J.o_status = status;
    return J;
}
// positions are swept only where some position can lie in a bin and something is wanted of it
inline bool sweeps(const Job& J) { return J.n > 0 && J.n_bins > 0 && (wants_sums(J) || wants_cov(J) || wants_hist(J)); }
// bytes the sweeps ask for / the destination bytes the call clears (brc_bins_last_timing)
inline void job_bytes(const Job& J, uint64_t* rd, uint64_t* wr) {
    const uint64_t n = (uint64_t)J.n, L = (uint64_t)J.Lp;
    *rd = J.edges ? 4u * ((uint64_t)J.n_bins + 1u) : 0u;
    if (sweeps(J)) {
        *rd += 4u * n * L * (wants_sums(J) ? 5u : 1u) + (wants_sums(J) ? n * L : 0u);
        if (walks_records(J)) *rd += 64u * J.n_xagg;
        if (walks_slots(J)) *rd += 72u * J.n_slots;
    }
    *wr = 8u * (clear_total(J) - 1u) + (J.o_status ? 4u : 0u);
}

}  // namespace brcbins
#endif
