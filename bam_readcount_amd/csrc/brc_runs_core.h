// brc_runs_core.h — per-lane functions of the device-side depth-class intervals (include/brc_runs.h), written once for the gfx950 kernels
// (brc_runs.hip) and for the CPU build the tests run (tests/sim_runs).
//
//   class_lane   lane = window element: ONE loop over the counted libraries — one depth word each, neighbouring lanes neighbouring
//                words — keeps a 64-bit V (minimum, maximum or sum), counts the cuts at or below it and applies the reference rule
//                (brcselect::ref_bucket: the selector's)
//   starts_run / ends_run   the boundary rule: position k STARTS an emitted run iff its class is kept and (k == k0 or class(k - 1) differs),
//                it ENDS one iff its class is kept and (k == k0 + n - 1 or class(k + 1) differs).  Emitted starts and emitted ends are
//                equal in number and in the same order, so the j-th start and the j-th end belong to one run: no lane looks ahead for
//                its end, two ranks per position suffice
//   emit_lane    lane = window element with its two ranks: start / cls at the start rank, end at the end rank, below cap
//   [ranks]      wave ballots, the waves' counts, reduce-then-scan across workgroups on the device (brc_runs.hip), serial loops in the
//                CPU build
// The only atomics add integers (per_class): the result is a pure function of the inputs.
//
// Nothing of the engine is included.
#ifndef BRC_RUNS_CORE_H
#define BRC_RUNS_CORE_H

#include <stdint.h>

#include "../../include/brc_runs.h"
#include "brc_select_core.h"

namespace brcruns {

enum { BLOCK = 256, WAVE = 64 };                           // lanes of a workgroup of every kernel = positions of a scan tile
enum { MAX_CUT = BRC_RUNS_MAX_CUT, ROLE_WORDS = 64 };      // 256 role bytes, four to a word: BRC_RUNS_MAX_LIB libraries fit
static const uint32_t NO_CLASS = 0xffffffffu;              // the class of the positions outside the window: differs from every class

// One call's work.  It travels BY VALUE in the kernel arguments, the cuts and the roles included: both are scalar loads.
struct Job {
    const uint32_t* depth;                                 // the view's depth plane, PS elements per library
    const char* ref; int64_t ref_lo, ref_hi, ref_len;
    int32_t Lp, pos0; int64_t PS;
    int64_t k0, n, cap;                                    // window [k0, k0 + n) of the planes
    uint32_t combine, n_cut, keep, flags;
    uint32_t cut[MAX_CUT];
    uint32_t role[ROLE_WORDS];
    // scratch (32-bit words): w_cls [n] the class of every window element; part_s, part_e [blocks] per workgroup its emitted starts and
    // its emitted ends, then their exclusive scans
    uint32_t *w_cls, *part_s, *part_e;
    int32_t *o_start, *o_end; uint32_t *o_cls, *o_counts; uint64_t* o_per;
};

inline uint64_t blocks_of(uint64_t n) { return (n + BLOCK - 1) / BLOCK; }
inline int64_t workspace_bytes(int64_t n) { return n <= 0 ? 0 : (int64_t)(4u * (uint64_t)n + 8u * blocks_of((uint64_t)n)); }

BRCD_HD uint32_t role_of(const Job& J, int l) { return (J.role[l >> 2] >> ((l & 3) * 8)) & 0xffu; }
BRCD_HD uint32_t n_class(const Job& J) { return J.n_cut + 2u; }
BRCD_HD bool kept(const Job& J, uint32_t c) { return c != NO_CLASS && ((J.keep >> c) & 1u); }

BRCD_HD void add64(uint64_t* p, uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd((unsigned long long*)p, (unsigned long long)v);
#else
    *p += v;
#endif
}

// The selector's reference rule itself (brcselect::ref_bucket), given the five fields it reads: 0 = none of ACGTacgt.
BRCD_HD uint32_t ref_bucket(const Job& J, int64_t k) {
    brcselect::Job S;
    S.ref = J.ref; S.ref_lo = J.ref_lo; S.ref_hi = J.ref_hi; S.ref_len = J.ref_len; S.pos0 = J.pos0;
    return brcselect::ref_bucket(S, k);
}

// Lane = window element j: its class.
BRCD_HD uint32_t class_lane(const Job& J, int64_t j) {
    const int64_t k = J.k0 + j;
    if ((J.flags & BRC_RUNS_REF_N) && !ref_bucket(J, k)) return J.n_cut + 1u;
    uint64_t V = J.combine == BRC_RUNS_MIN ? ~0ull : 0ull;
    for (int l = 0; l < J.Lp; ++l) {
        if (!role_of(J, l)) continue;                      // (uniform over the wave)
        const uint64_t d = J.depth[(int64_t)l * J.PS + k];
        if (J.combine == BRC_RUNS_MIN) V = d < V ? d : V;
        else if (J.combine == BRC_RUNS_MAX) V = d > V ? d : V;
        else V += d;
    }
    uint32_t c = 0u;
    for (uint32_t i = 0; i < J.n_cut; ++i) c += (uint64_t)J.cut[i] <= V;
    return c;
}

// The boundary rule, on the class of a position and of its neighbour (NO_CLASS: the neighbour lies outside the window).
BRCD_HD bool starts_run(const Job& J, uint32_t left, uint32_t c) { return kept(J, c) && left != c; }
BRCD_HD bool ends_run(const Job& J, uint32_t c, uint32_t right) { return kept(J, c) && right != c; }

// Lane = window element j of class c with its places among the emitted starts and the emitted ends: the list's stores.
BRCD_HD void emit_lane(const Job& J, int64_t j, uint32_t c, bool is_start, uint64_t at_start, bool is_end, uint64_t at_end) {
    if (is_start && (int64_t)at_start < J.cap) {
        if (J.o_start) J.o_start[at_start] = (int32_t)(J.k0 + j);
        if (J.o_cls) J.o_cls[at_start] = c;
    }
    if (is_end && (int64_t)at_end < J.cap && J.o_end) J.o_end[at_end] = (int32_t)(J.k0 + j + 1);
}

// a workgroup's two counts in one word for the scan (each stays below 2^31: no carry crosses), and back
BRCD_HD uint64_t pack(uint32_t starts, uint32_t ends) { return (uint64_t)starts | ((uint64_t)ends << 32); }
BRCD_HD uint32_t starts_of(uint64_t p) { return (uint32_t)p; }
BRCD_HD uint32_t ends_of(uint64_t p) { return (uint32_t)(p >> 32); }

// The argument checks of brc_runs_find (everything but the kind of memory, which the two libraries check themselves): 0 = fine.
inline int check_job(const brc_device_view* v, const brc_device_indels* d, const brc_runs_params* p, int64_t k0, int64_t n, int64_t cap, const void* ws,
                     const char** why) {
    if (!v) { *why = "no view"; return BRC_E_ARG; }
    if (!p) { *why = "no parameters"; return BRC_E_ARG; }
    if (v->n_lib < 1 || v->n_pos < 0 || v->stride < v->n_pos) { *why = "not a view of a computed region"; return BRC_E_ARG; }
    if (d) {
        if (d->n_lib < 1 || d->n_pos < 0) { *why = "not a view of a computed region"; return BRC_E_ARG; }
        if (v->memory != d->memory || v->device != d->device || v->n_lib != d->n_lib || v->pos0 != d->pos0 || v->n_pos != d->n_pos) {
            *why = "the two views are not of one region"; return BRC_E_ARG;
        }
        if (d->n_slots && (!d->slots || !d->seq4 || !d->seq_off || !d->l_qseq || d->n_reads < 0)) { *why = "a view with records but without its arrays"; return BRC_E_ARG; }
    }
    if (v->n_lib > BRC_RUNS_MAX_LIB) { *why = "more libraries than BRC_RUNS_MAX_LIB"; return BRC_E_ARG; }
    if (k0 < 0 || n < 0 || k0 > v->n_pos || n > v->n_pos - k0) { *why = "the window must lie inside the view's planes"; return BRC_E_ARG; }
    if (n > 0 && (!v->ncol || !v->depth || !v->slotid || !v->si || !v->sf)) { *why = "a view without planes"; return BRC_E_ARG; }
    if (v->n_xagg && !v->xagg) { *why = "a view without its third-allele records"; return BRC_E_ARG; }
    if (k0 + n > (int64_t)INT32_MAX) { *why = "the window ends behind plane index 2^31 - 1: start and end have 32 bits"; return BRC_E_ARG; }
    if (p->combine > BRC_RUNS_SUM) { *why = "combine: BRC_RUNS_MIN | BRC_RUNS_MAX | BRC_RUNS_SUM"; return BRC_E_ARG; }
    if (p->flags & ~BRC_RUNS_REF_N) { *why = "flags: 0 | BRC_RUNS_REF_N"; return BRC_E_ARG; }
    if (p->n_cut < 1u || p->n_cut > BRC_RUNS_MAX_CUT) { *why = "n_cut: 1 .. BRC_RUNS_MAX_CUT"; return BRC_E_ARG; }
    for (uint32_t i = 1; i < p->n_cut; ++i)
        if (p->cut[i] <= p->cut[i - 1]) { *why = "the cuts must ascend strictly"; return BRC_E_ARG; }
    if (p->keep == 0u || (p->keep >> (p->n_cut + 2u))) { *why = "keep: at least one class, none above n_cut + 1"; return BRC_E_ARG; }
    if ((p->flags & BRC_RUNS_REF_N) && !d) { *why = "BRC_RUNS_REF_N needs the indels view: it carries the reference"; return BRC_E_ARG; }
    bool any = !p->role;
    for (int l = 0; p->role && l < v->n_lib; ++l) {
        if (p->role[l] > 1) { *why = "a role above 1"; return BRC_E_ARG; }
        any = any || p->role[l] == 1;
    }
    if (!any) { *why = "no counted library"; return BRC_E_ARG; }
    if (cap < 0) { *why = "negative capacity"; return BRC_E_ARG; }
    if (n > 0 && !ws) { *why = "no workspace"; return BRC_E_ARG; }
    return BRC_OK;
}
inline Job make_job(const brc_device_view* v, const brc_device_indels* d, const brc_runs_params* p, int64_t k0, int64_t n, int64_t cap, int32_t* start,
                    int32_t* end, uint32_t* cls, uint32_t* counts, uint64_t* per_class, void* ws) {
    Job J;
    J.depth = v->depth;
    const bool ref = (p->flags & BRC_RUNS_REF_N) && d;
    J.ref = ref ? d->ref : nullptr; J.ref_lo = ref ? d->ref_lo : 0; J.ref_hi = ref ? d->ref_hi : 0; J.ref_len = ref ? d->ref_len : 0;
    J.Lp = v->n_lib; J.pos0 = v->pos0; J.PS = v->stride; J.k0 = k0; J.n = n; J.cap = cap;
    J.combine = p->combine; J.n_cut = p->n_cut; J.keep = p->keep; J.flags = p->flags;
    for (uint32_t i = 0; i < (uint32_t)MAX_CUT; ++i) J.cut[i] = i < p->n_cut ? p->cut[i] : 0xffffffffu;
    for (int w = 0; w < ROLE_WORDS; ++w) J.role[w] = 0u;
    for (int l = 0; l < v->n_lib; ++l) J.role[l >> 2] |= (uint32_t)(p->role ? p->role[l] : 1u) << ((l & 3) * 8);
    J.w_cls = (uint32_t*)ws; J.part_s = J.w_cls + (n > 0 ? n : 0); J.part_e = J.part_s + blocks_of((uint64_t)(n > 0 ? n : 0));
    J.o_start = start; J.o_end = end; J.o_cls = cls; J.o_counts = counts; J.o_per = per_class;
    return J;
}
inline bool wants_list(const Job& J) { return (J.o_start || J.o_end || J.o_cls) && J.cap > 0; }
inline bool wants_ranks(const Job& J) { return J.o_counts || wants_list(J); }
// bytes the sweeps ask for / the scratch bytes the call writes (brc_runs_last_timing)
inline void job_bytes(const Job& J, uint64_t* rd, uint64_t* wr) {
    const uint64_t n = (uint64_t)J.n, nb = blocks_of(n);
    uint64_t L = 0;
    for (int l = 0; l < J.Lp; ++l) L += role_of(J, l) != 0u;
    *rd = 4u * n * L + ((J.flags & BRC_RUNS_REF_N) ? n : 0u) + (wants_ranks(J) ? 8u * nb : 0u) + (wants_list(J) ? 4u * n + 8u * nb : 0u);
    *wr = 4u * n + (wants_ranks(J) ? 16u * nb : 0u);
}

}  // namespace brcruns
#endif
