// brc_select_core.h — per-lane functions of the device-side site selection (include/brc_select.h), written once for the gfx950 kernels
// (brc_select.hip) and for the CPU build the tests run (tests/sim_select).
//
//   link_lane    lane = third-allele record: a used record of a base bucket inside the window is pushed onto its position's list
//                (head[j] exchanged atomically, next[r] = the old head): a third allele's count sits only in such a record
//   flag_lane    lane = indel record: a live record inside the window judges itself against its library's role and depth and ORs one of
//                four bits — candidate / veto x insertion / deletion — into its position's flag word
//   why_lane     lane = position: ONE loop over the libraries — depth, slotid and the two slots' read counts, the position's records
//                on top (expand_lane's precedence, brc_dense_core.h) — keeps a 4-bit OR over the case libraries and a 4-bit AND over
//                the control libraries, and ends with the reason word, which takes the flag word's place in the scratch
//   [compaction] the non-zero reason words in order: wave ballot, block scan, reduce-then-scan across workgroups on the device
//                (brc_select.hip), a serial loop in the CPU build
// The atomics only link and flag: the list of a position holds the same records whatever their order, each (library, bucket) at most
// once, and an OR commutes — the result is a pure function of the inputs.
//
// Rec and Slot are brc_dense_core.h's and brc_indels_core.h's restatements of the engine's records; nothing of the engine is included.
#ifndef BRC_SELECT_CORE_H
#define BRC_SELECT_CORE_H

#include <stdint.h>

#include "../../include/brc_select.h"
#include "brc_indels_core.h"

namespace brcselect {

using brcdense::NI;
using brcdense::NONE32;
using brcdense::Rec;
using brcindels::Slot;

enum { BLOCK = 256, WAVE = 64 };                           // lanes of a workgroup of every kernel = positions of a scan tile
enum { F_CAND_INS = 1u, F_CAND_DEL = 2u, F_VETO_INS = 4u, F_VETO_DEL = 8u };
enum { ROLE_WORDS = 64 };                                  // 256 role bytes, four to a word: BRC_SELECT_MAX_LIB libraries fit

// One call's work.  It travels BY VALUE in the kernel arguments, the roles included: a library's role is a scalar load.
struct Job {
    const uint32_t *depth, *slotid, *si;                   // the view's planes, PS elements apart
    const Rec* xagg; uint64_t n_xagg;
    const Slot* slots; uint64_t n_slots;
    const char* ref; int64_t ref_lo, ref_hi, ref_len;
    int32_t Lp, pos0; int64_t PS;
    int64_t k0, n, cap;                                    // window [k0, k0 + n) of the planes
    uint32_t flags;
    uint32_t min_depth, min_alt, frac_num, frac_den, ctl_min_depth, ctl_max_alt, ctl_frac_num, ctl_frac_den;
    uint32_t role[ROLE_WORDS];
    // scratch (32-bit words): flag [n] the indel bits of a position, then its reason word; head [n] the first record of a position's
    // list (NONE32: none; present only when the view has records); next [n_xagg]; part [blocks + 1] the scan's workgroup sums; tot [1]
    uint32_t *flag, *head, *next, *part, *tot;
    int32_t* o_idx; uint32_t *o_why, *o_counts;
};

inline uint64_t blocks_of(uint64_t n) { return (n + BLOCK - 1) / BLOCK; }
inline uint64_t workspace_words(uint64_t n, uint64_t X) { return n + (X ? n + X : 0) + blocks_of(n) + 1 + 1; }
inline int64_t workspace_bytes(const brc_device_view* v, int64_t n) {
    if (!v || n <= 0) return 0;
    return (int64_t)(workspace_words((uint64_t)n, v->n_xagg) * 4u);
}
inline void carve(Job& J, void* ws) {
    uint32_t* w = (uint32_t*)ws; const uint64_t n = (uint64_t)J.n, X = J.n_xagg;
    J.flag = w; w += n;
    J.head = X ? w : nullptr; w += X ? n : 0;
    J.next = X ? w : nullptr; w += X;
    J.part = w; w += blocks_of(n) + 1; J.tot = w;
}

BRCD_HD uint32_t role_of(const Job& J, int l) { return (J.role[l >> 2] >> ((l & 3) * 8)) & 0xffu; }
BRCD_HD bool case_ok(const Job& J, uint32_t D, uint32_t c) {
    return D >= J.min_depth && c >= J.min_alt && (uint64_t)c * J.frac_den >= (uint64_t)J.frac_num * D;
}
// the last two terms of ctl_ok (the first, D >= ctl_min_depth, is a property of the library's position, not of a count)
BRCD_HD bool ctl_count_ok(const Job& J, uint32_t D, uint32_t c) {
    return c <= J.ctl_max_alt && (uint64_t)c * J.ctl_frac_den <= (uint64_t)J.ctl_frac_num * D;
}

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

// Lane = third-allele record r (head preset to NONE32): overlay_lane's bounds (brc_dense_core.h), and a base bucket only.
BRCD_HD void link_lane(const Job& J, uint64_t r) {
    const uint32_t k = J.xagg[r].k, lb = J.xagg[r].lib_b;
    if (k == NONE32) return;
    const int64_t l = lb >> 8, j = (int64_t)k - J.k0; const uint32_t b = lb & 0xffu;
    if (l >= J.Lp || b < 1u || b > 4u || j < 0 || j >= J.n) return;
    J.next[r] = exchange(J.head + j, (uint32_t)r);
}

// Lane = indel record s (flag preset to 0)
BRCD_HD void flag_lane(const Job& J, uint64_t s) {
    const Slot& o = J.slots[s];
    const int32_t len = o.len, lib = o.lib;
    if (len == 0 || lib < 0 || lib >= J.Lp) return;
    const int64_t j = (int64_t)o.pos - J.pos0 - J.k0;
    if (j < 0 || j >= J.n) return;
    const uint32_t role = role_of(J, lib);
    if (role == BRC_ROLE_IGNORE) return;
    const uint32_t D = J.depth[(int64_t)lib * J.PS + J.k0 + j], c = o.i[0];
    uint32_t bit = 0;
    if (role == BRC_ROLE_CASE) { if (case_ok(J, D, c)) bit = len > 0 ? F_CAND_INS : F_CAND_DEL; }
    else if (!ctl_count_ok(J, D, c)) bit = len > 0 ? F_VETO_INS : F_VETO_DEL;
    if (bit) fetch_or(J.flag + j, bit);
}

// indel records are looked at only when they are asked for and there are any (flag[] is preset only then)
BRCD_HD bool walks_slots(const Job& J) { return (J.flags & BRC_SELECT_INDEL) && J.n_slots; }

// reference character of plane index k -> its base bucket 1..4, 0: none of ACGTacgt (the rule of allele_char, brc_indels_core.h)
BRCD_HD uint32_t ref_bucket(const Job& J, int64_t k) {
    const int64_t p = (int64_t)J.pos0 + k;
    if (!J.ref || p < 0 || p >= J.ref_len || p < J.ref_lo || p >= J.ref_hi) return 0u;
    switch (J.ref[p - J.ref_lo] & 0xdf) {                   // (folds a..z onto A..Z; no other character lands on A C G T)
        case 'A': return 1u;
        case 'C': return 2u;
        case 'G': return 3u;
        case 'T': return 4u;
    }
    return 0u;
}

// Lane = window element j (after every link_lane and flag_lane of the call): the reason word, also left in flag[j].  Neighbouring
// lanes load neighbouring words of every plane; four loads per library, the position's records only where it has any.
BRCD_HD uint32_t why_lane(const Job& J, int64_t j) {
    const int64_t k = J.k0 + j;
    const uint32_t first = J.head ? J.head[j] : NONE32;
    uint32_t any_case = 0u, all_ctl = 0xfu; bool shallow = false;
    for (int l = 0; l < J.Lp; ++l) {
        const uint32_t role = role_of(J, l);               // (uniform over the wave)
        if (role == BRC_ROLE_IGNORE) continue;
        if (role == BRC_ROLE_CASE && !(J.flags & BRC_SELECT_SNV)) continue;      // (its indel records judged themselves: flag_lane)
        const int64_t row = (int64_t)l * J.PS + k;
        const uint32_t D = J.depth[row];
        if (role == BRC_ROLE_CONTROL && D < J.ctl_min_depth) shallow = true;
        if (!(J.flags & BRC_SELECT_SNV)) continue;
        const uint32_t sid = J.slotid[row], b0 = sid & 0xffu, b1 = (sid >> 8) & 0xffu;
        const uint32_t n0 = J.si[(((int64_t)l * 2 + 0) * NI) * J.PS + k], n1 = J.si[(((int64_t)l * 2 + 1) * NI) * J.PS + k];
        uint32_t c[4];
#pragma unroll
        for (uint32_t b = 0; b < 4u; ++b) {
            uint32_t v = 0u;
            if (b0 == b + 1u && n0) v = n0;
            if (b1 == b + 1u && n1) v = n1;
            c[b] = v;
        }
        for (uint32_t r = first; r != NONE32; r = J.next[r]) {
            const uint32_t lb = J.xagg[r].lib_b;
            if ((int)(lb >> 8) != l) continue;
            const uint32_t v = J.xagg[r].i[0];
#pragma unroll
            for (uint32_t b = 0; b < 4u; ++b) if ((lb & 0xffu) == b + 1u) c[b] = v;
        }
        uint32_t bits = 0u;
        if (role == BRC_ROLE_CASE) {
#pragma unroll
            for (uint32_t b = 0; b < 4u; ++b) if (case_ok(J, D, c[b])) bits |= 1u << b;
            any_case |= bits;
        } else {
#pragma unroll
            for (uint32_t b = 0; b < 4u; ++b) if (ctl_count_ok(J, D, c[b])) bits |= 1u << b;
            all_ctl &= bits;
        }
    }
    uint32_t why = 0u;
    if (J.flags & BRC_SELECT_SNV) {
        const uint32_t rb = ref_bucket(J, k);
        if (rb) why = any_case & all_ctl & ~(1u << (rb - 1u));
    }
    if (walks_slots(J)) {
        const uint32_t f = J.flag[j];
        why |= (f & ~(f >> 2) & 3u) << 4;
    }
    if (shallow) why = 0u;
    J.flag[j] = why;
    return why;
}

// Lane = window element j with its place `at` among the selected ones: the list's stores.
BRCD_HD void emit_lane(const Job& J, int64_t j, uint32_t why, uint64_t at) {
    if (!why || (int64_t)at >= J.cap) return;
    if (J.o_idx) J.o_idx[at] = (int32_t)(J.k0 + j);
    if (J.o_why) J.o_why[at] = why;
}

// The argument checks of brc_select_sites (everything but the kind of memory, which the two libraries check themselves): 0 = fine.
inline int check_job(const brc_device_view* v, const brc_device_indels* d, const brc_select_params* p, int64_t k0, int64_t n, int64_t cap, const void* ws,
                     const char** why) {
    if (!v || !d) { *why = "no view"; return BRC_E_ARG; }
    if (!p) { *why = "no parameters"; return BRC_E_ARG; }
    if (v->n_lib < 1 || v->n_pos < 0 || v->stride < v->n_pos || d->n_lib < 1 || d->n_pos < 0) { *why = "not a view of a computed region"; return BRC_E_ARG; }
    if (v->memory != d->memory || v->device != d->device || v->n_lib != d->n_lib || v->pos0 != d->pos0 || v->n_pos != d->n_pos) {
        *why = "the two views are not of one region"; return BRC_E_ARG;
    }
    if (v->n_lib > BRC_SELECT_MAX_LIB) { *why = "more libraries than BRC_SELECT_MAX_LIB"; return BRC_E_ARG; }
    if (k0 < 0 || n < 0 || k0 > v->n_pos || n > v->n_pos - k0) { *why = "the window must lie inside the view's planes"; return BRC_E_ARG; }
    if (n > 0 && (!v->ncol || !v->depth || !v->slotid || !v->si || !v->sf)) { *why = "a view without planes"; return BRC_E_ARG; }
    if (v->n_xagg && !v->xagg) { *why = "a view without its third-allele records"; return BRC_E_ARG; }
    if (d->n_slots && (!d->slots || !d->seq4 || !d->seq_off || !d->l_qseq || d->n_reads < 0)) { *why = "a view with records but without its arrays"; return BRC_E_ARG; }
    if (d->n_slots >= 0xfffffff0ull || v->n_xagg >= 0xfffffff0ull || (uint64_t)n >= 0x7ffffff0ull) { *why = "window too large: records and positions are indexed with 32 bits"; return BRC_E_ARG; }
    if (k0 + n > (int64_t)INT32_MAX) { *why = "the window ends behind plane index 2^31 - 1: idx has 32 bits"; return BRC_E_ARG; }
    if (p->flags == 0u || (p->flags & ~(BRC_SELECT_SNV | BRC_SELECT_INDEL))) { *why = "flags: BRC_SELECT_SNV | BRC_SELECT_INDEL"; return BRC_E_ARG; }
    if (p->min_alt == 0u || p->frac_den == 0u || p->ctl_frac_den == 0u) { *why = "min_alt, frac_den and ctl_frac_den must not be 0"; return BRC_E_ARG; }
    bool any_case = !p->role;
    for (int l = 0; p->role && l < v->n_lib; ++l) {
        if (p->role[l] > BRC_ROLE_CONTROL) { *why = "a role above 2"; return BRC_E_ARG; }
        any_case = any_case || p->role[l] == BRC_ROLE_CASE;
    }
    if (!any_case) { *why = "no case library"; return BRC_E_ARG; }
    if (cap < 0) { *why = "negative capacity"; return BRC_E_ARG; }
    if (n > 0 && !ws) { *why = "no workspace"; return BRC_E_ARG; }
    return BRC_OK;
}
inline Job make_job(const brc_device_view* v, const brc_device_indels* d, const brc_select_params* p, int64_t k0, int64_t n, int64_t cap, int32_t* idx,
                    uint32_t* why, uint32_t* counts, void* ws) {
    Job J;
    J.depth = v->depth; J.slotid = v->slotid; J.si = v->si; J.xagg = (const Rec*)v->xagg; J.n_xagg = v->n_xagg;
    J.slots = (const Slot*)d->slots; J.n_slots = d->n_slots;
    J.ref = d->ref; J.ref_lo = d->ref_lo; J.ref_hi = d->ref_hi; J.ref_len = d->ref_len;
    J.Lp = v->n_lib; J.pos0 = v->pos0; J.PS = v->stride; J.k0 = k0; J.n = n; J.cap = cap;
    J.flags = p->flags;
    J.min_depth = p->min_depth; J.min_alt = p->min_alt; J.frac_num = p->frac_num; J.frac_den = p->frac_den;
    J.ctl_min_depth = p->ctl_min_depth; J.ctl_max_alt = p->ctl_max_alt; J.ctl_frac_num = p->ctl_frac_num; J.ctl_frac_den = p->ctl_frac_den;
    for (int w = 0; w < ROLE_WORDS; ++w) J.role[w] = 0u;
    for (int l = 0; l < v->n_lib; ++l) J.role[l >> 2] |= (uint32_t)(p->role ? p->role[l] : BRC_ROLE_CASE) << ((l & 3) * 8);
    carve(J, ws);
    if (!(J.flags & BRC_SELECT_SNV)) J.head = nullptr;      // (base counts are not looked at: neither are their records)
    J.o_idx = idx; J.o_why = why; J.o_counts = counts;
    return J;
}
inline bool wants_list(const Job& J) { return (J.o_idx || J.o_why) && J.cap > 0; }
inline bool walks_records(const Job& J) { return J.head != nullptr; }
// bytes the sweeps ask for / the scratch bytes the call writes (brc_select_last_timing)
inline void job_bytes(const Job& J, uint64_t* rd, uint64_t* wr) {
    const uint64_t n = (uint64_t)J.n;
    uint64_t L = 0;
    for (int l = 0; l < J.Lp; ++l) L += role_of(J, l) != BRC_ROLE_IGNORE;
    const uint64_t snv = (J.flags & BRC_SELECT_SNV) ? 1u : 0u, chain = walks_records(J) ? 1u : 0u, ind = walks_slots(J) ? 1u : 0u;
    *rd = 4u * n * (L * (1u + 3u * snv) + chain + ind + (wants_list(J) ? 1u : 0u)) + n * snv + 64u * J.n_xagg * chain + 72u * J.n_slots * ind;
    *wr = 4u * (n * (1u + chain + ind) + J.n_xagg * chain + blocks_of(n) + 2u);
}

}  // namespace brcselect
#endif
