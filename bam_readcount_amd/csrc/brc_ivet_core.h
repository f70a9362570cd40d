// brc_ivet_core.h — per-lane functions of the device-side indel candidate filter (include/brc_ivet.h), written once for the gfx950
// kernels (brc_ivet.hip) and for the CPU build the tests run (tests/sim_ivet).
//
//   link_lane     lane = third-allele record: brc_vet_core.h's link with the table's pos as the searched list — a used record of a base
//                 bucket inside the planes looks for the FIRST table record of its position and pushes itself onto that record's list
//   list_lane     lane = list element j: its range and its order against the element before -> status bits
//   record_lane   lane = table record r: ONE load of pos, lib, len and the reference character; the record's 13 sums; the plane loads of
//                 brc_vet_core.h's sites_lane at (lib, pos - pos0) and the position's third-allele records on top -> the reference
//                 bucket; brc_vet_core.h's judge; the control libraries' depths; the walk over the record's run, left and right, with
//                 the allele text compared bytewise; the stores at r; a binary search over idx for the list elements of its position
//                 and an OR into keep
// The tests, the buckets, the reference character and the binary search are brc_vet_core.h's functions, not copies: this header adds
// the table, the roles and the run walk.  The atomics only link and OR bits: the result is a pure function of the inputs.
#ifndef BRC_IVET_CORE_H
#define BRC_IVET_CORE_H

#include <stdint.h>

#include "../../include/brc_ivet.h"
#include "brc_vet_core.h"

namespace brcivet {

using brcdense::I_N;
using brcdense::NF;
using brcdense::NI;
using brcdense::NONE32;
using brcdense::put;
using brcdense::Rec;
using brcvet::BLOCK;
using brcvet::blocks_of;
using brcvet::lower_bound;
using brcvet::NVAL;
using brcvet::Side;

enum { ROLE_WORDS = 16 };                                  // 256 roles of two bits: BRC_IVET_MAX_LIB libraries fit
static const uint32_t VET_TESTS = BRC_VET_ALL_TESTS & ~BRC_VET_VAR_BQ;

// One call's work, BY VALUE in the kernel arguments.  V is the SNV filter's job: the view's planes, the reference slice, the thresholds
// and the scratch (head [m], next [n_xagg]) as brc_vet_core.h's functions read them; its list and destinations are not used.
struct Job {
    brcvet::Job V;
    int64_t m, TS, A;                                      // records; istat / fstat planes TS elements apart; alleles_len
    const int32_t *pos, *lib, *len; const uint32_t* istat; const float* fstat; const uint32_t* off; const uint8_t* text;
    const int32_t* idx; const uint32_t* why; int64_t n, DS;
    uint32_t tests, kinds, ctl_min_depth, ctl_max_count, ctl_frac_num, ctl_frac_den;
    uint32_t any_ctl;                                      // some library is a control library
    uint32_t role[ROLE_WORDS];
    uint32_t *o_fail, *o_ctl, *o_keep; float* o_vals; uint32_t* status;
};

inline int64_t workspace_bytes(const brc_device_view* v, int64_t m) { return brcvet::workspace_bytes(v, m); }

BRCD_HD uint32_t role_of(const Job& J, int64_t l) { return (J.role[l >> 4] >> ((l & 15) * 2)) & 3u; }

// Lane = third-allele record r (head preset to NONE32): link_lane of brc_vet_core.h, the searched list being the table's positions.
BRCD_HD void link_lane(const Job& J, uint64_t r) {
    const uint32_t k = J.V.xagg[r].k, lb = J.V.xagg[r].lib_b;
    if (k == NONE32) return;
    const int64_t l = lb >> 8; const uint32_t b = lb & 0xffu;
    if (l >= J.V.Lp || b < 1u || b > 4u || (int64_t)k >= J.V.P) return;
    const int64_t p = (int64_t)J.V.pos0 + (int64_t)k;
    const int64_t j = lower_bound(J.pos, J.m, p);
    if (j >= J.m || (int64_t)J.pos[j] != p) return;
    J.V.next[r] = brcvet::exchange(J.V.head + j, (uint32_t)r);
}

// Lane = list element j: the list is judged once per element.
BRCD_HD void list_lane(const Job& J, int64_t j) {
    if (!J.status) return;
    const int64_t k = J.idx[j];
    uint32_t bits = (k >= 0 && k < J.V.P) ? 0u : BRC_IVET_LIST_OUT_OF_RANGE;
    if (j > 0 && (int64_t)J.idx[j - 1] > k) bits |= BRC_IVET_LIST_NOT_ASCENDING;
    if (bits) brcvet::status_or(J.status, bits);
}

// text(x) of include/brc_ivet.h: [*a, *a + return) inside alleles whatever allele_off holds
BRCD_HD int64_t text_of(const Job& J, int64_t x, int64_t* a) {
    int64_t a0 = J.off[x], a1 = J.off[x + 1];
    if (a0 > J.A) a0 = J.A;
    if (a1 > J.A) a1 = J.A;
    *a = a0;
    return a1 > a0 ? a1 - a0 : 0;
}

// Record x of r's run against r (length ln, text [a, a + na)): a control library's record of the same allele -> its count folds into
// *most, and its failing the control test into the return value.
BRCD_HD bool control_vetoes(const Job& J, int64_t x, int64_t k, int32_t ln, int64_t a, int64_t na, uint32_t* most) {
    const int64_t c = J.lib[x];
    if (c < 0 || c >= J.V.Lp || role_of(J, c) != (uint32_t)BRC_ROLE_CONTROL || J.len[x] != ln) return false;
    int64_t b;
    if (text_of(J, x, &b) != na) return false;
    for (int64_t i = 0; i < na; ++i) if (J.text[a + i] != J.text[b + i]) return false;
    const uint32_t C = J.istat[(int64_t)I_N * J.TS + x];
    if (C > *most) *most = C;
    const uint64_t D = J.V.depth[c * J.V.PS + k];
    return !(C <= J.ctl_max_count && (uint64_t)C * J.ctl_frac_den <= (uint64_t)J.ctl_frac_num * D);
}

// Lane = table record r (after every link_lane of the call; keep cleared).  Neighbouring lanes load neighbouring words of every table
// array and store neighbouring words of every destination: a wave's stores are runs of 256 contiguous bytes whatever the table holds.
BRCD_HD void record_lane(const Job& J, int64_t r) {
    const int64_t p = J.pos[r], l = J.lib[r]; const int32_t ln = J.len[r];
    const int64_t k = p - (int64_t)J.V.pos0;
    const bool in = k >= 0 && k < J.V.P && l >= 0 && l < J.V.Lp;
    const bool twin = r > 0 && (int64_t)J.pos[r - 1] == p;
    if (J.status) {
        uint32_t bits = (ln != 0 && !in) ? BRC_IVET_TABLE_OUT_OF_RANGE : 0u;
        if (r > 0 && (int64_t)J.pos[r - 1] > p) bits |= BRC_IVET_TABLE_NOT_ASCENDING;
        if (bits) brcvet::status_or(J.status, bits);
    }
    if (!J.o_fail && !J.o_vals && !J.o_ctl && !J.o_keep) return;
    const uint32_t kind = ln > 0 ? BRC_WHY_INS : BRC_WHY_DEL;
    uint32_t f, rb = 0u;
    if (ln == 0) f = BRC_IVET_NOT_ASKED;
    else if (!in) f = BRC_IVET_NO_SITE;
    else if (role_of(J, l) != (uint32_t)BRC_ROLE_CASE || !(J.kinds & kind)) f = BRC_IVET_NOT_ASKED;
    else if (!(rb = brcvet::ref_bucket(J.V, k))) f = BRC_IVET_NO_SITE;
    else f = 0u;
    float val[NVAL];
#pragma unroll
    for (int c = 0; c < NVAL; ++c) val[c] = 0.0f;
    uint32_t most = 0u;
    if (!f) {
        // the variant side: the record's own sums
        uint32_t vi[NI]; float vf[NF];
#pragma unroll
        for (int c = 0; c < NI; ++c) vi[c] = J.istat[(int64_t)c * J.TS + r];
#pragma unroll
        for (int c = 0; c < NF; ++c) vf[c] = J.fstat[(int64_t)c * J.TS + r];
        Side Vs = brcvet::side_of(vi, vf);
        Vs.m[brcvet::C_BQ] = 0.0f;                         // (no base-quality sum in an indel bucket)
        // the reference side: sites_lane's loads at (l, k)
        const int64_t row = l * J.V.PS + k;
        const uint32_t D = J.V.depth[row], sid = J.V.slotid[row], b0 = sid & 0xffu, b1 = (sid >> 8) & 0xffu;
        uint32_t si[2][NI]; float sf[2][NF];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
#pragma unroll
            for (int c = 0; c < NI; ++c) si[s][c] = J.V.si[((l * 2 + s) * NI + c) * J.V.PS + k];
#pragma unroll
            for (int c = 0; c < NF; ++c) sf[s][c] = J.V.sf[((l * 2 + s) * NF + c) * J.V.PS + k];
        }
        uint32_t first = NONE32;
        if (J.V.head) {                                    // (on an unsorted table the search may end at another position's run: its list is not this record's)
            const int64_t h = twin ? lower_bound(J.pos, r, p) : r;
            if ((int64_t)J.pos[h] == p) first = J.V.head[h];
        }
        const Side R = brcvet::bucket_side(J.V, (int)l, rb, b0, b1, si, sf, first);
        f = brcvet::judge(J.V, D, Vs, R, val);             // (J.V.tests: the seventeen tests that are asked)
        if (J.tests & BRC_IVET_CTL_DEPTH) {
            for (int c = 0; c < J.V.Lp; ++c)               // (uniform over the wave: the roles are kernel arguments)
                if (role_of(J, c) == (uint32_t)BRC_ROLE_CONTROL && J.V.depth[(int64_t)c * J.V.PS + k] < J.ctl_min_depth) f |= BRC_IVET_CTL_DEPTH;
        }
        if (J.any_ctl && J.off && J.text) {                 // (without a control library the walk can find nothing)
            int64_t a; const int64_t na = text_of(J, r, &a);
            bool veto = false;
            for (int64_t x = r - 1; x >= 0 && (int64_t)J.pos[x] == p; --x) veto |= control_vetoes(J, x, k, ln, a, na, &most);
            for (int64_t x = r + 1; x < J.m && (int64_t)J.pos[x] == p; ++x) veto |= control_vetoes(J, x, k, ln, a, na, &most);
            if (veto && (J.tests & BRC_IVET_CTL_ALLELE)) f |= BRC_IVET_CTL_ALLELE;
        }
        if (J.o_keep && !f) {
            for (int64_t j = lower_bound(J.idx, J.n, k); j < J.n && (int64_t)J.idx[j] == k; ++j)
                if (!J.why || (J.why[j] & kind)) brcvet::status_or(J.o_keep + j, kind);
        }
    }
    if (J.o_fail) put(J.o_fail + r, f);
    if (J.o_ctl) put(J.o_ctl + r, most);
    if (J.o_vals) {
#pragma unroll
        for (int c = 0; c < NVAL; ++c) put(J.o_vals + (int64_t)c * J.DS + r, val[c]);
    }
}

// The argument checks of brc_ivet_records (everything but the kind of memory, which the two libraries check themselves): 0 = fine.
// What the SNV filter refuses about the views, the list and the thresholds it shares is refused by ITS check.
inline brc_vet_params vet_params_of(const brc_ivet_params* p) {
    brc_vet_params q;
    q.lib_on = nullptr; q.tests = p->tests & VET_TESTS;
    q.min_depth = p->min_depth; q.min_var_count = p->min_var_count; q.freq_num = p->freq_num; q.freq_den = p->freq_den;
    q.min_strand_reads = p->min_strand_reads; q.strand_num = p->strand_num; q.strand_den = p->strand_den; q.min_ref_reads = p->min_ref_reads;
    q.min_var_readpos = p->min_var_readpos; q.min_var_dist3 = p->min_var_dist3; q.min_var_bq = 0.0f; q.min_var_mapq = p->min_var_mapq;
    q.max_var_mmqs = p->max_var_mmqs; q.min_var_rl = p->min_var_rl;
    q.min_ref_readpos = p->min_ref_readpos; q.min_ref_dist3 = p->min_ref_dist3; q.min_ref_bq = p->min_ref_bq; q.min_ref_mapq = p->min_ref_mapq;
    q.min_ref_rl = p->min_ref_rl; q.max_mmqs_diff = p->max_mmqs_diff; q.max_mapq_diff = p->max_mapq_diff; q.max_rl_diff = p->max_rl_diff;
    return q;
}
inline int check_job(const brc_device_view* v, const brc_device_indels* d, const brc_ivet_params* p, const brc_ivet_table* t, const int32_t* idx, int64_t n,
                     int64_t dst_stride, const void* ws, const char** why) {
    if (!p) { *why = "no parameters"; return BRC_E_ARG; }
    if (!t) { *why = "no table"; return BRC_E_ARG; }
    if (p->tests & ~BRC_IVET_ALL_TESTS) { *why = "tests: a mask of BRC_IVET_ALL_TESTS (VAR_BQ is not a test of indel records)"; return BRC_E_ARG; }
    const brc_vet_params q = vet_params_of(p);
    static const char some = 0;
    if (int rc = brcvet::check_job(v, d, &q, idx, n, n, &some, why)) return rc;
    if (t->m < 0 || t->stride < t->m) { *why = "a table with m below 0 or stride below m"; return BRC_E_ARG; }
    if ((uint64_t)t->m >= 0x7ffffff0ull) { *why = "table too large: records are indexed with 32 bits"; return BRC_E_ARG; }
    if (t->alleles_len < 0) { *why = "alleles_len below 0"; return BRC_E_ARG; }
    if (t->m > 0 && (!t->pos || !t->lib || !t->len || !t->istat || !t->fstat)) { *why = "a table without its arrays"; return BRC_E_ARG; }
    if (t->m > 0 && (p->tests & BRC_IVET_CTL_ALLELE) && (!t->allele_off || !t->alleles)) { *why = "CTL_ALLELE needs allele_off and alleles"; return BRC_E_ARG; }
    if (dst_stride < t->m) { *why = "dst_stride below m"; return BRC_E_ARG; }
    if (t->m > 0 && (!v->ncol || !v->depth || !v->slotid || !v->si || !v->sf)) { *why = "a view without planes"; return BRC_E_ARG; }
    if (!p->kinds || (p->kinds & ~(BRC_WHY_INS | BRC_WHY_DEL))) { *why = "kinds: a mask of BRC_WHY_INS | BRC_WHY_DEL, not 0"; return BRC_E_ARG; }
    if (p->ctl_frac_den == 0u) { *why = "ctl_frac_den must not be 0"; return BRC_E_ARG; }
    bool any = !p->role;
    for (int l = 0; p->role && l < v->n_lib; ++l) {
        if (p->role[l] > BRC_ROLE_CONTROL) { *why = "a role above 2"; return BRC_E_ARG; }
        any = any || p->role[l] == BRC_ROLE_CASE;
    }
    if (!any) { *why = "no case library"; return BRC_E_ARG; }
    if (t->m > 0 && !ws) { *why = "no workspace"; return BRC_E_ARG; }
    return BRC_OK;
}
inline Job make_job(const brc_device_view* v, const brc_device_indels* d, const brc_ivet_params* p, const brc_ivet_table* t, const int32_t* idx,
                    const uint32_t* why, int64_t n, int64_t dst_stride, uint32_t* fail, float* vals, uint32_t* ctl_count, uint32_t* keep, uint32_t* status,
                    void* ws) {
    Job J;
    const brc_vet_params q = vet_params_of(p);
    J.V = brcvet::make_job(v, d, &q, nullptr, nullptr, t->m, dst_stride, nullptr, nullptr, nullptr, status, ws);
    const bool chain = v->n_xagg != 0 && t->m > 0 && (fail || vals || ctl_count || keep);
    J.V.head = chain ? (uint32_t*)ws : nullptr;
    J.V.next = chain ? (uint32_t*)ws + t->m : nullptr;
    J.m = t->m; J.TS = t->stride; J.A = t->alleles_len;
    J.pos = t->pos; J.lib = t->lib; J.len = t->len; J.istat = t->istat; J.fstat = t->fstat; J.off = t->allele_off; J.text = t->alleles;
    J.idx = idx; J.why = why; J.n = n; J.DS = dst_stride;
    J.tests = p->tests; J.kinds = p->kinds;
    J.ctl_min_depth = p->ctl_min_depth; J.ctl_max_count = p->ctl_max_count; J.ctl_frac_num = p->ctl_frac_num; J.ctl_frac_den = p->ctl_frac_den;
    for (int w = 0; w < ROLE_WORDS; ++w) J.role[w] = 0u;
    J.any_ctl = 0u;
    for (int l = 0; l < v->n_lib; ++l) {
        const uint32_t ro = p->role ? p->role[l] : (uint32_t)BRC_ROLE_CASE;
        J.role[l >> 4] |= ro << ((l & 15) * 2);
        if (ro == (uint32_t)BRC_ROLE_CONTROL) J.any_ctl = 1u;
    }
    J.o_fail = fail; J.o_vals = vals; J.o_ctl = ctl_count; J.o_keep = keep; J.status = status;
    return J;
}
inline bool wants_dests(const Job& J) { return J.o_fail || J.o_vals || J.o_ctl || J.o_keep; }
inline bool walks_records(const Job& J) { return J.V.head != nullptr; }
inline uint64_t lanes_of(const Job& J) { return (uint64_t)(J.m > J.n ? J.m : J.n); }
// bytes the kernels ask for / write (brc_ivet_last_timing)
inline void job_bytes(const Job& J, uint64_t* rd, uint64_t* wr) {
    const uint64_t m = (uint64_t)J.m, n = (uint64_t)J.n, chain = walks_records(J) ? 1u : 0u, dests = wants_dests(J) ? 1u : 0u;
    uint64_t ctl = 0;
    for (int l = 0; l < J.V.Lp; ++l) ctl += role_of(J, l) == (uint32_t)BRC_ROLE_CONTROL;
    if (!(J.tests & BRC_IVET_CTL_DEPTH)) ctl = 0;
    *rd = 4u * m * (4u + dests * ((NI + NF) + (J.off ? 2u : 0u) + 2u + 2u * (NI + NF) + ctl + chain)) + m * dests + 4u * n * ((J.status ? 2u : 0u) + (J.why && J.o_keep ? 1u : 0u)) +
          64u * J.V.n_xagg * chain;
    *wr = 4u * m * ((J.o_fail ? 1u : 0u) + (J.o_ctl ? 1u : 0u) + (J.o_vals ? (uint64_t)NVAL : 0u) + chain) + 4u * n * (J.o_keep ? 1u : 0u) + 4u * J.V.n_xagg * chain;
}

}  // namespace brcivet
#endif
