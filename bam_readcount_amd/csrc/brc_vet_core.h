// brc_vet_core.h — per-lane functions of the device-side candidate filter (include/brc_vet.h), written once for the gfx950 kernels
// (brc_vet.hip) and for the CPU build the tests run (tests/sim_vet).
//
//   link_lane    lane = third-allele record: a used record of a base bucket inside the planes looks for the FIRST element that lists its
//                position (overlay_lane's binary search over idx, brc_panel_core.h) and pushes itself onto that element's list
//                (head[j] exchanged atomically, next[r] = the old head): a third allele's sums sit only in such a record
//   sites_lane   lane = list element j: ONE load of idx[j], alt[j] and the reference character, then a loop over the libraries —
//                gather_lane's loads at that index (depth, slotid, the two slots: 28 words), the position's records on top
//                (expand_lane's precedence, brc_dense_core.h), the four base buckets' counts and six tested columns, the tests of
//                every asked base against the reference's bucket — and the stores at j; keep is the lane's OR over the libraries
// The atomics only link (and OR status bits): the list of a position holds the same records whatever their order, each (library,
// bucket) at most once — the result is a pure function of the inputs.
//
// Rec, metrics13 and put are brc_dense_core.h's; layouts are restated by their strides, nothing of the engine is included.
#ifndef BRC_VET_CORE_H
#define BRC_VET_CORE_H

#include <stdint.h>

#include "../../include/brc_vet.h"
#include "brc_dense_core.h"

namespace brcvet {

using brcdense::I_MINUS;
using brcdense::I_N;
using brcdense::I_PLUS;
using brcdense::metrics13;
using brcdense::NF;
using brcdense::NI;
using brcdense::NM;
using brcdense::NONE32;
using brcdense::put;
using brcdense::Rec;

enum { BLOCK = 256 };                                      // lanes of a workgroup of both kernels
enum { NVAL = BRC_VET_NVAL, NCOL = 6 };                    // columns of vals; the tested columns of a side
enum { ON_WORDS = 8 };                                     // 256 lib_on bits: BRC_VET_MAX_LIB libraries fit

// One call's work.  It travels BY VALUE in the kernel arguments, lib_on included: whether a library is judged is a scalar load.
struct Job {
    const uint32_t *depth, *slotid, *si; const float* sf;  // the view's planes, PS elements apart
    const Rec* xagg; uint64_t n_xagg;
    const char* ref; int64_t ref_lo, ref_hi, ref_len;
    int32_t Lp, pos0; int64_t P, PS;
    const int32_t* idx; const uint32_t* alt; int64_t n, DS;     // element j is plane index idx[j]; destination planes DS elements apart
    uint32_t tests;
    uint32_t min_depth, min_var_count, freq_num, freq_den, min_strand_reads, strand_num, strand_den, min_ref_reads;
    float min_var[NCOL], min_ref[NCOL];                    // per tested column (C_POS ..): the side's threshold (C_MMQ of min_var: the maximum; of min_ref: unused)
    float max_mmqs_diff, max_mapq_diff, max_rl_diff;
    uint32_t on[ON_WORDS];
    uint32_t *head, *next;                                 // scratch: head [n] the first record of an element's list (NONE32: none), next [n_xagg]; nullptr without records
    uint32_t *o_fail, *o_keep; float* o_vals; uint32_t* status;
};

// the six tested columns of a side, in vals' order
enum { C_POS, C_3P, C_BQ, C_MAPQ, C_MMQ, C_CLIP };
// what the tests read of one bucket
struct Side { uint32_t C, P, M; float m[NCOL]; };

inline uint64_t blocks_of(uint64_t n) { return (n + BLOCK - 1) / BLOCK; }
inline int64_t workspace_bytes(const brc_device_view* v, int64_t n) {
    if (!v || n <= 0 || !v->n_xagg) return 0;
    return (int64_t)(((uint64_t)n + v->n_xagg) * 4u);
}

BRCD_HD bool lib_on(const Job& J, int l) { return (J.on[l >> 5] >> (l & 31)) & 1u; }

BRCD_HD uint32_t exchange(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicExch(p, v);
#else
    const uint32_t o = *p; *p = v; return o;
#endif
}
BRCD_HD void status_or(uint32_t* p, uint32_t bits) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicOr(p, bits);
#else
    *p |= bits;
#endif
}

// first element of idx[0, hi) that is not below k: a SIGNED compare, so entries outside the planes sort to the two ends; the result
// never leaves [0, hi], sorted list or not
BRCD_HD int64_t lower_bound(const int32_t* idx, int64_t hi, int64_t k) {
    int64_t lo = 0;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)idx[mid] < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Lane = third-allele record r (head preset to NONE32): overlay_lane's bounds (brc_panel_core.h), and a base bucket only.
BRCD_HD void link_lane(const Job& J, uint64_t r) {
    const uint32_t k = J.xagg[r].k, lb = J.xagg[r].lib_b;
    if (k == NONE32) return;
    const int64_t l = lb >> 8; const uint32_t b = lb & 0xffu;
    if (l >= J.Lp || b < 1u || b > 4u || (int64_t)k >= J.P) return;
    const int64_t j = lower_bound(J.idx, J.n, (int64_t)k);
    if (j >= J.n || (int64_t)J.idx[j] != (int64_t)k) return;
    J.next[r] = exchange(J.head + j, (uint32_t)r);
}

// reference character of plane index k -> its base bucket 1..4, 0: none of ACGTacgt (ref_bucket of brc_select_core.h)
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

// the tested part of the thirteen columns of one bucket's sums
BRCD_HD Side side_of(const uint32_t* vi, const float* vf) {
    float m[NM];
    metrics13(vi, vf, m);
    Side s;
    s.C = vi[I_N]; s.P = vi[I_PLUS]; s.M = vi[I_MINUS];
    s.m[C_POS] = m[BRC_M_AVG_POS]; s.m[C_3P] = m[BRC_M_AVG_3P]; s.m[C_BQ] = m[BRC_M_AVG_BQ]; s.m[C_MAPQ] = m[BRC_M_AVG_MAPQ];
    s.m[C_MMQ] = m[BRC_M_AVG_MMQ]; s.m[C_CLIP] = m[BRC_M_AVG_CLIPPED];
    return s;
}

// Bucket b (1..4) of library l at plane index k: the two slots with expand_lane's order of writes, then the element's record of that
// (library, bucket) where there is one.
BRCD_HD Side bucket_side(const Job& J, int l, uint32_t b, uint32_t b0, uint32_t b1, const uint32_t (*si)[NI], const float (*sf)[NF], uint32_t first) {
    const bool in0 = b0 == b, in1 = b1 == b;
    uint32_t vi[NI]; float vf[NF];
#pragma unroll
    for (int f = 0; f < NI; ++f) {
        uint32_t v = 0u;
        if (in0 && si[0][f]) v = si[0][f];
        if (in1 && si[1][f]) v = si[1][f];
        vi[f] = v;
    }
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        float v = 0.0f;
        if (in0) v = sf[0][f];
        if (in1) v = sf[1][f];
        vf[f] = v;
    }
    for (uint32_t r = first; r != NONE32; r = J.next[r]) {
        if (J.xagg[r].lib_b != (((uint32_t)l << 8) | b)) continue;
        const Rec a = J.xagg[r];
#pragma unroll
        for (int f = 0; f < NI; ++f) vi[f] = a.i[f];
#pragma unroll
        for (int f = 0; f < NF; ++f) vf[f] = a.f[f];
    }
    return side_of(vi, vf);
}

// The tests of one (library, base): the failure word, and the twenty numbers behind it.  Every fp32 operation is one statement of its
// own; the translation unit is compiled with -ffp-contract=off, so none is fused with its neighbour.
BRCD_HD uint32_t judge(const Job& J, uint32_t D, const Side& V, const Side& R, float* val) {
    uint32_t f = 0u;
    const uint64_t S = (uint64_t)V.P + V.M, lo = V.P < V.M ? V.P : V.M;
    if (D < J.min_depth) f |= BRC_VET_DEPTH;
    if (V.C < J.min_var_count) f |= BRC_VET_VAR_COUNT;
    if ((uint64_t)V.C * J.freq_den < (uint64_t)J.freq_num * D) f |= BRC_VET_VAR_FREQ;
    if (S >= J.min_strand_reads && lo * J.strand_den < (uint64_t)J.strand_num * S) f |= BRC_VET_STRAND;
    const bool var = V.C > 0u, ref = R.C >= J.min_ref_reads;
    if (var) {
        if (V.m[C_POS] < J.min_var[C_POS]) f |= BRC_VET_VAR_READPOS;
        if (V.m[C_3P] < J.min_var[C_3P]) f |= BRC_VET_VAR_DIST3;
        if (V.m[C_BQ] < J.min_var[C_BQ]) f |= BRC_VET_VAR_BQ;
        if (V.m[C_MAPQ] < J.min_var[C_MAPQ]) f |= BRC_VET_VAR_MAPQ;
        if (V.m[C_MMQ] > J.min_var[C_MMQ]) f |= BRC_VET_VAR_MMQS;
        if (V.m[C_CLIP] < J.min_var[C_CLIP]) f |= BRC_VET_VAR_RL;
    }
    if (ref) {
        if (R.m[C_POS] < J.min_ref[C_POS]) f |= BRC_VET_REF_READPOS;
        if (R.m[C_3P] < J.min_ref[C_3P]) f |= BRC_VET_REF_DIST3;
        if (R.m[C_BQ] < J.min_ref[C_BQ]) f |= BRC_VET_REF_BQ;
        if (R.m[C_MAPQ] < J.min_ref[C_MAPQ]) f |= BRC_VET_REF_MAPQ;
        if (R.m[C_CLIP] < J.min_ref[C_CLIP]) f |= BRC_VET_REF_RL;
    }
    const float mmqs_diff = V.m[C_MMQ] - R.m[C_MMQ];
    const float mapq_diff = R.m[C_MAPQ] - V.m[C_MAPQ];
    const float rl_diff = R.m[C_CLIP] - V.m[C_CLIP];
    const float rl_bound = J.max_rl_diff * R.m[C_CLIP];
    if (var && ref) {
        if (mmqs_diff > J.max_mmqs_diff) f |= BRC_VET_MMQS_DIFF;
        if (mapq_diff > J.max_mapq_diff) f |= BRC_VET_MAPQ_DIFF;
        if (rl_diff > rl_bound) f |= BRC_VET_RL_DIFF;
    }
    val[BRC_VET_V_CV] = (float)V.C; val[BRC_VET_V_CR] = (float)R.C; val[BRC_VET_V_D] = (float)D;
    val[BRC_VET_V_FREQ] = D ? (float)V.C / (float)D : 0.0f;
    val[BRC_VET_V_STRAND] = S ? (float)V.P / (float)S : 0.0f;
    val[BRC_VET_V_MMQS_DIFF] = mmqs_diff; val[BRC_VET_V_MAPQ_DIFF] = mapq_diff; val[BRC_VET_V_RL_DIFF] = rl_diff;
#pragma unroll
    for (int c = 0; c < NCOL; ++c) { val[BRC_VET_V_VAR + c] = V.m[c]; val[BRC_VET_V_REF + c] = R.m[c]; }
    return f & J.tests;
}

// the stores of one (library, base) at element j
BRCD_HD void store_lane(const Job& J, int l, uint32_t v, int64_t j, uint32_t f, const float* val) {
    const int64_t lv = (int64_t)l * 4 + v;
    if (J.o_fail) put(J.o_fail + lv * J.DS + j, f);
    if (J.o_vals) {
#pragma unroll
        for (int c = 0; c < NVAL; ++c) put(J.o_vals + (lv * NVAL + c) * J.DS + j, val[c]);
    }
}

// Lane = list element j (after every link_lane of the call).  Neighbouring lanes load neighbouring words of idx and alt and store
// neighbouring words of every destination plane: a wave's stores are runs of 256 contiguous bytes whatever the list holds; its plane
// loads meet in a cache line exactly when its positions do.  The list is judged once per element (range, order against the element
// before).  An element that repeats its neighbour's index finds the list of the first of them by the records' own binary search.
BRCD_HD void sites_lane(const Job& J, int64_t j) {
    const int64_t k = J.idx[j];
    const bool in = k >= 0 && k < J.P;
    const bool twin = j > 0 && (int64_t)J.idx[j - 1] == k;
    if (J.status) {
        uint32_t bits = in ? 0u : BRC_VET_OUT_OF_RANGE;
        if (j > 0 && (int64_t)J.idx[j - 1] > k) bits |= BRC_VET_NOT_ASCENDING;
        if (bits) status_or(J.status, bits);
    }
    if (!J.o_fail && !J.o_keep && !J.o_vals) return;
    const uint32_t asked = J.alt ? J.alt[j] & 0xfu : 0xfu;
    const uint32_t rb = in ? ref_bucket(J, k) : 0u;
    uint32_t first = NONE32;
    if (J.head && in) first = J.head[twin ? lower_bound(J.idx, j, k) : j];
    uint32_t keep = 0u;
    for (int l = 0; l < J.Lp; ++l) {
        const bool on = lib_on(J, l);                       // (uniform over the wave)
        const uint32_t nothing = !on ? BRC_VET_NOT_ASKED : !rb ? BRC_VET_NO_SITE : 0u;
        if (nothing) {                                      // nothing of the library is loaded
            float zero[NVAL];
#pragma unroll
            for (int c = 0; c < NVAL; ++c) zero[c] = 0.0f;
#pragma unroll
            for (uint32_t v = 0; v < 4u; ++v) store_lane(J, l, v, j, nothing, zero);
            continue;
        }
        const int64_t row = (int64_t)l * J.PS + k;
        const uint32_t D = J.depth[row], sid = J.slotid[row], b0 = sid & 0xffu, b1 = (sid >> 8) & 0xffu;
        uint32_t si[2][NI]; float sf[2][NF];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
#pragma unroll
            for (int f = 0; f < NI; ++f) si[s][f] = J.si[(((int64_t)l * 2 + s) * NI + f) * J.PS + k];
#pragma unroll
            for (int f = 0; f < NF; ++f) sf[s][f] = J.sf[(((int64_t)l * 2 + s) * NF + f) * J.PS + k];
        }
        const Side R = bucket_side(J, l, rb, b0, b1, si, sf, first);
#pragma unroll
        for (uint32_t v = 0; v < 4u; ++v) {
            uint32_t f = BRC_VET_NOT_ASKED;
            float val[NVAL];
#pragma unroll
            for (int c = 0; c < NVAL; ++c) val[c] = 0.0f;
            if (((asked >> v) & 1u) && rb != v + 1u) {
                const Side V = bucket_side(J, l, v + 1u, b0, b1, si, sf, first);
                f = judge(J, D, V, R, val);
                if (!f) keep |= 1u << v;
            }
            store_lane(J, l, v, j, f, val);
        }
    }
    if (J.o_keep) put(J.o_keep + j, keep);
}

BRCD_HD bool finite32(float x) {
    union { float f; uint32_t u; } b; b.f = x;
    return (b.u & 0x7f800000u) != 0x7f800000u;
}

// The argument checks of brc_vet_sites (everything but the kind of memory, which the two libraries check themselves): 0 = fine.
inline int check_job(const brc_device_view* v, const brc_device_indels* d, const brc_vet_params* p, const int32_t* idx, int64_t n, int64_t dst_stride,
                     const void* ws, const char** why) {
    if (!v || !d) { *why = "no view"; return BRC_E_ARG; }
    if (!p) { *why = "no parameters"; return BRC_E_ARG; }
    if (v->n_lib < 1 || v->n_pos < 0 || v->stride < v->n_pos || d->n_lib < 1 || d->n_pos < 0) { *why = "not a view of a computed region"; return BRC_E_ARG; }
    if (v->memory != d->memory || v->device != d->device || v->n_lib != d->n_lib || v->pos0 != d->pos0 || v->n_pos != d->n_pos) {
        *why = "the two views are not of one region"; return BRC_E_ARG;
    }
    if (v->n_lib > BRC_VET_MAX_LIB) { *why = "more libraries than BRC_VET_MAX_LIB"; return BRC_E_ARG; }
    if (n < 0) { *why = "n below 0"; return BRC_E_ARG; }
    if (v->n_xagg >= 0xfffffff0ull || (uint64_t)n >= 0x7ffffff0ull) { *why = "list too large: records and elements are indexed with 32 bits"; return BRC_E_ARG; }
    if (n > 0 && !idx) { *why = "no index list"; return BRC_E_ARG; }
    if (dst_stride < n) { *why = "dst_stride below n"; return BRC_E_ARG; }
    if (n > 0 && (!v->ncol || !v->depth || !v->slotid || !v->si || !v->sf)) { *why = "a view without planes"; return BRC_E_ARG; }
    if (v->n_xagg && !v->xagg) { *why = "a view without its third-allele records"; return BRC_E_ARG; }
    if (d->n_slots && (!d->slots || !d->seq4 || !d->seq_off || !d->l_qseq || d->n_reads < 0)) { *why = "a view with records but without its arrays"; return BRC_E_ARG; }
    if (p->tests & ~BRC_VET_ALL_TESTS) { *why = "tests: a mask of BRC_VET_DEPTH .. BRC_VET_RL_DIFF"; return BRC_E_ARG; }
    if (p->freq_den == 0u || p->strand_den == 0u) { *why = "freq_den and strand_den must not be 0"; return BRC_E_ARG; }
    const float thr[] = {p->min_var_readpos, p->min_var_dist3, p->min_var_bq, p->min_var_mapq, p->max_var_mmqs, p->min_var_rl, p->min_ref_readpos,
                         p->min_ref_dist3, p->min_ref_bq, p->min_ref_mapq, p->min_ref_rl, p->max_mmqs_diff, p->max_mapq_diff, p->max_rl_diff};
    for (float t : thr) if (!finite32(t)) { *why = "a threshold that is not finite"; return BRC_E_ARG; }
    bool any = !p->lib_on;
    for (int l = 0; p->lib_on && l < v->n_lib; ++l) {
        if (p->lib_on[l] > 1) { *why = "a lib_on entry above 1"; return BRC_E_ARG; }
        any = any || p->lib_on[l] == 1;
    }
    if (!any) { *why = "no judged library"; return BRC_E_ARG; }
    if (n > 0 && !ws) { *why = "no workspace"; return BRC_E_ARG; }
    return BRC_OK;
}
inline Job make_job(const brc_device_view* v, const brc_device_indels* d, const brc_vet_params* p, const int32_t* idx, const uint32_t* alt, int64_t n,
                    int64_t dst_stride, uint32_t* fail, uint32_t* keep, float* vals, uint32_t* status, void* ws) {
    Job J;
    J.depth = v->depth; J.slotid = v->slotid; J.si = v->si; J.sf = v->sf; J.xagg = (const Rec*)v->xagg; J.n_xagg = v->n_xagg;
    J.ref = d->ref; J.ref_lo = d->ref_lo; J.ref_hi = d->ref_hi; J.ref_len = d->ref_len;
    J.Lp = v->n_lib; J.pos0 = v->pos0; J.P = v->n_pos; J.PS = v->stride;
    J.idx = idx; J.alt = alt; J.n = n; J.DS = dst_stride;
    J.tests = p->tests;
    J.min_depth = p->min_depth; J.min_var_count = p->min_var_count; J.freq_num = p->freq_num; J.freq_den = p->freq_den;
    J.min_strand_reads = p->min_strand_reads; J.strand_num = p->strand_num; J.strand_den = p->strand_den; J.min_ref_reads = p->min_ref_reads;
    J.min_var[C_POS] = p->min_var_readpos; J.min_var[C_3P] = p->min_var_dist3; J.min_var[C_BQ] = p->min_var_bq; J.min_var[C_MAPQ] = p->min_var_mapq;
    J.min_var[C_MMQ] = p->max_var_mmqs; J.min_var[C_CLIP] = p->min_var_rl;
    J.min_ref[C_POS] = p->min_ref_readpos; J.min_ref[C_3P] = p->min_ref_dist3; J.min_ref[C_BQ] = p->min_ref_bq; J.min_ref[C_MAPQ] = p->min_ref_mapq;
    J.min_ref[C_MMQ] = 0.0f; J.min_ref[C_CLIP] = p->min_ref_rl;
    J.max_mmqs_diff = p->max_mmqs_diff; J.max_mapq_diff = p->max_mapq_diff; J.max_rl_diff = p->max_rl_diff;
    for (int w = 0; w < ON_WORDS; ++w) J.on[w] = 0u;
    for (int l = 0; l < v->n_lib; ++l) if (!p->lib_on || p->lib_on[l]) J.on[l >> 5] |= 1u << (l & 31);
    const bool chain = v->n_xagg != 0 && (fail || keep || vals);
    J.head = chain ? (uint32_t*)ws : nullptr;
    J.next = chain ? (uint32_t*)ws + n : nullptr;
    J.o_fail = fail; J.o_keep = keep; J.o_vals = vals; J.status = status;
    return J;
}
inline bool wants_dests(const Job& J) { return J.o_fail || J.o_keep || J.o_vals; }
inline bool walks_records(const Job& J) { return J.head != nullptr; }
// bytes the kernels ask for / write (brc_vet_last_timing)
inline void job_bytes(const Job& J, uint64_t* rd, uint64_t* wr) {
    const uint64_t n = (uint64_t)J.n, Lp = (uint64_t)J.Lp, chain = walks_records(J) ? 1u : 0u, dests = wants_dests(J) ? 1u : 0u;
    uint64_t L = 0;
    for (int l = 0; l < J.Lp; ++l) L += lib_on(J, l);
    *rd = 4u * n * (1u + (J.status ? 1u : 0u) + dests * ((J.alt ? 1u : 0u) + L * (2u + 2u * (NI + NF)) + chain)) + n * dests + 64u * J.n_xagg * chain;
    *wr = 4u * n * (Lp * 4u * ((J.o_fail ? 1u : 0u) + (J.o_vals ? (uint64_t)NVAL : 0u)) + (J.o_keep ? 1u : 0u) + chain) + 4u * J.n_xagg * chain;
}

}  // namespace brcvet
#endif
