// brc_panel_core.h — per-lane functions of the device-resident site panels (include/brc_panel.h), written once for the gfx950 kernels
// (brc_panel.hip) and for the CPU build the tests run (tests/sim_panel): brc_dense_core.h's expand_lane / overlay_lane with the plane
// index read from a list instead of counted from a window's start — what expand_slots (brc_host.cpp) does for one listed (position,
// library) or one XAgg record at a time.
//
// Rec, metrics13 and put are brc_dense_core.h's; layouts are restated by their strides, nothing of the engine is included.
#ifndef BRC_PANEL_CORE_H
#define BRC_PANEL_CORE_H

#include <stdint.h>

#include "../../include/brc_panel.h"
#include "brc_dense_core.h"

namespace brcpanel {

using brcdense::I_N;
using brcdense::metrics13;
using brcdense::NB;
using brcdense::NF;
using brcdense::NI;
using brcdense::NM;
using brcdense::NONE32;
using brcdense::put;
using brcdense::Rec;

enum { BLOCK = 256 };                                      // lanes of a workgroup of both kernels
static const int64_t MAX_N = (int64_t)0x7fffffff * BLOCK;  // one launch: 2^31 - 1 workgroups

// One call's work: the view, the list, the destinations (any of them nullptr: not wanted).
struct Job {
    const uint32_t *ncol, *depth, *slotid, *si, *unavail; const float* sf;      // the view's planes, PS elements apart
    const Rec* xagg; uint64_t n_xagg;
    int32_t Lp; int64_t P, PS;
    const int32_t* idx; int64_t n, DS;                                          // element j is plane index idx[j]; destination planes DS elements apart
    uint32_t *o_ncol, *o_depth, *o_unavail, *o_istat; float *o_fstat, *o_metrics;
    uint32_t* status;
};

BRCD_HD void status_or(uint32_t* p, uint32_t bits) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicOr(p, bits);
#else
    *p |= bits;
#endif
}

// Lane = list element j of library l: ONE load of idx[j] (neighbouring lanes, neighbouring words), then expand_lane's loads at that
// index — neighbouring lanes meet in a cache line exactly when their positions do — and expand_lane's stores at j: the stores of a
// wave stay runs of 256 contiguous bytes whatever the list holds.  An index outside the planes loads nothing and stores an empty
// position.  Library 0's lanes also judge the list (range, order against the element before).
BRCD_HD void gather_lane(const Job& J, int l, int64_t j) {
    const int64_t k = J.idx[j];
    const bool in = k >= 0 && k < J.P;
    if (l == 0 && J.status) {
        uint32_t bits = in ? 0u : BRC_PANEL_OUT_OF_RANGE;
        if (j > 0 && J.idx[j - 1] > (int32_t)k) bits |= BRC_PANEL_NOT_ASCENDING;
        if (bits) status_or(J.status, bits);
    }
    const int64_t row = (int64_t)l * J.PS + k;
    if (J.o_ncol) put(J.o_ncol + (int64_t)l * J.DS + j, in ? J.ncol[row] : 0u);
    if (J.o_depth) put(J.o_depth + (int64_t)l * J.DS + j, in ? J.depth[row] : 0u);
    if (J.o_unavail && l == 0) put(J.o_unavail + j, (in && J.unavail) ? J.unavail[k] : NONE32);
    if (!J.o_istat && !J.o_fstat && !J.o_metrics) return;
    const uint32_t sid = in ? J.slotid[row] : 0xffffu;                          // (0xff: no bucket)
    const uint32_t b0 = sid & 0xffu, b1 = (sid >> 8) & 0xffu;
    uint32_t si[2][NI]; float sf[2][NF];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int f = 0; f < NI; ++f) si[s][f] = in ? J.si[(((int64_t)l * 2 + s) * NI + f) * J.PS + k] : 0u;
#pragma unroll
        for (int f = 0; f < NF; ++f) sf[s][f] = in ? J.sf[(((int64_t)l * 2 + s) * NF + f) * J.PS + k] : 0.0f;
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const bool in0 = b0 == (uint32_t)b, in1 = b1 == (uint32_t)b;
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
        const int64_t lb = (int64_t)l * NB + b;
        if (J.o_istat) {
#pragma unroll
            for (int f = 0; f < NI; ++f) put(J.o_istat + (lb * NI + f) * J.DS + j, vi[f]);
        }
        if (J.o_fstat) {
#pragma unroll
            for (int f = 0; f < NF; ++f) put(J.o_fstat + (lb * NF + f) * J.DS + j, vf[f]);
        }
        if (J.o_metrics) {
            float m[NM];
            metrics13(vi, vf, m);
#pragma unroll
            for (int f = 0; f < NM; ++f) put(J.o_metrics + (lb * NM + f) * J.DS + j, m[f]);
        }
    }
}

// Lane = third-allele record r (after every gather_lane of the call): a used record inside the planes looks for the first element
// that lists its position — a binary search over idx with a SIGNED compare, so entries outside the planes sort to the two ends and
// never match — and overwrites its bucket's 13 values there and in every equal neighbour behind it.  j never leaves [0, n), sorted
// list or not.
BRCD_HD void overlay_lane(const Job& J, uint64_t r) {
    const Rec a = J.xagg[r];
    if (a.k == NONE32) return;
    const int64_t l = a.lib_b >> 8, k = a.k; const uint32_t b = a.lib_b & 0xffu;
    if (l >= J.Lp || b >= (uint32_t)NB || k >= J.P) return;
    int64_t lo = 0, hi = J.n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)J.idx[mid] < k) lo = mid + 1; else hi = mid;
    }
    const int64_t lb = l * NB + b;
    float m[NM];
    if (J.o_metrics) metrics13(a.i, a.f, m);
    for (int64_t j = lo; j < J.n && (int64_t)J.idx[j] == k; ++j) {
        if (J.o_istat) for (int f = 0; f < NI; ++f) J.o_istat[(lb * NI + f) * J.DS + j] = a.i[f];
        if (J.o_fstat) for (int f = 0; f < NF; ++f) J.o_fstat[(lb * NF + f) * J.DS + j] = a.f[f];
        if (J.o_metrics) for (int f = 0; f < NM; ++f) J.o_metrics[(lb * NM + f) * J.DS + j] = m[f];
    }
}

// The argument checks of brc_panel_gather (everything but the kind of memory, which the two libraries check themselves): 0 = fine.
inline int check_job(const brc_device_view* v, const int32_t* idx, int64_t n, int64_t dst_stride, const char** why) {
    if (!v) { *why = "no view"; return BRC_E_ARG; }
    if (v->n_lib < 1 || v->n_pos < 0 || v->stride < v->n_pos) { *why = "not a view of a computed region"; return BRC_E_ARG; }
    if (n < 0) { *why = "n below 0"; return BRC_E_ARG; }
    if (n > MAX_N || v->n_lib > 65535 || (v->n_xagg + BLOCK - 1) / BLOCK > 0x7fffffffULL) { *why = "list too large for one launch"; return BRC_E_ARG; }
    if (n > 0 && !idx) { *why = "no index list"; return BRC_E_ARG; }
    if (dst_stride < n) { *why = "dst_stride below n"; return BRC_E_ARG; }
    if (n > 0 && (!v->ncol || !v->depth || !v->slotid || !v->si || !v->sf)) { *why = "a view without planes"; return BRC_E_ARG; }
    if (v->n_xagg && !v->xagg) { *why = "a view without its third-allele records"; return BRC_E_ARG; }
    return BRC_OK;
}
inline Job make_job(const brc_device_view* v, const int32_t* idx, int64_t n, int64_t dst_stride, uint32_t* ncol, uint32_t* depth, uint32_t* unavail,
                    uint32_t* istat, float* fstat, float* metrics, uint32_t* status) {
    Job J;
    J.ncol = v->ncol; J.depth = v->depth; J.slotid = v->slotid; J.si = v->si; J.unavail = v->unavail; J.sf = v->sf;
    J.xagg = (const Rec*)v->xagg; J.n_xagg = v->n_xagg;
    J.Lp = v->n_lib; J.P = v->n_pos; J.PS = v->stride; J.idx = idx; J.n = n; J.DS = dst_stride;
    J.o_ncol = ncol; J.o_depth = depth; J.o_unavail = unavail; J.o_istat = istat; J.o_fstat = fstat; J.o_metrics = metrics;
    J.status = status;
    return J;
}
inline bool wants_buckets(const Job& J) { return J.o_istat || J.o_fstat || J.o_metrics; }
// bytes the planes kernel asks for / writes for a job (brc_panel_last_timing); the list and the records are counted as read
inline void job_bytes(const Job& J, uint64_t* rd, uint64_t* wr) {
    const uint64_t n = (uint64_t)J.n, L = (uint64_t)J.Lp;
    const bool slots = wants_buckets(J);
    *rd = 4u * n * (L * (1u + (J.o_ncol ? 1u : 0u) + (J.o_depth ? 1u : 0u) + (slots ? 1u + 2u * (NI + NF) : 0u)) + ((J.o_unavail && J.unavail) ? 1u : 0u)) +
          (slots ? 64u * J.n_xagg : 0u);
    *wr = 4u * n * (L * ((J.o_ncol ? 1u : 0u) + (J.o_depth ? 1u : 0u) + (uint64_t)NB * ((J.o_istat ? NI : 0) + (J.o_fstat ? NF : 0) + (J.o_metrics ? NM : 0))) +
                    (J.o_unavail ? 1u : 0u));
}

}  // namespace brcpanel
#endif
