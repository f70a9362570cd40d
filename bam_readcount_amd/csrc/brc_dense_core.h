// brc_dense_core.h — per-lane functions of the device-resident results (include/brc_dense.h), written once for the gfx950 kernels
// (brc_dense.hip) and for the CPU build the tests run (tests/sim_dense): what expand_slots (brc_host.cpp) does on the host, and the
// thirteen printed columns of operator<<(BasicStat) (BasicStat.cpp:110-159), for one (position, library) or one XAgg record at a time.
//
// Layouts are those of struct Planes / XAgg (brc_core.h), restated here by their strides so that this header includes nothing of
// the engine: the view (brc_device_view, include/brc.h) is plain data.
#ifndef BRC_DENSE_CORE_H
#define BRC_DENSE_CORE_H

#include <stdint.h>

#include "../../include/brc_dense.h"

#if defined(__HIPCC__)
#define BRCD_HD __host__ __device__ inline
#else
#define BRCD_HD inline
#endif

namespace brcdense {

enum { NB = BRC_NBUCKET, NI = BRC_NI, NF = BRC_NF, NM = BRC_NMETRIC };
static const uint32_t NONE32 = 0xFFFFFFFFu;
// integer / float plane order (include/brc.h)
enum { I_N = BRC_I_N, I_SMQ = BRC_I_SMQ, I_SSE = BRC_I_SSE, I_PLUS = BRC_I_PLUS, I_MINUS = BRC_I_MINUS, I_NQ2 = BRC_I_NQ2, I_SMMQ = BRC_I_SMMQ,
       I_SCLIP = BRC_I_SCLIP, I_SBQ = BRC_I_SBQ };
enum { F_SEV = BRC_F_SEV, F_SQ2 = BRC_F_SQ2, F_SNM = BRC_F_SNM, F_S3P = BRC_F_S3P };

// struct XAgg of brc_core.h, as the view hands it over (64 bytes)
struct alignas(16) Rec { uint32_t k; uint32_t lib_b; uint32_t i[NI]; float f[NF]; uint32_t pad; };
static_assert(sizeof(Rec) == 64, "a third-allele record is 64 bytes");

// One call's work: the view, the window, the destinations (any of them nullptr: not wanted).
struct Job {
    const uint32_t *ncol, *depth, *slotid, *si, *unavail; const float* sf;      // the view's planes, PS elements apart
    const Rec* xagg; uint64_t n_xagg;
    int32_t Lp; int64_t P, PS;
    int64_t k0, n, DS;                                                          // window [k0, k0 + n), destination planes DS elements apart
    uint32_t *o_ncol, *o_depth, *o_unavail, *o_istat; float *o_fstat, *o_metrics;
};

// A plane store: every destination element is written once and not read again by this library — on the device the store goes
// past the caches' retention (non-temporal), the 256 contiguous bytes of a wave's 64 lanes as one run.
template <class T> BRCD_HD void put(T* p, T v) {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_nontemporal_store(v, p);
#else
    *p = v;
#endif
}

// The thirteen printed columns of one bucket (operator<<(BasicStat), BasicStat.cpp:117-140; fmt_stat, brc_host.cpp): every average
// is one fp32 division of the converted sum by the converted count.
BRCD_HD void metrics13(const uint32_t* si, const float* sf, float* m) {
    const uint32_t cnt = si[I_N];
    if (cnt == 0u) { for (int f = 0; f < NM; ++f) m[f] = 0.0f; return; }
    const float c = (float)cnt;
    m[BRC_M_COUNT] = c;
    m[BRC_M_AVG_MAPQ] = (float)si[I_SMQ] / c;
    m[BRC_M_AVG_BQ] = (float)si[I_SBQ] / c;
    m[BRC_M_AVG_SE_MAPQ] = (float)si[I_SSE] / c;
    m[BRC_M_PLUS] = (float)si[I_PLUS];
    m[BRC_M_MINUS] = (float)si[I_MINUS];
    m[BRC_M_AVG_POS] = sf[F_SEV] / c;
    m[BRC_M_AVG_NM] = sf[F_SNM] / c;
    m[BRC_M_AVG_MMQ] = (float)si[I_SMMQ] / c;
    m[BRC_M_NQ2] = (float)si[I_NQ2];
    m[BRC_M_AVG_Q2_DIST] = si[I_NQ2] > 0u ? sf[F_SQ2] / (float)si[I_NQ2] : 0.0f;
    m[BRC_M_AVG_CLIPPED] = (float)si[I_SCLIP] / c;
    m[BRC_M_AVG_3P] = sf[F_S3P] / c;
}

// Lane = window element j of library l: the position's two slots -> its six buckets, in expand_slots' order of writes (zero; slot 0;
// slot 1 — integers where non-zero, floats unconditionally).  26 loads (+ slotid), 78 stores per wanted kind; neighbouring lanes
// load and store neighbouring elements of every plane.
BRCD_HD void expand_lane(const Job& J, int l, int64_t j) {
    const int64_t k = J.k0 + j, row = (int64_t)l * J.PS + k;
    if (J.o_ncol) put(J.o_ncol + (int64_t)l * J.DS + j, J.ncol[row]);
    if (J.o_depth) put(J.o_depth + (int64_t)l * J.DS + j, J.depth[row]);
    if (J.o_unavail && l == 0) put(J.o_unavail + j, J.unavail ? J.unavail[k] : NONE32);
    if (!J.o_istat && !J.o_fstat && !J.o_metrics) return;
    const uint32_t sid = J.slotid[row];
    const uint32_t b0 = sid & 0xffu, b1 = (sid >> 8) & 0xffu;
    uint32_t si[2][NI]; float sf[2][NF];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int f = 0; f < NI; ++f) si[s][f] = J.si[(((int64_t)l * 2 + s) * NI + f) * J.PS + k];
#pragma unroll
        for (int f = 0; f < NF; ++f) sf[s][f] = J.sf[(((int64_t)l * 2 + s) * NF + f) * J.PS + k];
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

// Lane = third-allele record r (after every expand_lane of the call): a used record whose position lies in the window overwrites
// its bucket's 13 values — expand_slots' last loop, with its bounds.
BRCD_HD void overlay_lane(const Job& J, uint64_t r) {
    const Rec a = J.xagg[r];
    if (a.k == NONE32) return;
    const int64_t l = a.lib_b >> 8, k = a.k; const uint32_t b = a.lib_b & 0xffu;
    if (l >= J.Lp || b >= (uint32_t)NB || k >= J.P || k < J.k0 || k >= J.k0 + J.n) return;
    const int64_t j = k - J.k0, lb = l * NB + b;
    if (J.o_istat) for (int f = 0; f < NI; ++f) J.o_istat[(lb * NI + f) * J.DS + j] = a.i[f];
    if (J.o_fstat) for (int f = 0; f < NF; ++f) J.o_fstat[(lb * NF + f) * J.DS + j] = a.f[f];
    if (J.o_metrics) {
        float m[NM];
        metrics13(a.i, a.f, m);
        for (int f = 0; f < NM; ++f) J.o_metrics[(lb * NM + f) * J.DS + j] = m[f];
    }
}

// The argument checks of brc_dense_expand (everything but the kind of memory, which the two libraries check themselves): 0 = fine.
inline int check_job(const brc_device_view* v, int64_t k0, int64_t n, int64_t dst_stride, const char** why) {
    if (!v) { *why = "no view"; return BRC_E_ARG; }
    if (v->n_lib < 1 || v->n_pos < 0 || v->stride < v->n_pos) { *why = "not a view of a computed region"; return BRC_E_ARG; }
    if (k0 < 0 || n < 0 || k0 > v->n_pos || n > v->n_pos - k0) { *why = "the window must lie inside the view's planes"; return BRC_E_ARG; }
    if (dst_stride < n) { *why = "dst_stride below n"; return BRC_E_ARG; }
    if (n > 0 && (!v->ncol || !v->depth || !v->slotid || !v->si || !v->sf)) { *why = "a view without planes"; return BRC_E_ARG; }
    if (v->n_xagg && !v->xagg) { *why = "a view without its third-allele records"; return BRC_E_ARG; }
    return BRC_OK;
}
inline Job make_job(const brc_device_view* v, int64_t k0, int64_t n, int64_t dst_stride, uint32_t* ncol, uint32_t* depth, uint32_t* unavail,
                    uint32_t* istat, float* fstat, float* metrics) {
    Job J;
    J.ncol = v->ncol; J.depth = v->depth; J.slotid = v->slotid; J.si = v->si; J.unavail = v->unavail; J.sf = v->sf;
    J.xagg = (const Rec*)v->xagg; J.n_xagg = v->n_xagg;
    J.Lp = v->n_lib; J.P = v->n_pos; J.PS = v->stride; J.k0 = k0; J.n = n; J.DS = dst_stride;
    J.o_ncol = ncol; J.o_depth = depth; J.o_unavail = unavail; J.o_istat = istat; J.o_fstat = fstat; J.o_metrics = metrics;
    return J;
}
// bytes the planes kernel reads / writes for a job (brc_dense_last_timing); the records are counted as read
inline void job_bytes(const Job& J, uint64_t* rd, uint64_t* wr) {
    const uint64_t n = (uint64_t)J.n, L = (uint64_t)J.Lp;
    const bool slots = J.o_istat || J.o_fstat || J.o_metrics;
    *rd = 4u * n * (L * ((J.o_ncol ? 1u : 0u) + (J.o_depth ? 1u : 0u) + (slots ? 1u + 2u * (NI + NF) : 0u)) + ((J.o_unavail && J.unavail) ? 1u : 0u)) +
          (slots ? 64u * J.n_xagg : 0u);
    *wr = 4u * n * (L * ((J.o_ncol ? 1u : 0u) + (J.o_depth ? 1u : 0u) + (uint64_t)NB * ((J.o_istat ? NI : 0) + (J.o_fstat ? NF : 0) + (J.o_metrics ? NM : 0))) +
                    (J.o_unavail ? 1u : 0u));
}

}  // namespace brcdense
#endif
