// brc_panel.hip — device-resident site panels for gfx950 behind the C-ABI of include/brc_panel.h (libbrc_panel_hip.so; a translation
// unit and a library of its own: the engine's libraries keep exactly the device code they had, and this one links nothing of the engine).
//
// Per call, on the caller's stream: the status word's clear, then two launches —
//   k_panel_planes   lane == list element j, wave == (64 consecutive elements, library), blockIdx.y == library: one coalesced load of
//                    idx[j], the 27 plane loads of the dense expansion at that index (listed neighbours share their cache lines, an
//                    isolated site pays a line per word), and the dense expansion's stores at j: every plane store of a wave is
//                    one run of 256 contiguous bytes, non-temporal.  Library 0's lanes also judge the list.  No LDS.
//   k_panel_overlay  lane == third-allele record: a binary search over idx, then its bucket's 13 values in every element that lists
//                    its position.  Launched only when the view has records and a bucket destination is wanted.
// The per-lane work is brc_panel_core.h, shared with the CPU build the tests run.  DESIGN.md 6e has the reasoning and the measurements.
#include <hip/hip_runtime.h>

#include "brc_panel_core.h"
#include "brc_side_hip.h"

using namespace brcpanel;

__global__ __launch_bounds__(BLOCK) void k_panel_planes(const Job J) {
    const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= J.n) return;
    gather_lane(J, (int)blockIdx.y, j);
}

__global__ __launch_bounds__(BLOCK) void k_panel_overlay(const Job J) {
    const uint64_t r = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (r >= J.n_xagg) return;
    overlay_lane(J, r);
}

struct brc_panel : brcside::Handle {};

extern "C" {

const char* brc_panel_kind(void) { return "hip-gfx950"; }
int brc_panel_create(int device, brc_panel** out) { return brcside::create(device, (const void*)k_panel_planes, out); }
void brc_panel_destroy(brc_panel* h) { brcside::destroy(h); }
const char* brc_panel_last_error(const brc_panel* h) { return brcside::last_error(h); }
void brc_panel_last_timing(const brc_panel* h, double* kernel_s, uint64_t* bytes_read, uint64_t* bytes_written) { brcside::last_timing(h, kernel_s, bytes_read, bytes_written); }

int brc_panel_gather(brc_panel* h, const brc_device_view* v, const int32_t* idx, int64_t n, int64_t dst_stride, uint32_t* ncol, uint32_t* depth,
                     uint32_t* unavail, uint32_t* istat, float* fstat, float* metrics, uint32_t* status, void* stream_) {
    if (!h) return BRC_E_ARG;
    brcside::clear(h);
    const char* why = "";
    if (check_job(v, idx, n, dst_stride, &why)) return brcside::refuse(h, why);
    if (int rc = brcside::resident(h, v, brcside::ONE_VIEW)) return rc;
    const bool dests = ncol || depth || unavail || istat || fstat || metrics;
    if (!status && (n == 0 || !dests)) return BRC_OK;
    hipStream_t stream = (hipStream_t)stream_;
    HIPOK(hipSetDevice(h->device));
    if (status) HIPOK(hipMemsetAsync(status, 0, sizeof(uint32_t), stream));
    if (n == 0) return BRC_OK;
    const Job J = make_job(v, idx, n, dst_stride, ncol, depth, unavail, istat, fstat, metrics, status);
    if (int rc = brcside::start(h, stream)) return rc;
    // (a call that wants the verdict alone needs library 0's lanes only)
    LAUNCH(k_panel_planes, dim3((unsigned)((n + BLOCK - 1) / BLOCK), dests ? (unsigned)v->n_lib : 1u), dim3(BLOCK), 0, stream, J);
    if (J.n_xagg && wants_buckets(J)) LAUNCH(k_panel_overlay, dim3((unsigned)((J.n_xagg + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, stream, J);
    return brcside::done(h, stream, J);
}

}  // extern "C"
