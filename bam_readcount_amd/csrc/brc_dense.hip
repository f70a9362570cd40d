// brc_dense.hip — device-resident results for gfx950 behind the C-ABI of include/brc_dense.h (libbrc_dense_hip.so; a translation
// unit and a library of its own: the engine's libraries keep exactly the device code they had, and this one links nothing of the engine).
//
// Two launches per call, on the caller's stream:
//   k_dense_planes   lane == position, wave == (64 positions, library): every load and every plane store of a wave is one run of
//                    256 contiguous bytes (aligned when k0, the view's stride and the destination are).  No LDS, no arithmetic to
//                    speak of: a copy with a 1 : 3 fan-out, whose yardstick is the copy rate.
//   k_dense_overlay  lane == third-allele record: the few buckets whose sums sit in the XAgg table overwrite their 13 values.
// The per-lane work is brc_dense_core.h, shared with the CPU build the tests run.  DESIGN.md 6c has the reasoning and the measurements.
#include <hip/hip_runtime.h>

#include "brc_dense_core.h"
#include "brc_side_hip.h"

using namespace brcdense;

enum { BLOCK = 256 };      // four waves: four tiles of 64 positions of one library

__global__ __launch_bounds__(BLOCK) void k_dense_planes(const Job J) {
    const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= J.n) return;
    expand_lane(J, (int)blockIdx.y, j);
}

__global__ __launch_bounds__(BLOCK) void k_dense_overlay(const Job J) {
    const uint64_t r = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (r >= J.n_xagg) return;
    overlay_lane(J, r);
}

struct brc_dense : brcside::Handle {};

extern "C" {

const char* brc_dense_kind(void) { return "hip-gfx950"; }
int brc_dense_create(int device, brc_dense** out) { return brcside::create(device, (const void*)k_dense_planes, out); }
void brc_dense_destroy(brc_dense* h) { brcside::destroy(h); }
const char* brc_dense_last_error(const brc_dense* h) { return brcside::last_error(h); }
void brc_dense_last_timing(const brc_dense* h, double* kernel_s, uint64_t* bytes_read, uint64_t* bytes_written) { brcside::last_timing(h, kernel_s, bytes_read, bytes_written); }

int brc_dense_expand(brc_dense* h, const brc_device_view* v, int64_t k0, int64_t n, int64_t dst_stride, uint32_t* ncol, uint32_t* depth,
                     uint32_t* unavail, uint32_t* istat, float* fstat, float* metrics, void* stream_) {
    if (!h) return BRC_E_ARG;
    brcside::clear(h);
    const char* why = "";
    if (check_job(v, k0, n, dst_stride, &why)) return brcside::refuse(h, why);
    if (int rc = brcside::resident(h, v, brcside::ONE_VIEW)) return rc;
    if (n == 0 || (!ncol && !depth && !unavail && !istat && !fstat && !metrics)) return BRC_OK;
    if ((n + BLOCK - 1) / BLOCK > 0x7fffffffLL || v->n_lib > 65535 || (v->n_xagg + BLOCK - 1) / BLOCK > 0x7fffffffULL) return brcside::refuse(h, "window too large for one launch");
    const Job J = make_job(v, k0, n, dst_stride, ncol, depth, unavail, istat, fstat, metrics);
    hipStream_t stream = (hipStream_t)stream_;
    HIPOK(hipSetDevice(h->device));
    if (int rc = brcside::start(h, stream)) return rc;
    LAUNCH(k_dense_planes, dim3((unsigned)((n + BLOCK - 1) / BLOCK), (unsigned)v->n_lib), dim3(BLOCK), 0, stream, J);
    if (J.n_xagg && (istat || fstat || metrics)) LAUNCH(k_dense_overlay, dim3((unsigned)((J.n_xagg + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, stream, J);
    return brcside::done(h, stream, J);
}

}  // extern "C"
