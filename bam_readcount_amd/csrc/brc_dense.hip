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

#include <new>
#include <string>

#include "brc_dense_core.h"

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

struct brc_dense {
    int device = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    uint64_t bytes_read = 0, bytes_written = 0;
    std::string err;
};

#define HIPOK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { h->err = std::string(#call) + ": " + hipGetErrorString(e_); return BRC_E_HIP; } } while (0)

extern "C" {

const char* brc_dense_kind(void) { return "hip-gfx950"; }

void brc_dense_destroy(brc_dense* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    delete h;
}

int brc_dense_create(int device, brc_dense** out) {
    if (!out) return BRC_E_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) { (void)hipGetLastError(); return BRC_E_NODEVICE; }
    brc_dense* h = new (std::nothrow) brc_dense();
    if (!h) return BRC_E_NOMEM;
    h->device = device;
    hipFuncAttributes fa;
    if (hipSetDevice(device) != hipSuccess || hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess ||
        hipFuncGetAttributes(&fa, (const void*)k_dense_planes) != hipSuccess) {
        (void)hipGetLastError(); brc_dense_destroy(h); return BRC_E_NODEVICE;     // (no kernel for this device either: nothing falls back)
    }
    *out = h;
    return BRC_OK;
}

const char* brc_dense_last_error(const brc_dense* h) { return h ? h->err.c_str() : ""; }

int brc_dense_expand(brc_dense* h, const brc_device_view* v, int64_t k0, int64_t n, int64_t dst_stride, uint32_t* ncol, uint32_t* depth,
                     uint32_t* unavail, uint32_t* istat, float* fstat, float* metrics, void* stream_) {
    if (!h) return BRC_E_ARG;
    h->err.clear(); h->timed = false; h->bytes_read = h->bytes_written = 0;
    const char* why = "";
    if (check_job(v, k0, n, dst_stride, &why)) { h->err = why; return BRC_E_ARG; }
    if (v->memory != BRC_MEM_DEVICE) { h->err = "the view does not lie in device memory"; return BRC_E_ARG; }
    if (v->device != h->device) { h->err = "the view lies on another device"; return BRC_E_ARG; }
    if (n == 0 || (!ncol && !depth && !unavail && !istat && !fstat && !metrics)) return BRC_OK;
    if ((n + BLOCK - 1) / BLOCK > 0x7fffffffLL || v->n_lib > 65535 || (v->n_xagg + BLOCK - 1) / BLOCK > 0x7fffffffULL) { h->err = "window too large for one launch"; return BRC_E_ARG; }
    const Job J = make_job(v, k0, n, dst_stride, ncol, depth, unavail, istat, fstat, metrics);
    hipStream_t stream = (hipStream_t)stream_;
    HIPOK(hipSetDevice(h->device));
    HIPOK(hipEventRecord(h->ev0, stream));
    hipLaunchKernelGGL(k_dense_planes, dim3((unsigned)((n + BLOCK - 1) / BLOCK), (unsigned)v->n_lib), dim3(BLOCK), 0, stream, J);
    HIPOK(hipGetLastError());
    if (J.n_xagg && (istat || fstat || metrics)) {
        hipLaunchKernelGGL(k_dense_overlay, dim3((unsigned)((J.n_xagg + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, stream, J);
        HIPOK(hipGetLastError());
    }
    HIPOK(hipEventRecord(h->ev1, stream));
    h->timed = true;
    job_bytes(J, &h->bytes_read, &h->bytes_written);
    return BRC_OK;
}

void brc_dense_last_timing(const brc_dense* h, double* kernel_s, uint64_t* bytes_read, uint64_t* bytes_written) {
    if (!h) return;
    double s = 0;
    if (h->timed && kernel_s) {
        float ms = 0;
        if (hipEventSynchronize(h->ev1) == hipSuccess && hipEventElapsedTime(&ms, h->ev0, h->ev1) == hipSuccess) s = ms * 1e-3; else (void)hipGetLastError();
    }
    if (kernel_s) *kernel_s = s;
    if (bytes_read) *bytes_read = h->bytes_read;
    if (bytes_written) *bytes_written = h->bytes_written;
}

}  // extern "C"
