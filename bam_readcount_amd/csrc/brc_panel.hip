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

#include <new>
#include <string>

#include "brc_panel_core.h"

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

struct brc_panel {
    int device = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    uint64_t bytes_read = 0, bytes_written = 0;
    std::string err;
};

#define HIPOK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { h->err = std::string(#call) + ": " + hipGetErrorString(e_); return BRC_E_HIP; } } while (0)

extern "C" {

const char* brc_panel_kind(void) { return "hip-gfx950"; }

void brc_panel_destroy(brc_panel* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    delete h;
}

int brc_panel_create(int device, brc_panel** out) {
    if (!out) return BRC_E_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) { (void)hipGetLastError(); return BRC_E_NODEVICE; }
    brc_panel* h = new (std::nothrow) brc_panel();
    if (!h) return BRC_E_NOMEM;
    h->device = device;
    hipFuncAttributes fa;
    if (hipSetDevice(device) != hipSuccess || hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess ||
        hipFuncGetAttributes(&fa, (const void*)k_panel_planes) != hipSuccess) {
        (void)hipGetLastError(); brc_panel_destroy(h); return BRC_E_NODEVICE;     // (no kernel for this device either: nothing falls back)
    }
    *out = h;
    return BRC_OK;
}

const char* brc_panel_last_error(const brc_panel* h) { return h ? h->err.c_str() : ""; }

int brc_panel_gather(brc_panel* h, const brc_device_view* v, const int32_t* idx, int64_t n, int64_t dst_stride, uint32_t* ncol, uint32_t* depth,
                     uint32_t* unavail, uint32_t* istat, float* fstat, float* metrics, uint32_t* status, void* stream_) {
    if (!h) return BRC_E_ARG;
    h->err.clear(); h->timed = false; h->bytes_read = h->bytes_written = 0;
    const char* why = "";
    if (check_job(v, idx, n, dst_stride, &why)) { h->err = why; return BRC_E_ARG; }
    if (v->memory != BRC_MEM_DEVICE) { h->err = "the view does not lie in device memory"; return BRC_E_ARG; }
    if (v->device != h->device) { h->err = "the view lies on another device"; return BRC_E_ARG; }
    const bool dests = ncol || depth || unavail || istat || fstat || metrics;
    if (!status && (n == 0 || !dests)) return BRC_OK;
    hipStream_t stream = (hipStream_t)stream_;
    HIPOK(hipSetDevice(h->device));
    if (status) HIPOK(hipMemsetAsync(status, 0, sizeof(uint32_t), stream));
    if (n == 0) return BRC_OK;
    const Job J = make_job(v, idx, n, dst_stride, ncol, depth, unavail, istat, fstat, metrics, status);
    HIPOK(hipEventRecord(h->ev0, stream));
    // (a call that wants the verdict alone needs library 0's lanes only)
    hipLaunchKernelGGL(k_panel_planes, dim3((unsigned)((n + BLOCK - 1) / BLOCK), dests ? (unsigned)v->n_lib : 1u), dim3(BLOCK), 0, stream, J);
    HIPOK(hipGetLastError());
    if (J.n_xagg && wants_buckets(J)) {
        hipLaunchKernelGGL(k_panel_overlay, dim3((unsigned)((J.n_xagg + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, stream, J);
        HIPOK(hipGetLastError());
    }
    HIPOK(hipEventRecord(h->ev1, stream));
    h->timed = true;
    job_bytes(J, &h->bytes_read, &h->bytes_written);
    return BRC_OK;
}

void brc_panel_last_timing(const brc_panel* h, double* kernel_s, uint64_t* bytes_read, uint64_t* bytes_written) {
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
