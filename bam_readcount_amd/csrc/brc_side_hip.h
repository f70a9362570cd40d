// brc_side_hip.h — the host side every gfx950 side library shares (brc_dense.hip, brc_indels.hip, brc_panel.hip, brc_select.hip,
// brc_bins.hip): the handle behind their C-ABIs, its lifecycle, the checks in front of a call's launches and the bookkeeping behind
// them.  A side library supplies its kernels, `struct brc_X : brcside::Handle {}`, five one-line forwards and ONE entry point that reads
//   clear | check_job, refuse | resident | hipSetDevice | job | start | launches | done
// Host code only, all of it static: nothing of it is exported, and nothing of the engine is included.  tests/sim_side.h is the same
// under the same names for the CPU builds, so that the two entry points of a library read alike.
#pragma once
#include <hip/hip_runtime.h>

#include <new>
#include <string>

#include "../../include/brc.h"

namespace brcside {

struct Handle {
    int device = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;      // around the launches of the last call
    bool timed = false;
    uint64_t bytes_read = 0, bytes_written = 0;
    std::string err;
};

// In a function that has the handle as `h` and returns a code: a failed runtime call leaves its text in the handle and ends the function.
#define HIPOK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { h->err = std::string(#call) + ": " + hipGetErrorString(e_); return BRC_E_HIP; } } while (0)
// One launch and the runtime's verdict on it.
#define LAUNCH(kernel, grid, block, lds, stream, ...) do { hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__); HIPOK(hipGetLastError()); } while (0)

template <class H> static void destroy(H* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    delete h;
}

// probe_kernel: one kernel of the library; a device its code object has no code for gets no handle (nothing falls back)
template <class H> static int create(int device, const void* probe_kernel, H** out) {
    if (!out) return BRC_E_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) { (void)hipGetLastError(); return BRC_E_NODEVICE; }
    H* h = new (std::nothrow) H();
    if (!h) return BRC_E_NOMEM;
    h->device = device;
    hipFuncAttributes fa;
    if (hipSetDevice(device) != hipSuccess || hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess ||
        hipFuncGetAttributes(&fa, probe_kernel) != hipSuccess) {
        (void)hipGetLastError(); destroy(h); return BRC_E_NODEVICE;
    }
    *out = h;
    return BRC_OK;
}

static inline const char* last_error(const Handle* h) { return h ? h->err.c_str() : ""; }

static inline void last_timing(const Handle* h, double* kernel_s, uint64_t* bytes_read, uint64_t* bytes_written) {
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

// --- one call: what the last one left goes first
static inline void clear(Handle* h) { h->err.clear(); h->timed = false; h->bytes_read = h->bytes_written = 0; }

static inline int refuse(Handle* h, const char* why) { h->err = why; return BRC_E_ARG; }

// a library speaks of "the view" or, where a call takes two that check_job has tied to each other, of "the views"
enum Views { ONE_VIEW, TWO_VIEWS };
template <class View> static int resident(Handle* h, const View* v, Views views) {
    if (v->memory != BRC_MEM_DEVICE) return refuse(h, views == ONE_VIEW ? "the view does not lie in device memory" : "the views do not lie in device memory");
    if (v->device != h->device) return refuse(h, views == ONE_VIEW ? "the view lies on another device" : "the views lie on another device");
    return BRC_OK;
}

// in front of the first launch that counts / behind the last: the events of last_timing and the job's traffic (job_bytes of its core)
static inline int start(Handle* h, hipStream_t stream) {
    HIPOK(hipEventRecord(h->ev0, stream));
    return BRC_OK;
}
template <class Job> static int done(Handle* h, hipStream_t stream, const Job& J) {
    HIPOK(hipEventRecord(h->ev1, stream));
    h->timed = true;
    job_bytes(J, &h->bytes_read, &h->bytes_written);
    return BRC_OK;
}

}  // namespace brcside
