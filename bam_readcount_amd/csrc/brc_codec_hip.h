// brc_codec_hip.h — the host side the two gfx950 codec libraries share (brc_inflate.hip, brc_deflate.hip): the handle behind their
// C-ABIs with its own stream, events and page-locked staging, its lifecycle, the buffers that only ever grow, and the pieces of one
// call around what is the library's own.  A codec library supplies its kernels, `struct brc_X : brccodec::Handle { its buffers }`,
// one-line forwards and ONE entry point that reads
//   Call | its plan, call.early | hipSetDevice | grow | upload | ev0 | launches | ev1 | sync | landing | copy back | sync | call.done
// Host code only, all of it static or inline: nothing of it is exported, and nothing of the engine or of the side libraries is
// included.  The codec headers stand alone, so the codes are theirs: include include/brc_inflate.h or include/brc_deflate.h first.
// tests/sim_codec.h is the same under the same names for the CPU builds.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <mutex>
#include <new>
#include <string>

#include <string.h>

#ifndef BRC_OK
#error "brc_codec_hip.h: include the codec's public header (BRC_OK .. BRC_E_NOMEM) first"
#endif

namespace brccodec {

struct Handle;

// In a function that has the handle as `h` and returns a code: a failed runtime call leaves its text in the handle and ends the function.
#define HIPOK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { h->err = std::string(#call) + ": " + hipGetErrorString(e_); return BRC_E_HIP; } } while (0)
// One launch and the runtime's verdict on it.
#define LAUNCH(kernel, grid, block, lds, stream, ...) do { hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__); HIPOK(hipGetLastError()); } while (0)

// Pointer plus capacity (in elements) of memory the handle owns, on the device or page-locked on the host.  It is reallocated only
// when a call wants more than there is, then with a quarter and a page to spare, and freed BEFORE the larger one is asked for.
enum Where { DEVICE, PINNED };
template <class T, Where W> struct Buf {
    T* p = nullptr;
    size_t cap = 0;
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    ~Buf() { release(); }
    inline int grow(Handle* h, size_t want);
    void release() { if (p) (void)(W == DEVICE ? hipFree(p) : hipHostFree(p)); p = nullptr; cap = 0; }
};
template <class T> using DevBuf = Buf<T, DEVICE>;
using PinnedBuf = Buf<uint8_t, PINNED>;

struct Handle {
    int device = 0;
    hipStream_t stream = nullptr;                 // its own, non-blocking: every copy and launch of a call
    hipEvent_t ev0 = nullptr, ev1 = nullptr;      // around the launches of the last call
    PinnedBuf h_src, h_dst;                       // staging for callers' pageable memory
    std::mutex mu;
    std::string err;
    double kernel_s = 0, call_s = 0; uint64_t bytes_in = 0, bytes_out = 0;
    // (behind the members of the library's struct, which are its device buffers; destroy() has made the device current and waited)
    ~Handle() {
        h_src.release(); h_dst.release();
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

template <class T, Where W> inline int Buf<T, W>::grow(Handle* h, size_t want) {
    if (want <= cap) return BRC_OK;
    if (p) { HIPOK(W == DEVICE ? hipFree(p) : hipHostFree(p)); p = nullptr; cap = 0; }
    const size_t n = want + want / 4 + 4096;
    if ((W == DEVICE ? hipMalloc((void**)&p, n * sizeof(T)) : hipHostMalloc((void**)&p, n * sizeof(T), hipHostMallocPortable)) != hipSuccess) {
        (void)hipGetLastError(); p = nullptr; h->err = W == DEVICE ? "out of device memory" : "out of page-locked memory"; return BRC_E_NOMEM;
    }
    cap = n;
    return BRC_OK;
}

static inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// page-locked memory (the library's own host_alloc or anyone's hipHostMalloc / hipHostRegister) is copied from and to as it lies
static inline bool is_pinned(const void* p) {
    hipPointerAttribute_t a; memset(&a, 0, sizeof a);
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost;
}

template <class H> static void destroy(H* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    delete h;       // the library's buffers, then ~Handle: staging, events, stream
}

// kernel: the one that needs lds_bytes of dynamic LDS; a device its code object has no code for gets no handle (nothing falls back)
template <class H> static int create(int device, const void* kernel, size_t lds_bytes, H** out) {
    if (!out) return BRC_E_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) { (void)hipGetLastError(); return BRC_E_NODEVICE; }
    H* h = new (std::nothrow) H();
    if (!h) return BRC_E_NOMEM;
    h->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess ||
        hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess) {
        (void)hipGetLastError(); destroy(h); return BRC_E_NODEVICE;
    }
    *out = h;
    return BRC_OK;
}

static inline const char* last_error(const Handle* h) { return h ? h->err.c_str() : ""; }

static inline void last_timing(const Handle* h, double* kernel_s, double* call_s, uint64_t* bytes_in, uint64_t* bytes_out) {
    if (!h) return;
    if (kernel_s) *kernel_s = h->kernel_s;
    if (call_s) *call_s = h->call_s;
    if (bytes_in) *bytes_in = h->bytes_in;
    if (bytes_out) *bytes_out = h->bytes_out;
}

static inline void* host_alloc(size_t bytes) { void* p = nullptr; if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); return nullptr; } return p; }
static inline void host_free(void* p) { if (p) (void)hipHostFree(p); }

// --- one call.  The guard: the handle is this caller's until the call returns, its clock starts and what the last call left goes.
// A call that ends on a refusal or a runtime error leaves the four figures at 0.
struct Call {
    std::lock_guard<std::mutex> lock;
    Handle* const h;
    const double t0;
    explicit Call(Handle* h_) : lock(h_->mu), h(h_), t0(now_s()) { h->err.clear(); h->kernel_s = 0; h->call_s = 0; h->bytes_in = 0; h->bytes_out = 0; }
    // a call that found nothing to launch
    int early(int rc) { h->call_s = now_s() - t0; return rc; }
    // behind the second wait: the kernel time between the events and the call's traffic
    int done(uint64_t bytes_in, uint64_t bytes_out) {
        float ms = 0; HIPOK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
        h->kernel_s = ms * 1e-3; h->bytes_in = bytes_in; h->bytes_out = bytes_out; h->call_s = now_s() - t0;
        return BRC_OK;
    }
};

// src[0, bytes) -> dev on the handle's stream: as it lies when it is page-locked, else through h_src
static inline int upload(Handle* h, void* dev, const void* src, size_t bytes) {
    if (!bytes) return BRC_OK;
    if (!is_pinned(src)) {
        if (const int g = h->h_src.grow(h, bytes)) return g;
        memcpy(h->h_src.p, src, bytes); src = h->h_src.p;
    }
    HIPOK(hipMemcpyAsync(dev, src, bytes, hipMemcpyHostToDevice, h->stream));
    return BRC_OK;
}

// where `bytes` from the device land: dst itself when it is page-locked (or nothing comes), else h_dst, which the caller copies from
static inline int landing(Handle* h, const void* dst, size_t bytes, bool* pinned) {
    *pinned = bytes == 0 || is_pinned(dst);
    return *pinned ? BRC_OK : h->h_dst.grow(h, bytes);
}

}  // namespace brccodec
