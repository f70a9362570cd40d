// sim_codec.h — what the CPU builds of the two codec libraries share (sim_inflate, sim_deflate): the handle behind their C-ABIs, its
// lifecycle, the guard of one call and the host threads the members are spread over, under the names of
// bam_readcount_amd/csrc/brc_codec_hip.h, so that the two entry points of a library read alike.  Here every buffer is the caller's,
// host_alloc is malloc, and the times are the wall clock.  The codes are those of the codec's public header: include it first.
// All of it static or inline: nothing of it is exported.  Test infrastructure only.
#pragma once
#include <stdlib.h>

#include <atomic>
#include <chrono>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#ifndef BRC_OK
#error "sim_codec.h: include the codec's public header (BRC_OK .. BRC_E_NOMEM) first"
#endif

namespace brccodec {

struct Handle {
    std::mutex mu;
    std::string err;
    double kernel_s = 0, call_s = 0; uint64_t bytes_in = 0, bytes_out = 0;
};

static inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

template <class H> static int create(int device, H** out) {
    if (!out || device < 0) return BRC_E_ARG;
    *out = new (std::nothrow) H();
    return *out ? BRC_OK : BRC_E_NOMEM;
}
template <class H> static void destroy(H* h) { delete h; }
static inline const char* last_error(const Handle* h) { return h ? h->err.c_str() : ""; }

static inline void last_timing(const Handle* h, double* kernel_s, double* call_s, uint64_t* bytes_in, uint64_t* bytes_out) {
    if (!h) return;
    if (kernel_s) *kernel_s = h->kernel_s;
    if (call_s) *call_s = h->call_s;
    if (bytes_in) *bytes_in = h->bytes_in;
    if (bytes_out) *bytes_out = h->bytes_out;
}

static inline void* host_alloc(size_t bytes) { return malloc(bytes ? bytes : 1); }
static inline void host_free(void* p) { free(p); }

// --- one call.  The guard: the handle is this caller's until the call returns, its clock starts and what the last call left goes.
struct Call {
    std::lock_guard<std::mutex> lock;
    Handle* const h;
    const double t0;
    explicit Call(Handle* h_) : lock(h_->mu), h(h_), t0(now_s()) { h->err.clear(); h->kernel_s = 0; h->call_s = 0; h->bytes_in = 0; h->bytes_out = 0; }
    // a call that found nothing to do
    int early(int rc) { h->call_s = now_s() - t0; return rc; }
    // k0: when what stands for the kernels began
    int done(double k0, uint64_t bytes_in, uint64_t bytes_out) {
        h->kernel_s = now_s() - k0; h->bytes_in = bytes_in; h->bytes_out = bytes_out; h->call_s = now_s() - t0;
        return BRC_OK;
    }
};

// fn(shared, i) for every member i of [0, n), spread over at most 16 host threads (one below serial_below members); every thread has
// one Shared of its own on the heap, as every workgroup has one in LDS
template <class Shared, class Fn> static void for_members(size_t n, size_t serial_below, Fn fn) {
    unsigned nthr = std::thread::hardware_concurrency(); if (nthr > 16) nthr = 16; if (nthr < 1) nthr = 1;
    if (n < serial_below) nthr = 1;
    std::atomic<size_t> next(0);
    auto work = [&]() {
        std::unique_ptr<Shared> sh(new Shared());
        for (;;) {
            const size_t i = next.fetch_add(1);
            if (i >= n) break;
            fn(*sh, i);
        }
    };
    std::vector<std::thread> th;
    for (unsigned k = 1; k < nthr; ++k) th.emplace_back(work);
    work();
    for (std::thread& t : th) t.join();
}

}  // namespace brccodec
