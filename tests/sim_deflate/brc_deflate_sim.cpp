// CPU build of the deflater's C-ABI (include/brc_deflate.h) over brc_deflate_core.h: the test counterpart of libbrc_deflate_hip.so,
// as libbrc_inflate_sim.so is the inflater's.  Every member is compressed by deflate_member() — the function the gfx950 kernel
// runs — with the 256 lanes of each parallel phase executed one after the other, into a zeroed slot of its own; the members are
// spread over host threads and then packed back to back, as the device's scan and gather kernels do.  Test infrastructure only.
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <chrono>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../bam_readcount_amd/csrc/brc_deflate_core.h"
#include "../../include/brc_deflate.h"

using namespace brcdef;

struct brc_deflater {
    std::mutex mu;
    std::string err;
    double kernel_s = 0, call_s = 0; uint64_t bytes_in = 0, bytes_out = 0;
};

static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

extern "C" {

const char* brc_deflater_kind(void) { return "sim"; }

int brc_deflater_create(int device, brc_deflater** out) {
    if (!out || device < 0) return BRC_E_ARG;
    *out = new (std::nothrow) brc_deflater();
    return *out ? BRC_OK : BRC_E_NOMEM;
}
void brc_deflater_destroy(brc_deflater* h) { delete h; }
const char* brc_deflater_last_error(const brc_deflater* h) { return h ? h->err.c_str() : ""; }
size_t brc_deflate_bound(size_t src_len) { return bound(src_len); }
const uint8_t* brc_deflate_eof_block(size_t* len) { if (len) *len = EOF_LEN; return eof_member(); }
void* brc_deflate_host_alloc(size_t bytes) { return malloc(bytes ? bytes : 1); }
void brc_deflate_host_free(void* p) { free(p); }

void brc_deflater_last_timing(const brc_deflater* h, double* kernel_s, double* call_s, uint64_t* bytes_in, uint64_t* bytes_out) {
    if (!h) return;
    if (kernel_s) *kernel_s = h->kernel_s;
    if (call_s) *call_s = h->call_s;
    if (bytes_in) *bytes_in = h->bytes_in;
    if (bytes_out) *bytes_out = h->bytes_out;
}

int brc_deflate_bgzf(brc_deflater* h, const void* src_, size_t src_len, void* dst_, size_t dst_cap, size_t* dst_len, size_t* n_members_out) {
    if (!h || !dst_len || !n_members_out || (!src_ && src_len) || (!dst_ && src_len) || dst_cap < bound(src_len)) return BRC_E_ARG;
    std::lock_guard<std::mutex> guard(h->mu);
    const double t0 = now_s();
    h->err.clear(); h->kernel_s = 0; h->call_s = 0; h->bytes_in = 0; h->bytes_out = 0;
    *dst_len = 0; *n_members_out = 0;
    const size_t n = n_members(src_len);
    if (n == 0) { h->call_s = now_s() - t0; return BRC_OK; }
    const uint8_t* src = (const uint8_t*)src_; uint8_t* dst = (uint8_t*)dst_;
    std::vector<uint32_t> slots(n * (size_t)SLOT_WORDS, 0u), sizes(n);
    unsigned nthr = std::thread::hardware_concurrency(); if (nthr > 16) nthr = 16; if (nthr < 1) nthr = 1;
    if (n < 4) nthr = 1;
    std::atomic<size_t> next(0);
    auto work = [&]() {
        std::unique_ptr<Shared> sh(new Shared());
        for (;;) {
            const size_t i = next.fetch_add(1);
            if (i >= n) break;
            const size_t off = i * (size_t)MEMBER_IN;
            // (the member's input as an exact sub-range: a sanitizer build sees every read outside it)
            sizes[i] = deflate_member(*sh, src + off, (uint32_t)(src_len - off < MEMBER_IN ? src_len - off : MEMBER_IN), slots.data() + i * (size_t)SLOT_WORDS);
        }
    };
    std::vector<std::thread> th;
    for (unsigned k = 1; k < nthr; ++k) th.emplace_back(work);
    work();
    for (std::thread& t : th) t.join();
    size_t total = 0;
    for (size_t i = 0; i < n; ++i) {
        if (sizes[i] > SLOT || total + sizes[i] > dst_cap) { h->err = "a member outgrew its bound"; return BRC_E_HIP; }
        memcpy(dst + total, slots.data() + i * (size_t)SLOT_WORDS, sizes[i]); total += sizes[i];
    }
    *dst_len = total; *n_members_out = n;
    h->kernel_s = now_s() - t0; h->bytes_in = src_len; h->bytes_out = total; h->call_s = now_s() - t0;
    return BRC_OK;
}

}  // extern "C"
