// CPU build of the inflater's C-ABI (include/brc_inflate.h) over brc_inflate_core.h: the test counterpart of libbrc_inflate_hip.so,
// as libbrc_sim.so is the engine's.  Every member is decoded by inflate_member() — the function the gfx950 kernel runs — with the 64
// lanes of each parallel phase executed one after the other; members are spread over host threads.  Test infrastructure only.
#include <string.h>

#include <atomic>
#include <chrono>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../bam_readcount_amd/csrc/brc_inflate_plan.h"

using namespace brcinf;

struct brc_inflater {
    std::vector<Member> members;
    std::mutex mu;
    std::string err;
    double kernel_s = 0, call_s = 0; uint64_t bytes_in = 0, bytes_out = 0;
};

static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

extern "C" {

const char* brc_inflater_kind(void) { return "sim"; }

int brc_inflater_create(int device, brc_inflater** out) {
    if (!out || device < 0) return BRC_E_ARG;
    *out = new (std::nothrow) brc_inflater();
    return *out ? BRC_OK : BRC_E_NOMEM;
}
void brc_inflater_destroy(brc_inflater* h) { delete h; }
const char* brc_inflater_last_error(const brc_inflater* h) { return h ? h->err.c_str() : ""; }
void* brc_inflate_host_alloc(size_t bytes) { return malloc(bytes ? bytes : 1); }
void brc_inflate_host_free(void* p) { free(p); }

void brc_inflater_last_timing(const brc_inflater* h, double* kernel_s, double* call_s, uint64_t* bytes_in, uint64_t* bytes_out) {
    if (!h) return;
    if (kernel_s) *kernel_s = h->kernel_s;
    if (call_s) *call_s = h->call_s;
    if (bytes_in) *bytes_in = h->bytes_in;
    if (bytes_out) *bytes_out = h->bytes_out;
}

int brc_inflate_bgzf(brc_inflater* h, const void* src_, size_t src_len, void* dst_, size_t dst_cap, uint64_t* dst_off, uint8_t* status, size_t* n_members) {
    if (!h || !n_members || !dst_off || (!src_ && src_len) || (!dst_ && dst_cap) || (!status && *n_members)) return BRC_E_ARG;
    std::lock_guard<std::mutex> guard(h->mu);
    const double t0 = now_s();
    h->err.clear(); h->kernel_s = 0; h->call_s = 0; h->bytes_in = 0; h->bytes_out = 0;
    const uint8_t* src = (const uint8_t*)src_; uint8_t* dst = (uint8_t*)dst_;
    bool run = false;
    const int rc = plan_chain(src, src_len, dst_cap, *n_members, h->members, dst_off, status, n_members, &run);
    const size_t n = h->members.size();
    if (!run || n == 0) { h->call_s = now_s() - t0; return rc; }
    const double k0 = now_s();
    unsigned nthr = std::thread::hardware_concurrency(); if (nthr > 16) nthr = 16; if (nthr < 1) nthr = 1;
    if (n < 8) nthr = 1;
    std::atomic<size_t> next(0);
    auto work = [&]() {
        std::unique_ptr<Shared> sh(new Shared());
        for (;;) {
            const size_t i = next.fetch_add(1);
            if (i >= n) break;
            const Member& m = h->members[i];
            // (the member's payload and slot as exact sub-ranges: a sanitizer build sees every step outside them)
            status[i] = (uint8_t)(m.pre_status ? (int)m.pre_status : inflate_member(*sh, src + m.src_off, m.clen, dst + m.dst_off, m.isize, m.crc));
        }
    };
    std::vector<std::thread> th;
    for (unsigned k = 1; k < nthr; ++k) th.emplace_back(work);
    work();
    for (std::thread& t : th) t.join();
    h->kernel_s = now_s() - k0; h->bytes_in = src_len; h->bytes_out = dst_off[n]; h->call_s = now_s() - t0;
    return rc;
}

}  // extern "C"
