// brc_inflate.hip — device-side BGZF inflate for gfx950 behind the C-ABI of include/brc_inflate.h (libbrc_inflate_hip.so; a
// translation unit and a library of its own: the engine's libraries keep exactly the device code they had).
//
// One wave (a workgroup of 64 lanes) per BGZF member; the decoder itself is brc_inflate_core.h, shared with the CPU build the
// tests run.  LDS per workgroup: sizeof(brcinf::Shared) = 64 KB output window + 5.6 KB of tables and lists, two workgroups per CU
// (160 KB), 512 members in flight on 256 CUs.  DESIGN.md 6a has the reasoning and the measurements.
#include <hip/hip_runtime.h>

#include <chrono>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include <string.h>

#include "brc_inflate_plan.h"

using namespace brcinf;

static_assert(sizeof(Shared) <= 80 * 1024, "two workgroups must fit the 160 KB of LDS of a CU");
static_assert(sizeof(Member) == 32, "Member layout");

__global__ __launch_bounds__(LANES) void k_inflate_bgzf(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const Member* __restrict__ members,
                                                          uint8_t* __restrict__ status, uint32_t n) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    Shared& sh = *reinterpret_cast<Shared*>(lds_raw);
    const uint32_t i = blockIdx.x;
    if (i >= n) return;
    const Member m = members[i];
    // (the host has checked src_off + clen <= src_len and dst_off + isize <= dst_cap for every member it lists)
    const int st = m.pre_status ? (int)m.pre_status : inflate_member(sh, src + m.src_off, m.clen, dst + m.dst_off, m.isize, m.crc);
    if (threadIdx.x == 0) status[i] = (uint8_t)st;
}

struct brc_inflater {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    uint8_t *d_src = nullptr, *d_dst = nullptr, *d_status = nullptr; Member* d_members = nullptr;
    size_t cap_src = 0, cap_dst = 0, cap_status = 0, cap_members = 0;
    uint8_t *h_src = nullptr, *h_dst = nullptr; size_t hcap_src = 0, hcap_dst = 0;     // page-locked staging for callers' pageable memory
    std::vector<Member> members;
    std::vector<uint8_t> st;
    std::mutex mu;
    std::string err;
    double kernel_s = 0, call_s = 0; uint64_t bytes_in = 0, bytes_out = 0;
};

static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
#define HIPOK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { h->err = std::string(#call) + ": " + hipGetErrorString(e_); return BRC_E_HIP; } } while (0)

template <class T> static int grow_dev(brc_inflater* h, T** p, size_t* cap, size_t want) {
    if (want <= *cap) return BRC_OK;
    if (*p) { HIPOK(hipFree(*p)); *p = nullptr; *cap = 0; }
    const size_t n = want + want / 4 + 4096;
    if (hipMalloc((void**)p, n * sizeof(T)) != hipSuccess) { (void)hipGetLastError(); *p = nullptr; h->err = "out of device memory"; return BRC_E_NOMEM; }
    *cap = n;
    return BRC_OK;
}
static int grow_host(brc_inflater* h, uint8_t** p, size_t* cap, size_t want) {
    if (want <= *cap) return BRC_OK;
    if (*p) { HIPOK(hipHostFree(*p)); *p = nullptr; *cap = 0; }
    const size_t n = want + want / 4 + 4096;
    if (hipHostMalloc((void**)p, n, hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); *p = nullptr; h->err = "out of page-locked memory"; return BRC_E_NOMEM; }
    *cap = n;
    return BRC_OK;
}
static bool is_pinned(const void* p) {
    hipPointerAttribute_t a; memset(&a, 0, sizeof a);
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost;
}

extern "C" {

const char* brc_inflater_kind(void) { return "hip-gfx950"; }

void brc_inflater_destroy(brc_inflater* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->d_src) (void)hipFree(h->d_src);
    if (h->d_dst) (void)hipFree(h->d_dst);
    if (h->d_status) (void)hipFree(h->d_status);
    if (h->d_members) (void)hipFree(h->d_members);
    if (h->h_src) (void)hipHostFree(h->h_src);
    if (h->h_dst) (void)hipHostFree(h->h_dst);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int brc_inflater_create(int device, brc_inflater** out) {
    if (!out) return BRC_E_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) { (void)hipGetLastError(); return BRC_E_NODEVICE; }
    brc_inflater* h = new (std::nothrow) brc_inflater();
    if (!h) return BRC_E_NOMEM;
    h->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess ||
        hipFuncSetAttribute((const void*)k_inflate_bgzf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(Shared)) != hipSuccess) {
        (void)hipGetLastError(); brc_inflater_destroy(h); return BRC_E_NODEVICE;     // (no kernel for this device either: nothing falls back)
    }
    *out = h;
    return BRC_OK;
}

const char* brc_inflater_last_error(const brc_inflater* h) { return h ? h->err.c_str() : ""; }

void* brc_inflate_host_alloc(size_t bytes) { void* p = nullptr; if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); return nullptr; } return p; }
void brc_inflate_host_free(void* p) { if (p) (void)hipHostFree(p); }

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
    if (n > 0x7fffffffu) return BRC_E_ARG;
    // (plan_chain: every listed member lies inside src[0, src_len) and its slot inside dst[0, dst_cap))
    const size_t used = (size_t)(h->members[n - 1].src_off + h->members[n - 1].clen), out_bytes = (size_t)dst_off[n];
    HIPOK(hipSetDevice(h->device));
    int g;
    if ((g = grow_dev(h, &h->d_src, &h->cap_src, used + 16)) || (g = grow_dev(h, &h->d_dst, &h->cap_dst, out_bytes + 16)) ||
        (g = grow_dev(h, &h->d_status, &h->cap_status, n)) || (g = grow_dev(h, &h->d_members, &h->cap_members, n))) return g;
    const uint8_t* up = src;
    if (used && !is_pinned(src)) { if ((g = grow_host(h, &h->h_src, &h->hcap_src, used))) return g; memcpy(h->h_src, src, used); up = h->h_src; }
    uint8_t* down = dst;
    const bool dst_pinned = out_bytes == 0 || is_pinned(dst);
    if (!dst_pinned) { if ((g = grow_host(h, &h->h_dst, &h->hcap_dst, out_bytes))) return g; down = h->h_dst; }
    if (used) HIPOK(hipMemcpyAsync(h->d_src, up, used, hipMemcpyHostToDevice, h->stream));
    HIPOK(hipMemcpyAsync(h->d_members, h->members.data(), n * sizeof(Member), hipMemcpyHostToDevice, h->stream));
    HIPOK(hipEventRecord(h->ev0, h->stream));
    hipLaunchKernelGGL(k_inflate_bgzf, dim3((unsigned)n), dim3(LANES), sizeof(Shared), h->stream, h->d_src, h->d_dst, h->d_members, h->d_status, (uint32_t)n);
    HIPOK(hipGetLastError());
    HIPOK(hipEventRecord(h->ev1, h->stream));
    h->st.resize(n);
    HIPOK(hipMemcpyAsync(h->st.data(), h->d_status, n, hipMemcpyDeviceToHost, h->stream));
    // the slots of the members that came out right travel back: one copy per run of them (one copy in all when none failed); a
    // member that failed leaves its slot as the caller had it
    // (the statuses decide which bytes to fetch, so they are waited for first)
    HIPOK(hipStreamSynchronize(h->stream));
    bool all_ok = true;
    for (size_t i = 0; i < n; ++i) all_ok &= h->st[i] == ST_OK;
    for (size_t i = 0; i < n;) {
        if (h->st[i] != ST_OK) { ++i; continue; }
        size_t j = i; while (j < n && h->st[j] == ST_OK) ++j;
        const size_t a = (size_t)dst_off[i], b = (size_t)dst_off[j];
        if (b > a) HIPOK(hipMemcpyAsync(down + a, h->d_dst + a, b - a, hipMemcpyDeviceToHost, h->stream));
        i = j;
    }
    HIPOK(hipStreamSynchronize(h->stream));
    if (!dst_pinned) {
        if (all_ok) memcpy(dst, h->h_dst, out_bytes);
        else for (size_t i = 0; i < n; ++i) if (h->st[i] == ST_OK) memcpy(dst + dst_off[i], h->h_dst + dst_off[i], (size_t)(dst_off[i + 1] - dst_off[i]));
    }
    memcpy(status, h->st.data(), n);
    float ms = 0; HIPOK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    h->kernel_s = ms * 1e-3; h->bytes_in = used; h->bytes_out = out_bytes; h->call_s = now_s() - t0;
    return rc;
}

}  // extern "C"
