// brc_deflate.hip — device-side BGZF compression for gfx950 behind the C-ABI of include/brc_deflate.h (libbrc_deflate_hip.so; a
// translation unit and a library of its own: the engine's and the inflater's libraries keep exactly the device code they had).
//
// One workgroup of 256 lanes per member; the compressor itself is brc_deflate_core.h, shared with the CPU build the tests run.
// LDS per workgroup: sizeof(brcdef::Shared) = 156 660 bytes (the static_assert below; 64 KB input window + 64 KB match / token
// array + 16 KB head table + tables), one workgroup per CU (160 KB), 256 members in flight.  Every member is written into a slot of its own (zeroed first: the bits are
// ORed in); k_scan_sizes turns the member sizes into offsets and k_gather packs the members back to back, so only compressed bytes
// cross PCIe.  DESIGN.md 6b has the reasoning and the measurements.
#include <hip/hip_runtime.h>

#include <chrono>
#include <mutex>
#include <new>
#include <string>

#include <string.h>

#include "brc_deflate_core.h"
#include "../../include/brc_deflate.h"

using namespace brcdef;

static_assert(sizeof(Shared) == 156660 && sizeof(Shared) <= 160 * 1024, "one workgroup must fit the 160 KB of LDS of a CU (the figure the comments and DESIGN.md 6b quote)");
static_assert(SLOT % 16 == 0 && MEMBER_IN % 16 == 0, "members and slots start on 16-byte boundaries");

__global__ __launch_bounds__(LANES) void k_deflate_bgzf(const uint8_t* __restrict__ src, uint64_t src_len, uint8_t* __restrict__ slots, uint32_t* __restrict__ sizes, uint32_t n) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    Shared& sh = *reinterpret_cast<Shared*>(lds_raw);
    const uint32_t i = blockIdx.x;
    if (i >= n) return;
    const uint64_t off = (uint64_t)i * MEMBER_IN;
    const uint32_t len = (uint32_t)(src_len - off < MEMBER_IN ? src_len - off : MEMBER_IN);        // (the host launches ceil(src_len / MEMBER_IN) workgroups: off < src_len)
    const uint32_t total = deflate_member(sh, src + off, len, (uint32_t*)(slots + (uint64_t)i * SLOT));
    if (threadIdx.x == 0) sizes[i] = total;
}

// offs[0 .. n]: exclusive prefix sum of sizes[0 .. n).  One workgroup: a share of the members per lane, lane 0 scans the 256 sums.
__global__ __launch_bounds__(LANES) void k_scan_sizes(const uint32_t* __restrict__ sizes, uint64_t* __restrict__ offs, uint32_t n) {
    __shared__ uint64_t sum[LANES];
    const uint32_t per = (n + LANES - 1) / LANES, a = threadIdx.x * per < n ? threadIdx.x * per : n, b = a + per < n ? a + per : n;
    uint64_t s = 0;
    for (uint32_t i = a; i < b; ++i) s += sizes[i];
    sum[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) { uint64_t run = 0; for (int l = 0; l < LANES; ++l) { const uint64_t v = sum[l]; sum[l] = run; run += v; } offs[n] = run; }
    __syncthreads();
    uint64_t run = sum[threadIdx.x];
    for (uint32_t i = a; i < b; ++i) { offs[i] = run; run += sizes[i]; }
}

__global__ __launch_bounds__(LANES) void k_gather(const uint8_t* __restrict__ slots, const uint32_t* __restrict__ sizes, const uint64_t* __restrict__ offs, uint8_t* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x;
    if (i >= n) return;
    const uint8_t* s = slots + (uint64_t)i * SLOT;
    uint8_t* d = out + offs[i];
    const uint32_t sz = sizes[i] <= SLOT ? sizes[i] : SLOT;
    // bytes up to the first 4-byte boundary of the destination, whole words put together from the slot's bytes, the rest
    uint32_t head = (uint32_t)((4u - ((uintptr_t)d & 3u)) & 3u); if (head > sz) head = sz;
    const uint32_t nw = (sz - head) / 4u, tail0 = head + nw * 4u;
    if (threadIdx.x < head) d[threadIdx.x] = s[threadIdx.x];
    for (uint32_t w = threadIdx.x; w < nw; w += LANES) {
        const uint8_t* q = s + head + w * 4u;
        *(uint32_t*)(d + head + w * 4u) = (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24;
    }
    if (tail0 + threadIdx.x < sz) d[tail0 + threadIdx.x] = s[tail0 + threadIdx.x];
}

struct brc_deflater {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    uint8_t *d_src = nullptr, *d_slots = nullptr, *d_out = nullptr; uint32_t* d_sizes = nullptr; uint64_t* d_offs = nullptr;
    size_t cap_src = 0, cap_slots = 0, cap_out = 0, cap_sizes = 0, cap_offs = 0;
    uint8_t *h_src = nullptr, *h_dst = nullptr; size_t hcap_src = 0, hcap_dst = 0;     // page-locked staging for callers' pageable memory
    uint64_t* h_total = nullptr;                                                          // page-locked: where the scan's last word lands
    std::mutex mu;
    std::string err;
    double kernel_s = 0, call_s = 0; uint64_t bytes_in = 0, bytes_out = 0;
};

static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
#define HIPOK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { h->err = std::string(#call) + ": " + hipGetErrorString(e_); return BRC_E_HIP; } } while (0)

template <class T> static int grow_dev(brc_deflater* h, T** p, size_t* cap, size_t want) {
    if (want <= *cap) return BRC_OK;
    if (*p) { HIPOK(hipFree(*p)); *p = nullptr; *cap = 0; }
    const size_t n = want + want / 4 + 4096;
    if (hipMalloc((void**)p, n * sizeof(T)) != hipSuccess) { (void)hipGetLastError(); *p = nullptr; h->err = "out of device memory"; return BRC_E_NOMEM; }
    *cap = n;
    return BRC_OK;
}
static int grow_host(brc_deflater* h, uint8_t** p, size_t* cap, size_t want) {
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

const char* brc_deflater_kind(void) { return "hip-gfx950"; }

void brc_deflater_destroy(brc_deflater* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->d_src) (void)hipFree(h->d_src);
    if (h->d_slots) (void)hipFree(h->d_slots);
    if (h->d_out) (void)hipFree(h->d_out);
    if (h->d_sizes) (void)hipFree(h->d_sizes);
    if (h->d_offs) (void)hipFree(h->d_offs);
    if (h->h_src) (void)hipHostFree(h->h_src);
    if (h->h_dst) (void)hipHostFree(h->h_dst);
    if (h->h_total) (void)hipHostFree(h->h_total);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int brc_deflater_create(int device, brc_deflater** out) {
    if (!out) return BRC_E_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) { (void)hipGetLastError(); return BRC_E_NODEVICE; }
    brc_deflater* h = new (std::nothrow) brc_deflater();
    if (!h) return BRC_E_NOMEM;
    h->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess ||
        hipHostMalloc((void**)&h->h_total, sizeof(uint64_t), hipHostMallocPortable) != hipSuccess ||
        hipFuncSetAttribute((const void*)k_deflate_bgzf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(Shared)) != hipSuccess) {
        (void)hipGetLastError(); brc_deflater_destroy(h); return BRC_E_NODEVICE;     // (no kernel for this device either: nothing falls back)
    }
    *out = h;
    return BRC_OK;
}

const char* brc_deflater_last_error(const brc_deflater* h) { return h ? h->err.c_str() : ""; }

size_t brc_deflate_bound(size_t src_len) { return bound(src_len); }
const uint8_t* brc_deflate_eof_block(size_t* len) { if (len) *len = EOF_LEN; return eof_member(); }

void* brc_deflate_host_alloc(size_t bytes) { void* p = nullptr; if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); return nullptr; } return p; }
void brc_deflate_host_free(void* p) { if (p) (void)hipHostFree(p); }

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
    if (n > 0x7fffffffu) return BRC_E_ARG;
    const uint8_t* src = (const uint8_t*)src_; uint8_t* dst = (uint8_t*)dst_;
    HIPOK(hipSetDevice(h->device));
    int g;
    if ((g = grow_dev(h, &h->d_src, &h->cap_src, src_len + 16)) || (g = grow_dev(h, &h->d_slots, &h->cap_slots, n * (size_t)SLOT)) ||
        (g = grow_dev(h, &h->d_out, &h->cap_out, n * (size_t)SLOT)) || (g = grow_dev(h, &h->d_sizes, &h->cap_sizes, n)) || (g = grow_dev(h, &h->d_offs, &h->cap_offs, n + 1))) return g;
    const uint8_t* up = src;
    if (!is_pinned(src)) { if ((g = grow_host(h, &h->h_src, &h->hcap_src, src_len))) return g; memcpy(h->h_src, src, src_len); up = h->h_src; }
    HIPOK(hipMemcpyAsync(h->d_src, up, src_len, hipMemcpyHostToDevice, h->stream));
    HIPOK(hipEventRecord(h->ev0, h->stream));
    HIPOK(hipMemsetAsync(h->d_slots, 0, n * (size_t)SLOT, h->stream));
    hipLaunchKernelGGL(k_deflate_bgzf, dim3((unsigned)n), dim3(LANES), sizeof(Shared), h->stream, h->d_src, (uint64_t)src_len, h->d_slots, h->d_sizes, (uint32_t)n);
    HIPOK(hipGetLastError());
    hipLaunchKernelGGL(k_scan_sizes, dim3(1), dim3(LANES), 0, h->stream, h->d_sizes, h->d_offs, (uint32_t)n);
    HIPOK(hipGetLastError());
    hipLaunchKernelGGL(k_gather, dim3((unsigned)n), dim3(LANES), 0, h->stream, h->d_slots, h->d_sizes, h->d_offs, h->d_out, (uint32_t)n);
    HIPOK(hipGetLastError());
    HIPOK(hipEventRecord(h->ev1, h->stream));
    // (the total decides how many bytes to fetch, so it is waited for first)
    HIPOK(hipMemcpyAsync(h->h_total, h->d_offs + n, sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HIPOK(hipStreamSynchronize(h->stream));
    const size_t total = (size_t)*h->h_total;
    if (total > dst_cap || total > n * (size_t)SLOT) { h->err = "the members outgrew their bound"; return BRC_E_HIP; }      // (cannot happen: every member is at most its input + 31)
    uint8_t* down = dst;
    const bool dst_pinned = is_pinned(dst);
    if (!dst_pinned) { if ((g = grow_host(h, &h->h_dst, &h->hcap_dst, total))) return g; down = h->h_dst; }
    HIPOK(hipMemcpyAsync(down, h->d_out, total, hipMemcpyDeviceToHost, h->stream));
    HIPOK(hipStreamSynchronize(h->stream));
    if (!dst_pinned) memcpy(dst, h->h_dst, total);
    float ms = 0; HIPOK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    *dst_len = total; *n_members_out = n;
    h->kernel_s = ms * 1e-3; h->bytes_in = src_len; h->bytes_out = total; h->call_s = now_s() - t0;
    return BRC_OK;
}

}  // extern "C"
