// brc_deflate.hip — device-side BGZF compression for gfx950 behind the C-ABI of include/brc_deflate.h (libbrc_deflate_hip.so; a
// translation unit and a library of its own: the engine's and the inflater's libraries keep exactly the device code they had).
//
// One workgroup of 256 lanes per member; the compressor itself is brc_deflate_core.h, shared with the CPU build the tests run.
// LDS per workgroup: sizeof(brcdef::Shared) = 156 660 bytes (the static_assert below; 64 KB input window + 64 KB match / token
// array + 16 KB head table + tables), one workgroup per CU (160 KB), 256 members in flight.  Every member is written into a slot of its own (zeroed first: the bits are
// ORed in); k_scan_sizes turns the member sizes into offsets and k_gather packs the members back to back, so only compressed bytes
// cross PCIe.  DESIGN.md 6b has the reasoning and the measurements.
#include <hip/hip_runtime.h>

#include <string.h>

#include "brc_deflate_core.h"
#include "../../include/brc_deflate.h"
#include "brc_codec_hip.h"

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

struct brc_deflater : brccodec::Handle {
    brccodec::DevBuf<uint8_t> d_src, d_slots, d_out; brccodec::DevBuf<uint32_t> d_sizes; brccodec::DevBuf<uint64_t> d_offs;
    uint64_t* h_total = nullptr;                                                          // page-locked: where the scan's last word lands
    ~brc_deflater() { brccodec::host_free(h_total); }
};

extern "C" {

const char* brc_deflater_kind(void) { return "hip-gfx950"; }
int brc_deflater_create(int device, brc_deflater** out) {
    const int rc = brccodec::create(device, (const void*)k_deflate_bgzf, sizeof(Shared), out);
    if (rc != BRC_OK) return rc;
    if (!((*out)->h_total = (uint64_t*)brccodec::host_alloc(sizeof(uint64_t)))) { brccodec::destroy(*out); *out = nullptr; return BRC_E_NODEVICE; }
    return BRC_OK;
}
void brc_deflater_destroy(brc_deflater* h) { brccodec::destroy(h); }
const char* brc_deflater_last_error(const brc_deflater* h) { return brccodec::last_error(h); }
void brc_deflater_last_timing(const brc_deflater* h, double* kernel_s, double* call_s, uint64_t* bytes_in, uint64_t* bytes_out) { brccodec::last_timing(h, kernel_s, call_s, bytes_in, bytes_out); }
void* brc_deflate_host_alloc(size_t bytes) { return brccodec::host_alloc(bytes); }
void brc_deflate_host_free(void* p) { brccodec::host_free(p); }

size_t brc_deflate_bound(size_t src_len) { return bound(src_len); }
const uint8_t* brc_deflate_eof_block(size_t* len) { if (len) *len = EOF_LEN; return eof_member(); }

int brc_deflate_bgzf(brc_deflater* h, const void* src_, size_t src_len, void* dst_, size_t dst_cap, size_t* dst_len, size_t* n_members_out) {
    if (!h || !dst_len || !n_members_out || (!src_ && src_len) || (!dst_ && src_len) || dst_cap < bound(src_len)) return BRC_E_ARG;
    brccodec::Call call(h);
    *dst_len = 0; *n_members_out = 0;
    const size_t n = n_members(src_len);
    if (n == 0) return call.early(BRC_OK);
    if (n > 0x7fffffffu) return BRC_E_ARG;
    uint8_t* dst = (uint8_t*)dst_;
    HIPOK(hipSetDevice(h->device));
    int g;
    if ((g = h->d_src.grow(h, src_len + 16)) || (g = h->d_slots.grow(h, n * (size_t)SLOT)) || (g = h->d_out.grow(h, n * (size_t)SLOT)) ||
        (g = h->d_sizes.grow(h, n)) || (g = h->d_offs.grow(h, n + 1))) return g;
    if ((g = brccodec::upload(h, h->d_src.p, src_, src_len))) return g;
    HIPOK(hipEventRecord(h->ev0, h->stream));
    HIPOK(hipMemsetAsync(h->d_slots.p, 0, n * (size_t)SLOT, h->stream));
    LAUNCH(k_deflate_bgzf, dim3((unsigned)n), dim3(LANES), sizeof(Shared), h->stream, h->d_src.p, (uint64_t)src_len, h->d_slots.p, h->d_sizes.p, (uint32_t)n);
    LAUNCH(k_scan_sizes, dim3(1), dim3(LANES), 0, h->stream, h->d_sizes.p, h->d_offs.p, (uint32_t)n);
    LAUNCH(k_gather, dim3((unsigned)n), dim3(LANES), 0, h->stream, h->d_slots.p, h->d_sizes.p, h->d_offs.p, h->d_out.p, (uint32_t)n);
    HIPOK(hipEventRecord(h->ev1, h->stream));
    // (the total decides how many bytes to fetch, so it is waited for first)
    HIPOK(hipMemcpyAsync(h->h_total, h->d_offs.p + n, sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HIPOK(hipStreamSynchronize(h->stream));
    const size_t total = (size_t)*h->h_total;
    if (total > dst_cap || total > n * (size_t)SLOT) { h->err = "the members outgrew their bound"; return BRC_E_HIP; }      // (cannot happen: every member is at most its input + 31)
    bool dst_pinned;
    if ((g = brccodec::landing(h, dst, total, &dst_pinned))) return g;
    HIPOK(hipMemcpyAsync(dst_pinned ? dst : h->h_dst.p, h->d_out.p, total, hipMemcpyDeviceToHost, h->stream));
    HIPOK(hipStreamSynchronize(h->stream));
    if (!dst_pinned) memcpy(dst, h->h_dst.p, total);
    if ((g = call.done(src_len, total))) return g;
    *dst_len = total; *n_members_out = n;
    return BRC_OK;
}

}  // extern "C"
