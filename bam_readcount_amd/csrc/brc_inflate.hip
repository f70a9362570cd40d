// brc_inflate.hip — device-side BGZF inflate for gfx950 behind the C-ABI of include/brc_inflate.h (libbrc_inflate_hip.so; a
// translation unit and a library of its own: the engine's libraries keep exactly the device code they had).
//
// One wave (a workgroup of 64 lanes) per BGZF member; the decoder itself is brc_inflate_core.h, shared with the CPU build the
// tests run.  LDS per workgroup: sizeof(brcinf::Shared) = 64 KB output window + 5.6 KB of tables and lists, two workgroups per CU
// (160 KB), 512 members in flight on 256 CUs.  DESIGN.md 6a has the reasoning and the measurements.
#include <hip/hip_runtime.h>

#include <vector>

#include <string.h>

#include "brc_inflate_plan.h"
#include "brc_codec_hip.h"

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

struct brc_inflater : brccodec::Handle {
    brccodec::DevBuf<uint8_t> d_src, d_dst, d_status; brccodec::DevBuf<Member> d_members;
    std::vector<Member> members;
    std::vector<uint8_t> st;
};

extern "C" {

const char* brc_inflater_kind(void) { return "hip-gfx950"; }
int brc_inflater_create(int device, brc_inflater** out) { return brccodec::create(device, (const void*)k_inflate_bgzf, sizeof(Shared), out); }
void brc_inflater_destroy(brc_inflater* h) { brccodec::destroy(h); }
const char* brc_inflater_last_error(const brc_inflater* h) { return brccodec::last_error(h); }
void brc_inflater_last_timing(const brc_inflater* h, double* kernel_s, double* call_s, uint64_t* bytes_in, uint64_t* bytes_out) { brccodec::last_timing(h, kernel_s, call_s, bytes_in, bytes_out); }
void* brc_inflate_host_alloc(size_t bytes) { return brccodec::host_alloc(bytes); }
void brc_inflate_host_free(void* p) { brccodec::host_free(p); }

int brc_inflate_bgzf(brc_inflater* h, const void* src_, size_t src_len, void* dst_, size_t dst_cap, uint64_t* dst_off, uint8_t* status, size_t* n_members) {
    if (!h || !n_members || !dst_off || (!src_ && src_len) || (!dst_ && dst_cap) || (!status && *n_members)) return BRC_E_ARG;
    brccodec::Call call(h);
    const uint8_t* src = (const uint8_t*)src_; uint8_t* dst = (uint8_t*)dst_;
    bool run = false;
    const int rc = plan_chain(src, src_len, dst_cap, *n_members, h->members, dst_off, status, n_members, &run);
    const size_t n = h->members.size();
    if (!run || n == 0) return call.early(rc);
    if (n > 0x7fffffffu) return BRC_E_ARG;
    // (plan_chain: every listed member lies inside src[0, src_len) and its slot inside dst[0, dst_cap))
    const size_t used = (size_t)(h->members[n - 1].src_off + h->members[n - 1].clen), out_bytes = (size_t)dst_off[n];
    HIPOK(hipSetDevice(h->device));
    int g;
    if ((g = h->d_src.grow(h, used + 16)) || (g = h->d_dst.grow(h, out_bytes + 16)) || (g = h->d_status.grow(h, n)) || (g = h->d_members.grow(h, n))) return g;
    bool dst_pinned;
    if ((g = brccodec::landing(h, dst, out_bytes, &dst_pinned))) return g;
    uint8_t* down = dst_pinned ? dst : h->h_dst.p;
    if ((g = brccodec::upload(h, h->d_src.p, src, used))) return g;
    HIPOK(hipMemcpyAsync(h->d_members.p, h->members.data(), n * sizeof(Member), hipMemcpyHostToDevice, h->stream));
    HIPOK(hipEventRecord(h->ev0, h->stream));
    LAUNCH(k_inflate_bgzf, dim3((unsigned)n), dim3(LANES), sizeof(Shared), h->stream, h->d_src.p, h->d_dst.p, h->d_members.p, h->d_status.p, (uint32_t)n);
    HIPOK(hipEventRecord(h->ev1, h->stream));
    h->st.resize(n);
    HIPOK(hipMemcpyAsync(h->st.data(), h->d_status.p, n, hipMemcpyDeviceToHost, h->stream));
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
        if (b > a) HIPOK(hipMemcpyAsync(down + a, h->d_dst.p + a, b - a, hipMemcpyDeviceToHost, h->stream));
        i = j;
    }
    HIPOK(hipStreamSynchronize(h->stream));
    if (!dst_pinned) {
        if (all_ok) memcpy(dst, down, out_bytes);
        else for (size_t i = 0; i < n; ++i) if (h->st[i] == ST_OK) memcpy(dst + dst_off[i], down + dst_off[i], (size_t)(dst_off[i + 1] - dst_off[i]));
    }
    memcpy(status, h->st.data(), n);
    if ((g = call.done(used, out_bytes))) return g;
    return rc;
}

}  // extern "C"
