// CPU build of the deflater's C-ABI (include/brc_deflate.h) over brc_deflate_core.h: the test counterpart of libbrc_deflate_hip.so,
// as libbrc_inflate_sim.so is the inflater's.  Every member is compressed by deflate_member() — the function the gfx950 kernel
// runs — with the 256 lanes of each parallel phase executed one after the other, into a zeroed slot of its own; the members are
// spread over host threads and then packed back to back, as the device's scan and gather kernels do.  Test infrastructure only.
#include <string.h>

#include <vector>

#include "../../bam_readcount_amd/csrc/brc_deflate_core.h"
#include "../../include/brc_deflate.h"
#include "../sim_codec.h"

using namespace brcdef;

struct brc_deflater : brccodec::Handle {};

extern "C" {

const char* brc_deflater_kind(void) { return "sim"; }
int brc_deflater_create(int device, brc_deflater** out) { return brccodec::create(device, out); }
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
    const uint8_t* src = (const uint8_t*)src_; uint8_t* dst = (uint8_t*)dst_;
    std::vector<uint32_t> slots(n * (size_t)SLOT_WORDS, 0u), sizes(n);
    brccodec::for_members<Shared>(n, 4, [&](Shared& sh, size_t i) {
        const size_t off = i * (size_t)MEMBER_IN;
        // (the member's input as an exact sub-range: a sanitizer build sees every read outside it)
        sizes[i] = deflate_member(sh, src + off, (uint32_t)(src_len - off < MEMBER_IN ? src_len - off : MEMBER_IN), slots.data() + i * (size_t)SLOT_WORDS);
    });
    size_t total = 0;
    for (size_t i = 0; i < n; ++i) {
        if (sizes[i] > SLOT || total + sizes[i] > dst_cap) { h->err = "a member outgrew its bound"; return BRC_E_HIP; }
        memcpy(dst + total, slots.data() + i * (size_t)SLOT_WORDS, sizes[i]); total += sizes[i];
    }
    *dst_len = total; *n_members_out = n;
    return call.done(call.t0, src_len, total);
}

}  // extern "C"
