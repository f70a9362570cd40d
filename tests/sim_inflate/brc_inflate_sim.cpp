// CPU build of the inflater's C-ABI (include/brc_inflate.h) over brc_inflate_core.h: the test counterpart of libbrc_inflate_hip.so,
// as libbrc_sim.so is the engine's.  Every member is decoded by inflate_member() — the function the gfx950 kernel runs — with the 64
// lanes of each parallel phase executed one after the other; members are spread over host threads.  Test infrastructure only.
#include <string.h>

#include <vector>

#include "../../bam_readcount_amd/csrc/brc_inflate_plan.h"
#include "../sim_codec.h"

using namespace brcinf;

struct brc_inflater : brccodec::Handle {
    std::vector<Member> members;
};

extern "C" {

const char* brc_inflater_kind(void) { return "sim"; }
int brc_inflater_create(int device, brc_inflater** out) { return brccodec::create(device, out); }
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
    const double k0 = brccodec::now_s();
    brccodec::for_members<Shared>(n, 8, [&](Shared& sh, size_t i) {
        const Member& m = h->members[i];
        // (the member's payload and slot as exact sub-ranges: a sanitizer build sees every step outside them)
        status[i] = (uint8_t)(m.pre_status ? (int)m.pre_status : inflate_member(sh, src + m.src_off, m.clen, dst + m.dst_off, m.isize, m.crc));
    });
    call.done(k0, src_len, dst_off[n]);
    return rc;
}

}  // extern "C"
