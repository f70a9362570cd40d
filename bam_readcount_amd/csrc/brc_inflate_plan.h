// brc_inflate_plan.h — host side shared by every build of the inflater (brc_inflate.hip, tests/sim_inflate): the walk over the BSIZE
// chain of brc_inflate_bgzf (include/brc_inflate.h) and its argument rules.
#ifndef BRC_INFLATE_PLAN_H
#define BRC_INFLATE_PLAN_H

#include <vector>

#include "../../include/brc_inflate.h"
#include "brc_inflate_core.h"

namespace brcinf {

// The members of src[0, src_len) and where their bytes go.  Returns BRC_OK, or BRC_E_ARG with the whole members in front of the
// break in `m` (*broken) or with nothing to run (capacity / dst_cap short: *run = false).
static inline int plan_chain(const uint8_t* src, size_t src_len, size_t dst_cap, size_t cap, std::vector<Member>& m, uint64_t* dst_off, uint8_t* status, size_t* n_members, bool* run) {
    m.clear(); *run = false;
    bool broken = false;
    uint64_t out = 0;
    for (size_t o = 0; o < src_len;) {
        uint32_t total = 0, hdr = 0;
        if (member_header(src + o, src_len - o, &total, &hdr) != 0 || total > src_len - o) { broken = true; break; }
        Member x; x.pre_status = ST_OK; x.src_off = o + hdr; x.dst_off = out; x.clen = 0; x.isize = 0; x.crc = 0;
        if (total < hdr + 8u) x.pre_status = ST_BAD_HEADER;
        else {
            const uint8_t* t = src + o + total - 8;
            x.clen = total - hdr - 8u;
            x.crc = (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
            x.isize = (uint32_t)t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24;
            if (x.isize > WINDOW) { x.pre_status = ST_BAD_HEADER; x.isize = 0; }
        }
        out += x.isize;
        m.push_back(x);
        o += total;
    }
    const size_t n = m.size();
    *n_members = n;
    if (n > cap) return BRC_E_ARG;
    for (size_t i = 0; i < n; ++i) { dst_off[i] = m[i].dst_off; status[i] = (uint8_t)m[i].pre_status; }
    dst_off[n] = out;
    if (out > dst_cap) return BRC_E_ARG;
    *run = true;
    return broken ? BRC_E_ARG : BRC_OK;
}

}  // namespace brcinf
#endif
