// CPU build of the indel candidate filter's C-ABI (include/brc_ivet.h) over brc_ivet_core.h: the test counterpart of libbrc_ivet_hip.so,
// as libbrc_sim.so is the engine's.  The launches of the gfx950 library run here as loops on host memory: views with memory ==
// BRC_MEM_HOST (what libbrc_sim.so hands out), table, list, scratch and destinations in host memory.  The loops run from the LAST lane
// to the first: nothing may depend on the order of the lanes.  Test infrastructure only.
#include <string.h>

#include "../../bam_readcount_amd/csrc/brc_ivet_core.h"
#include "../sim_side.h"

using namespace brcivet;

struct brc_ivet : brcside::Handle {};

extern "C" {

const char* brc_ivet_kind(void) { return "sim"; }
int brc_ivet_create(int device, brc_ivet** out) { return brcside::create(device, out); }
void brc_ivet_destroy(brc_ivet* h) { brcside::destroy(h); }
const char* brc_ivet_last_error(const brc_ivet* h) { return brcside::last_error(h); }
void brc_ivet_last_timing(const brc_ivet* h, double* kernel_s, uint64_t* bytes_read, uint64_t* bytes_written) { brcside::last_timing(h, kernel_s, bytes_read, bytes_written); }
int64_t brc_ivet_workspace(const brc_device_view* v, int64_t m) { return workspace_bytes(v, m); }

int brc_ivet_records(brc_ivet* h, const brc_device_view* v, const brc_device_indels* d, const brc_ivet_params* p, const brc_ivet_table* t, const int32_t* idx,
                     const uint32_t* why, int64_t n, int64_t dst_stride, uint32_t* fail, float* vals, uint32_t* ctl_count, uint32_t* keep, uint32_t* status,
                     void* workspace, void*) {
    if (!h) return BRC_E_ARG;
    brcside::clear(h);
    const char* said = "";
    if (check_job(v, d, p, t, idx, n, dst_stride, workspace, &said)) return brcside::refuse(h, said);
    if (int rc = brcside::resident(h, v, brcside::TWO_VIEWS)) return rc;
    const Job J = make_job(v, d, p, t, idx, why, n, dst_stride, fail, vals, ctl_count, keep, status, workspace);
    if (!status && !(keep && n > 0) && !(wants_dests(J) && J.m > 0)) return BRC_OK;
    if (status) *status = 0u;
    if (keep && n > 0) memset(keep, 0, (size_t)n * sizeof(uint32_t));
    const bool lanes = (status && lanes_of(J) > 0) || (wants_dests(J) && J.m > 0);
    if (!lanes) return BRC_OK;
    brcside::start(h);
    if (walks_records(J)) {
        memset(J.V.head, 0xff, (size_t)J.m * sizeof(uint32_t));
        for (uint64_t r = J.V.n_xagg; r-- > 0;) link_lane(J, r);
    }
    for (int64_t i = (int64_t)lanes_of(J) - 1; i >= 0; --i) {
        if (i < J.n) list_lane(J, i);
        if (i < J.m) record_lane(J, i);
    }
    return brcside::done(h, J);
}

}  // extern "C"
