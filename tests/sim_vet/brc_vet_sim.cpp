// CPU build of the candidate filter's C-ABI (include/brc_vet.h) over brc_vet_core.h: the test counterpart of libbrc_vet_hip.so, as
// libbrc_sim.so is the engine's.  The launches of the gfx950 library run here as loops on host memory: views with memory ==
// BRC_MEM_HOST (what libbrc_sim.so hands out), lists, scratch and destinations in host memory.  The record and element loops run from the
// LAST lane to the first: nothing may depend on the order of the lanes (an element's list of records comes out reversed against an
// ascending run).  Test infrastructure only.
#include <string.h>

#include "../../bam_readcount_amd/csrc/brc_vet_core.h"
#include "../sim_side.h"

using namespace brcvet;

struct brc_vet : brcside::Handle {};

extern "C" {

const char* brc_vet_kind(void) { return "sim"; }
int brc_vet_create(int device, brc_vet** out) { return brcside::create(device, out); }
void brc_vet_destroy(brc_vet* h) { brcside::destroy(h); }
const char* brc_vet_last_error(const brc_vet* h) { return brcside::last_error(h); }
void brc_vet_last_timing(const brc_vet* h, double* kernel_s, uint64_t* bytes_read, uint64_t* bytes_written) { brcside::last_timing(h, kernel_s, bytes_read, bytes_written); }
int64_t brc_vet_workspace(const brc_device_view* v, int64_t n) { return workspace_bytes(v, n); }

int brc_vet_sites(brc_vet* h, const brc_device_view* v, const brc_device_indels* d, const brc_vet_params* p, const int32_t* idx, const uint32_t* alt, int64_t n,
                  int64_t dst_stride, uint32_t* fail, uint32_t* keep, float* vals, uint32_t* status, void* workspace, void*) {
    if (!h) return BRC_E_ARG;
    brcside::clear(h);
    const char* why = "";
    if (check_job(v, d, p, idx, n, dst_stride, workspace, &why)) return brcside::refuse(h, why);
    if (int rc = brcside::resident(h, v, brcside::TWO_VIEWS)) return rc;
    const bool dests = fail || keep || vals;
    if (!status && (n == 0 || !dests)) return BRC_OK;
    if (status) *status = 0u;
    if (n == 0) return BRC_OK;
    const Job J = make_job(v, d, p, idx, alt, n, dst_stride, fail, keep, vals, status, workspace);
    brcside::start(h);
    if (walks_records(J)) {
        memset(J.head, 0xff, (size_t)n * sizeof(uint32_t));
        for (uint64_t r = J.n_xagg; r-- > 0;) link_lane(J, r);
    }
    for (int64_t j = n - 1; j >= 0; --j) sites_lane(J, j);
    return brcside::done(h, J);
}

}  // extern "C"
