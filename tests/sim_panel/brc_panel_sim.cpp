// CPU build of the device-resident site panels' C-ABI (include/brc_panel.h) over brc_panel_core.h: the test counterpart of
// libbrc_panel_hip.so, as libbrc_sim.so is the engine's.  The two launches of the gfx950 library run here as two loops on host memory:
// a view with memory == BRC_MEM_HOST (what libbrc_sim.so hands out), idx and the status word in host memory.  The planes loop runs
// from the LAST lane to the first: nothing may depend on the order of the lanes.  Test infrastructure only.
#include "../../bam_readcount_amd/csrc/brc_panel_core.h"
#include "../sim_side.h"

using namespace brcpanel;

struct brc_panel : brcside::Handle {};

extern "C" {

const char* brc_panel_kind(void) { return "sim"; }
int brc_panel_create(int device, brc_panel** out) { return brcside::create(device, out); }
void brc_panel_destroy(brc_panel* h) { brcside::destroy(h); }
const char* brc_panel_last_error(const brc_panel* h) { return brcside::last_error(h); }
void brc_panel_last_timing(const brc_panel* h, double* kernel_s, uint64_t* bytes_read, uint64_t* bytes_written) { brcside::last_timing(h, kernel_s, bytes_read, bytes_written); }

int brc_panel_gather(brc_panel* h, const brc_device_view* v, const int32_t* idx, int64_t n, int64_t dst_stride, uint32_t* ncol, uint32_t* depth,
                     uint32_t* unavail, uint32_t* istat, float* fstat, float* metrics, uint32_t* status, void*) {
    if (!h) return BRC_E_ARG;
    brcside::clear(h);
    const char* why = "";
    if (check_job(v, idx, n, dst_stride, &why)) return brcside::refuse(h, why);
    if (int rc = brcside::resident(h, v, brcside::ONE_VIEW)) return rc;
    const bool dests = ncol || depth || unavail || istat || fstat || metrics;
    if (!status && (n == 0 || !dests)) return BRC_OK;
    if (status) *status = 0;
    if (n == 0) return BRC_OK;
    const Job J = make_job(v, idx, n, dst_stride, ncol, depth, unavail, istat, fstat, metrics, status);
    brcside::start(h);
    for (int l = (dests ? J.Lp : 1) - 1; l >= 0; --l) for (int64_t j = n - 1; j >= 0; --j) gather_lane(J, l, j);
    if (wants_buckets(J)) for (uint64_t r = 0; r < J.n_xagg; ++r) overlay_lane(J, r);
    return brcside::done(h, J);
}

}  // extern "C"
