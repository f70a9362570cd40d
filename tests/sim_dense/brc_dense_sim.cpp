// CPU build of the device-resident results' C-ABI (include/brc_dense.h) over brc_dense_core.h: the test counterpart of
// libbrc_dense_hip.so, as libbrc_sim.so is the engine's.  The two launches of the gfx950 library run here as two loops in the same
// order — every (library, position) lane of the planes kernel, then every record lane of the overlay — on host memory: a view with
// memory == BRC_MEM_HOST (what libbrc_sim.so hands out).  Test infrastructure only.
#include "../../bam_readcount_amd/csrc/brc_dense_core.h"
#include "../sim_side.h"

using namespace brcdense;

struct brc_dense : brcside::Handle {};

extern "C" {

const char* brc_dense_kind(void) { return "sim"; }
int brc_dense_create(int device, brc_dense** out) { return brcside::create(device, out); }
void brc_dense_destroy(brc_dense* h) { brcside::destroy(h); }
const char* brc_dense_last_error(const brc_dense* h) { return brcside::last_error(h); }
void brc_dense_last_timing(const brc_dense* h, double* kernel_s, uint64_t* bytes_read, uint64_t* bytes_written) { brcside::last_timing(h, kernel_s, bytes_read, bytes_written); }

int brc_dense_expand(brc_dense* h, const brc_device_view* v, int64_t k0, int64_t n, int64_t dst_stride, uint32_t* ncol, uint32_t* depth,
                     uint32_t* unavail, uint32_t* istat, float* fstat, float* metrics, void*) {
    if (!h) return BRC_E_ARG;
    brcside::clear(h);
    const char* why = "";
    if (check_job(v, k0, n, dst_stride, &why)) return brcside::refuse(h, why);
    if (int rc = brcside::resident(h, v, brcside::ONE_VIEW)) return rc;
    if (n == 0 || (!ncol && !depth && !unavail && !istat && !fstat && !metrics)) return BRC_OK;
    const Job J = make_job(v, k0, n, dst_stride, ncol, depth, unavail, istat, fstat, metrics);
    brcside::start(h);
    for (int l = 0; l < J.Lp; ++l) for (int64_t j = 0; j < n; ++j) expand_lane(J, l, j);
    if (istat || fstat || metrics) for (uint64_t r = 0; r < J.n_xagg; ++r) overlay_lane(J, r);
    return brcside::done(h, J);
}

}  // extern "C"
