// CPU build of the window summaries' C-ABI (include/brc_bins.h) over brc_bins_core.h: the test counterpart of libbrc_bins_hip.so, as
// libbrc_sim.so is the engine's.  The launches of the gfx950 library run here as loops on host memory: views with memory ==
// BRC_MEM_HOST (what libbrc_sim.so hands out), edge list and destinations in host memory.  Every loop — destination elements, edges,
// positions, libraries, records — runs from the LAST lane to the first: nothing may depend on the order of the lanes.  Every lane commits
// its own values (the device's reduction across a wave is brc_bins.hip's alone).  Test infrastructure only.
#include "../../bam_readcount_amd/csrc/brc_bins_core.h"
#include "../sim_side.h"

using namespace brcbins;

struct brc_bins : brcside::Handle {};

extern "C" {

const char* brc_bins_kind(void) { return "sim"; }
int brc_bins_create(int device, brc_bins** out) { return brcside::create(device, out); }
void brc_bins_destroy(brc_bins* h) { brcside::destroy(h); }
const char* brc_bins_last_error(const brc_bins* h) { return brcside::last_error(h); }
void brc_bins_last_timing(const brc_bins* h, double* kernel_s, uint64_t* bytes_read, uint64_t* bytes_written) { brcside::last_timing(h, kernel_s, bytes_read, bytes_written); }

int brc_bins_reduce(brc_bins* h, const brc_device_view* v, const brc_device_indels* d, const brc_bins_params* p, int64_t k0, int64_t n,
                    uint64_t* sums, uint64_t* covered, uint64_t* hist, int64_t dst_stride, uint32_t* status, void*) {
    if (!h) return BRC_E_ARG;
    brcside::clear(h);
    const char* why = "";
    if (check_job(v, d, p, k0, n, dst_stride, &why)) return brcside::refuse(h, why);
    if (int rc = brcside::resident(h, v, brcside::TWO_VIEWS)) return rc;
    const Job J = make_job(v, d, p, k0, n, dst_stride, sums, covered, hist, status);
    if (!wants_sums(J) && !wants_cov(J) && !wants_hist(J) && !status) return BRC_OK;
    brcside::start(h);
    for (uint64_t i = clear_total(J); i-- > 0;) clear_lane(J, i);
    if (J.edges && status)
        for (uint64_t i = (uint64_t)J.n_bins + 1u; i-- > 0;) edge_lane(J, i);
    if (sweeps(J)) {
        for (int l = J.Lp - 1; l >= 0; --l)
            for (int64_t j = n - 1; j >= 0; --j) {
                const Lane o = plane_lane(J, l, j);
                if (wants_hist(J) && o.bin >= 0) add64(J.o_hist + (int64_t)l * J.n_hist + hist_bar(J, o.depth), 1u);
                commit_lane(J, l, o);
            }
        if (walks_records(J))
            for (uint64_t r = J.n_xagg; r-- > 0;) record_lane(J, r);
        if (walks_slots(J))
            for (uint64_t s = J.n_slots; s-- > 0;) indel_lane(J, s);
    }
    return brcside::done(h, J);
}

}  // extern "C"
