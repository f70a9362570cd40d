// CPU build of the window summaries' C-ABI (include/brc_bins.h) over brc_bins_core.h: the test counterpart of libbrc_bins_hip.so, as
// libbrc_sim.so is the engine's.  The launches of the gfx950 library run here as loops on host memory: views with memory ==
// BRC_MEM_HOST (what libbrc_sim.so hands out), edge list and destinations in host memory.  Every loop — destination elements, edges,
// positions, libraries, records — runs from the LAST lane to the first: nothing may depend on the order of the lanes.  Every lane commits
// its own values (the device's reduction across a wave is brc_bins.hip's alone).  Test infrastructure only.
#include <chrono>
#include <new>
#include <string>

#include "../../bam_readcount_amd/csrc/brc_bins_core.h"

using namespace brcbins;

struct brc_bins {
    int device = 0;                 // (host views carry device 0: a handle made for another ordinal refuses them like the hip library would)
    std::string err;
    double kernel_s = 0; uint64_t bytes_read = 0, bytes_written = 0;
};

static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

extern "C" {

const char* brc_bins_kind(void) { return "sim"; }

int brc_bins_create(int device, brc_bins** out) {
    if (!out || device < 0) return BRC_E_ARG;
    *out = new (std::nothrow) brc_bins();
    if (*out) (*out)->device = device;
    return *out ? BRC_OK : BRC_E_NOMEM;
}
void brc_bins_destroy(brc_bins* h) { delete h; }
const char* brc_bins_last_error(const brc_bins* h) { return h ? h->err.c_str() : ""; }

int brc_bins_reduce(brc_bins* h, const brc_device_view* v, const brc_device_indels* d, const brc_bins_params* p, int64_t k0, int64_t n,
                    uint64_t* sums, uint64_t* covered, uint64_t* hist, int64_t dst_stride, uint32_t* status, void*) {
    if (!h) return BRC_E_ARG;
    h->err.clear(); h->kernel_s = 0; h->bytes_read = h->bytes_written = 0;
    const char* why = "";
    if (check_job(v, d, p, k0, n, dst_stride, &why)) { h->err = why; return BRC_E_ARG; }
    if (v->memory != BRC_MEM_HOST) { h->err = "the views do not lie in host memory"; return BRC_E_ARG; }
    if (v->device != h->device) { h->err = "the views lie on another device"; return BRC_E_ARG; }
    const Job J = make_job(v, d, p, k0, n, dst_stride, sums, covered, hist, status);
    if (!wants_sums(J) && !wants_cov(J) && !wants_hist(J) && !status) return BRC_OK;
    const double t0 = now_s();
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
    h->kernel_s = now_s() - t0;
    job_bytes(J, &h->bytes_read, &h->bytes_written);
    return BRC_OK;
}

void brc_bins_last_timing(const brc_bins* h, double* kernel_s, uint64_t* bytes_read, uint64_t* bytes_written) {
    if (!h) return;
    if (kernel_s) *kernel_s = h->kernel_s;
    if (bytes_read) *bytes_read = h->bytes_read;
    if (bytes_written) *bytes_written = h->bytes_written;
}

}  // extern "C"
