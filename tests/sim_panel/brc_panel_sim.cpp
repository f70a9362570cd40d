// CPU build of the device-resident site panels' C-ABI (include/brc_panel.h) over brc_panel_core.h: the test counterpart of
// libbrc_panel_hip.so, as libbrc_sim.so is the engine's.  The two launches of the gfx950 library run here as two loops on host memory:
// a view with memory == BRC_MEM_HOST (what libbrc_sim.so hands out), idx and the status word in host memory.  The planes loop runs
// from the LAST lane to the first: nothing may depend on the order of the lanes.  Test infrastructure only.
#include <chrono>
#include <new>
#include <string>

#include "../../bam_readcount_amd/csrc/brc_panel_core.h"

using namespace brcpanel;

struct brc_panel {
    int device = 0;                 // (host views carry device 0: a handle made for another ordinal refuses them like the hip library would)
    std::string err;
    double kernel_s = 0; uint64_t bytes_read = 0, bytes_written = 0;
};

static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

extern "C" {

const char* brc_panel_kind(void) { return "sim"; }

int brc_panel_create(int device, brc_panel** out) {
    if (!out || device < 0) return BRC_E_ARG;
    *out = new (std::nothrow) brc_panel();
    if (*out) (*out)->device = device;
    return *out ? BRC_OK : BRC_E_NOMEM;
}
void brc_panel_destroy(brc_panel* h) { delete h; }
const char* brc_panel_last_error(const brc_panel* h) { return h ? h->err.c_str() : ""; }

int brc_panel_gather(brc_panel* h, const brc_device_view* v, const int32_t* idx, int64_t n, int64_t dst_stride, uint32_t* ncol, uint32_t* depth,
                     uint32_t* unavail, uint32_t* istat, float* fstat, float* metrics, uint32_t* status, void*) {
    if (!h) return BRC_E_ARG;
    h->err.clear(); h->kernel_s = 0; h->bytes_read = h->bytes_written = 0;
    const char* why = "";
    if (check_job(v, idx, n, dst_stride, &why)) { h->err = why; return BRC_E_ARG; }
    if (v->memory != BRC_MEM_HOST) { h->err = "the view does not lie in host memory"; return BRC_E_ARG; }
    if (v->device != h->device) { h->err = "the view lies on another device"; return BRC_E_ARG; }
    const bool dests = ncol || depth || unavail || istat || fstat || metrics;
    if (!status && (n == 0 || !dests)) return BRC_OK;
    if (status) *status = 0;
    if (n == 0) return BRC_OK;
    const Job J = make_job(v, idx, n, dst_stride, ncol, depth, unavail, istat, fstat, metrics, status);
    const double t0 = now_s();
    for (int l = (dests ? J.Lp : 1) - 1; l >= 0; --l) for (int64_t j = n - 1; j >= 0; --j) gather_lane(J, l, j);
    if (wants_buckets(J)) for (uint64_t r = 0; r < J.n_xagg; ++r) overlay_lane(J, r);
    h->kernel_s = now_s() - t0;
    job_bytes(J, &h->bytes_read, &h->bytes_written);
    return BRC_OK;
}

void brc_panel_last_timing(const brc_panel* h, double* kernel_s, uint64_t* bytes_read, uint64_t* bytes_written) {
    if (!h) return;
    if (kernel_s) *kernel_s = h->kernel_s;
    if (bytes_read) *bytes_read = h->bytes_read;
    if (bytes_written) *bytes_written = h->bytes_written;
}

}  // extern "C"
