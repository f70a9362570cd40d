// CPU build of the device-resident results' C-ABI (include/brc_dense.h) over brc_dense_core.h: the test counterpart of
// libbrc_dense_hip.so, as libbrc_sim.so is the engine's.  The two launches of the gfx950 library run here as two loops in the same
// order — every (library, position) lane of the planes kernel, then every record lane of the overlay — on host memory: a view with
// memory == BRC_MEM_HOST (what libbrc_sim.so hands out).  Test infrastructure only.
#include <chrono>
#include <new>
#include <string>

#include "../../bam_readcount_amd/csrc/brc_dense_core.h"

using namespace brcdense;

struct brc_dense {
    int device = 0;                 // (host views carry device 0: a handle made for another ordinal refuses them like the hip library would)
    std::string err;
    double kernel_s = 0; uint64_t bytes_read = 0, bytes_written = 0;
};

static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

extern "C" {

const char* brc_dense_kind(void) { return "sim"; }

int brc_dense_create(int device, brc_dense** out) {
    if (!out || device < 0) return BRC_E_ARG;
    *out = new (std::nothrow) brc_dense();
    if (*out) (*out)->device = device;
    return *out ? BRC_OK : BRC_E_NOMEM;
}
void brc_dense_destroy(brc_dense* h) { delete h; }
const char* brc_dense_last_error(const brc_dense* h) { return h ? h->err.c_str() : ""; }

int brc_dense_expand(brc_dense* h, const brc_device_view* v, int64_t k0, int64_t n, int64_t dst_stride, uint32_t* ncol, uint32_t* depth,
                     uint32_t* unavail, uint32_t* istat, float* fstat, float* metrics, void*) {
    if (!h) return BRC_E_ARG;
    h->err.clear(); h->kernel_s = 0; h->bytes_read = h->bytes_written = 0;
    const char* why = "";
    if (check_job(v, k0, n, dst_stride, &why)) { h->err = why; return BRC_E_ARG; }
    if (v->memory != BRC_MEM_HOST) { h->err = "the view does not lie in host memory"; return BRC_E_ARG; }
    if (v->device != h->device) { h->err = "the view lies on another device"; return BRC_E_ARG; }
    if (n == 0 || (!ncol && !depth && !unavail && !istat && !fstat && !metrics)) return BRC_OK;
    const Job J = make_job(v, k0, n, dst_stride, ncol, depth, unavail, istat, fstat, metrics);
    const double t0 = now_s();
    for (int l = 0; l < J.Lp; ++l) for (int64_t j = 0; j < n; ++j) expand_lane(J, l, j);
    if (istat || fstat || metrics) for (uint64_t r = 0; r < J.n_xagg; ++r) overlay_lane(J, r);
    h->kernel_s = now_s() - t0;
    job_bytes(J, &h->bytes_read, &h->bytes_written);
    return BRC_OK;
}

void brc_dense_last_timing(const brc_dense* h, double* kernel_s, uint64_t* bytes_read, uint64_t* bytes_written) {
    if (!h) return;
    if (kernel_s) *kernel_s = h->kernel_s;
    if (bytes_read) *bytes_read = h->bytes_read;
    if (bytes_written) *bytes_written = h->bytes_written;
}

}  // extern "C"
