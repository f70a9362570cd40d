// sim_side.h — what the CPU builds of the side libraries share (sim_dense, sim_indels, sim_panel, sim_select, sim_bins): the handle
// behind their C-ABIs, its lifecycle, the checks in front of a call's loops and the bookkeeping behind them, under the names of
// bam_readcount_amd/csrc/brc_side_hip.h, so that the two entry points of a library read alike.  Here a view lies in host memory, the
// stream is nobody's, and the time is the wall clock around the loops.  All of it static: nothing of it is exported.
// Test infrastructure only.
#pragma once
#include <chrono>
#include <new>
#include <string>

#include "../include/brc.h"

namespace brcside {

struct Handle {
    int device = 0;                 // (host views carry device 0: a handle made for another ordinal refuses them like the hip library would)
    std::string err;
    double t0 = 0, kernel_s = 0; uint64_t bytes_read = 0, bytes_written = 0;
};

static inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

template <class H> static int create(int device, H** out) {
    if (!out || device < 0) return BRC_E_ARG;
    *out = new (std::nothrow) H();
    if (*out) (*out)->device = device;
    return *out ? BRC_OK : BRC_E_NOMEM;
}
template <class H> static void destroy(H* h) { delete h; }
static inline const char* last_error(const Handle* h) { return h ? h->err.c_str() : ""; }

static inline void last_timing(const Handle* h, double* kernel_s, uint64_t* bytes_read, uint64_t* bytes_written) {
    if (!h) return;
    if (kernel_s) *kernel_s = h->kernel_s;
    if (bytes_read) *bytes_read = h->bytes_read;
    if (bytes_written) *bytes_written = h->bytes_written;
}

static inline void clear(Handle* h) { h->err.clear(); h->kernel_s = 0; h->bytes_read = h->bytes_written = 0; }

static inline int refuse(Handle* h, const char* why) { h->err = why; return BRC_E_ARG; }

enum Views { ONE_VIEW, TWO_VIEWS };
template <class View> static int resident(Handle* h, const View* v, Views views) {
    if (v->memory != BRC_MEM_HOST) return refuse(h, views == ONE_VIEW ? "the view does not lie in host memory" : "the views do not lie in host memory");
    if (v->device != h->device) return refuse(h, views == ONE_VIEW ? "the view lies on another device" : "the views lie on another device");
    return BRC_OK;
}

static inline void start(Handle* h) { h->t0 = now_s(); }
template <class Job> static int done(Handle* h, const Job& J) {
    h->kernel_s = now_s() - h->t0;
    job_bytes(J, &h->bytes_read, &h->bytes_written);
    return BRC_OK;
}

}  // namespace brcside
