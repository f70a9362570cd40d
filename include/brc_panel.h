/* brc_panel.h — C-ABI of the device-resident SITE PANELS: a list of plane positions of a computed region (brc_device_view,
 * include/brc.h) gathered to the dense planes of brc_result, and to the thirteen columns the reference prints, for exactly those
 * positions, IN THE MEMORY THE VIEW LIVES IN — one call on the caller's stream, nothing crosses PCIe.
 *
 * A library of its own (libbrc_panel_hip.so: the gfx950 kernels of bam_readcount_amd/csrc/brc_panel.hip; tests/sim_panel/
 * libbrc_panel_sim.so: the same per-lane functions, brc_panel_core.h, run lane for lane on host memory) with a handle of its own.  It
 * links nothing of the engine: the view is plain data.  Error codes are the BRC_E_* of include/brc.h; the columns of `metrics` are the
 * BRC_M_* of include/brc_dense.h.
 *
 * What it stands in for: a site list (-l) makes the reference run one fetch + pileup per line (bamreadcount.cpp:574-607) and print
 * the BasicStat of every (library, base) of that line's positions (:351-416, operator<<(BasicStat), BasicStat.cpp:110-159).  A caller
 * that laid its lines side by side on one axis (brc_region_windows, include/brc.h) finds the announced positions scattered over
 * planes whose other positions are EMPTY; brc_dense_expand (include/brc_dense.h) serves contiguous windows only.  This serves the
 * listed positions alone. */
#ifndef BRC_PANEL_H
#define BRC_PANEL_H

#include "brc_dense.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct brc_panel brc_panel;

/* One handle per device (hip: BRC_E_NODEVICE without a GPU — the product library has no CPU path; sim: host views carry device 0).
 * The handle owns two timing events and nothing else: sources are the view's, the list and the destinations the caller's. */
int  brc_panel_create(int device, brc_panel** out);
void brc_panel_destroy(brc_panel*);
const char* brc_panel_kind(void);                         /* "hip-gfx950" | "sim" */
const char* brc_panel_last_error(const brc_panel*);

/* bits of the status word */
#define BRC_PANEL_OUT_OF_RANGE   1u      /* some idx[j] lies outside [0, n_pos) */
#define BRC_PANEL_NOT_ASCENDING  2u      /* some idx[j] < idx[j - 1] */

/*
 * idx: n plane indices of the view, in memory of the view's kind (device memory of the view's device for the hip library, host memory
 * for the sim library) — element j of every destination plane is position view.pos0 + idx[j].  The list is NON-DECREASING; equal
 * neighbours are allowed (site lists repeat lines).
 * Destinations: CALLER-owned memory of the view's kind, with exactly the shapes and the meaning of brc_dense_expand's —
 *   ncol, depth [Lp][.]   unavail [.]   istat, fstat [Lp][6][9][.], [Lp][6][4][.]   metrics [Lp][6][13][.]
 * — planes dst_stride (>= n) elements apart, elements [n, dst_stride) of a plane not touched, any of them NULL (not wanted).  Element j
 * of every wanted plane is written with what brc_dense_expand(k0 = idx[j], n = 1) writes to its element 0: the two slots' buckets, then
 * the XAgg record of a bucket that has one (expand_slots, brc_host.cpp), and for `metrics` ONE correctly rounded fp32 division per
 * average.
 * An index outside [0, n_pos) reads nothing: its element is written as an EMPTY position (zeros; unavail 0xFFFFFFFF) and
 * BRC_PANEL_OUT_OF_RANGE is set.
 * A descent (idx[j] < idx[j - 1]) sets BRC_PANEL_NOT_ASCENDING; ncol / depth / unavail and every bucket WITHOUT an XAgg record are then
 * still exact, a bucket that has such a record holds either the slots' values or the record's (unspecified which: the records find
 * their elements by a binary search over idx).  Whatever the list holds, every store stays inside [0, n) of its plane.
 * status: NULL, or ONE word in memory of the view's kind.  The library clears it on the stream before its launches, the kernels OR the
 * bits above into it (an ordinary atomic), the host never reads it: a caller that wants to know reads it behind the work.
 * stream: a hipStream_t, or NULL for the default stream (ignored by the sim library).  The hip library returns once its work is
 * enqueued on it — the status word's clear, the planes, then one lane per XAgg record — it never waits and allocates nothing: work queued
 * on that stream afterwards sees the result.  The view must stay valid (include/brc.h) until that work has run.
 * BRC_E_ARG, and nothing is written: a NULL handle or view, a NULL idx with n > 0, n < 0, dst_stride < n, a view whose `memory` is not
 * this library's (BRC_MEM_DEVICE for hip, BRC_MEM_HOST for sim) or that lies on another device than the handle's, a view without its
 * planes, n above 2^31 - 1 workgroups of 256 lanes (one launch).  n == 0 is BRC_OK (a status word is cleared).
 */
int  brc_panel_gather(brc_panel*, const brc_device_view*,
                      const int32_t* idx, int64_t n, int64_t dst_stride,
                      uint32_t* ncol, uint32_t* depth, uint32_t* unavail,          /* [Lp][.], [Lp][.], [.] */
                      uint32_t* istat, float* fstat, float* metrics,               /* [Lp][6][9][.], [Lp][6][4][.], [Lp][6][13][.] */
                      uint32_t* status, void* stream);

/* The last brc_panel_gather's account: seconds between the HIP events around its launches (hip: WAITS for the second event; sim: wall
 * time), the bytes its planes kernel asks for and writes (4 per listed word: an isolated site costs a cache line per word on top of
 * that, which the host cannot know; the XAgg launch adds 64 bytes read per record and a binary search over idx: counted as read).
 * (tools/panel_bench.py) */
void brc_panel_last_timing(const brc_panel*, double* kernel_s, uint64_t* bytes_read, uint64_t* bytes_written);

#ifdef __cplusplus
}
#endif
#endif
