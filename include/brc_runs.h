/* brc_runs.h — C-ABI of the device-side DEPTH-CLASS INTERVALS: the maximal stretches of a computed region (brc_device_view, and the
 * reference slice of brc_device_indels, include/brc.h) over which coverage stays in one class — callable in every library, below 10x in
 * the normal, no coverage, too deep to trust, reference is N — as an ascending list of intervals [start, end) of plane indices with a
 * class word per interval, and the number of positions per class, IN THE MEMORY THE VIEW LIVES IN.  The starts and ends are what
 * brc_bins_reduce (include/brc_bins.h) takes as an edge list and what masks a list of brc_select_sites (include/brc_select.h).
 *
 * A library of its own (libbrc_runs_hip.so: the gfx950 kernels of bam_readcount_amd/csrc/brc_runs.hip; tests/sim_runs/
 * libbrc_runs_sim.so: the same per-lane functions, brc_runs_core.h, run lane for lane on host memory) with a handle of its own.
 * It links nothing of the engine: the views are plain data.  Error codes are the BRC_E_* of include/brc.h.
 *
 * What it stands in for: the reference prints every position and leaves intervals to whoever reads its text (bamreadcount.cpp:351-416);
 * a GPU consumer had to expand the whole region (brc_dense_expand: 312 bytes per position and library) and run min / bucketize / diff /
 * nonzero over it.  The intervals need ONE word per position and library (depth) and the reference byte. */
#ifndef BRC_RUNS_H
#define BRC_RUNS_H

#include "brc.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct brc_runs brc_runs;

/* One handle per device (hip: BRC_E_NODEVICE without a GPU — the product library has no CPU path; sim: host views carry device 0).
 * The handle owns two timing events and nothing else: sources are the views', scratch and destinations the caller's. */
int  brc_runs_create(int device, brc_runs** out);
void brc_runs_destroy(brc_runs*);
const char* brc_runs_kind(void);                           /* "hip-gfx950" | "sim" */
const char* brc_runs_last_error(const brc_runs*);

#define BRC_RUNS_MAX_LIB 254            /* libraries of a view the library takes: the roles travel in the kernel arguments */
#define BRC_RUNS_MAX_CUT 15             /* cuts of a call: classes 0 .. 15, and 16 for "no reference base" */
/* brc_runs_params.combine: what V(k) is over the counted libraries */
#define BRC_RUNS_MIN 0
#define BRC_RUNS_MAX 1
#define BRC_RUNS_SUM 2
/* brc_runs_params.flags */
#define BRC_RUNS_REF_N 1u               /* a position whose reference character is none of ACGTacgt gets class n_cut + 1 */

typedef struct brc_runs_params {
    const uint8_t* role;    /* HOST memory, view->n_lib entries: 0 the library is ignored, 1 it is counted; NULL = every library counts */
    uint32_t combine;       /* BRC_RUNS_MIN | BRC_RUNS_MAX | BRC_RUNS_SUM */
    uint32_t n_cut;         /* 1 .. BRC_RUNS_MAX_CUT */
    uint32_t cut[BRC_RUNS_MAX_CUT];     /* strictly ascending; elements at and behind n_cut are not read */
    uint32_t keep;          /* bit c set: runs of class c are written */
    uint32_t flags;         /* 0 | BRC_RUNS_REF_N */
} brc_runs_params;

/* Bytes of scratch a call over n positions needs (a function of n alone; 0 for n <= 0).  The scratch is the caller's, of the view's
 * kind of memory, 4-byte aligned; its contents before and after a call mean nothing. */
int64_t brc_runs_workspace(int64_t n);

/*
 * THE DEFINITION is pure integer arithmetic, stated on the dense result (brc_result).  For plane index k in [k0, k0 + n):
 *   V(k)     = the minimum, the maximum or the sum (in 64 bits) of depth[l][k] over the counted libraries l.  An EMPTY position of a
 *              site-list axis (brc_region_windows) has depth 0.
 *   class(k) = the number of cut[i] <= V(k), i < n_cut: 0 .. n_cut.
 *              With BRC_RUNS_REF_N: n_cut + 1 instead when the reference character R of position pos0 + k is none of "ACGTacgt" — R from
 *              brc_device_indels.ref / ref_lo / ref_hi / ref_len by brc_select.h's rule: outside the slice, at or past ref_len, a NUL
 *              character or no reference => 'N'.
 * A RUN is a maximal [s, e) inside the window over which class is constant: the runs tile the window.  The runs whose class bit is set
 * in `keep` are the EMITTED runs, in ascending order.
 *
 * Destinations: CALLER-owned memory of the view's kind, any of them NULL (not wanted):
 *   counts    [1]           the number of emitted runs of the window: the true total whatever cap is
 *   start     [cap]         for j < min(total, cap): the first plane index of emitted run j (k0 <= start[j])
 *   end       [cap]         for j < min(total, cap): the plane index behind its last one (start[j] < end[j] <= k0 + n; end[j] <= start[j + 1])
 *   cls       [cap]         for j < min(total, cap): its class
 *   per_class [n_cut + 2]   uint64_t, 8-byte aligned: the number of window positions of each class, whatever `keep` is; their sum is n
 *                           (element n_cut + 1 is 0 without BRC_RUNS_REF_N)
 * Nothing at or behind index min(total, cap) of start / end / cls is touched.  So a caller asks for `counts` alone, reads it — the one
 * host synchronisation — allocates exactly and calls again; start / end interleaved are an edge list of brc_bins_reduce.
 * workspace: brc_runs_workspace(n) bytes of the caller's, of the view's kind.
 * indels: the view that carries the reference slice.  It may be NULL when BRC_RUNS_REF_N is not set (nothing of it is read then); if it
 * is given, it must agree with the view as brc_select_sites demands.
 * stream: a hipStream_t, or NULL for the default stream (ignored by the sim library).  The hip library returns once its work is
 * enqueued on it and never waits; it allocates nothing; no kernel waits for another workgroup.  The result is a pure function of the
 * views, the window and the parameters: two calls give identical bytes (the atomics inside only add integers).
 * The views must stay valid (include/brc.h) until that work has run; params and role are read before the call returns.
 * BRC_E_ARG, and nothing is written: a NULL handle, view or params; what brc_select_sites refuses about its views and the window
 * (k0 < 0, n < 0, k0 + n > n_pos, a view without planes, records without their arrays, memory that is not this library's —
 * BRC_MEM_DEVICE for hip, BRC_MEM_HOST for sim — or of another device than the handle's; an indels view that disagrees with the view in
 * memory / device / n_lib / pos0 / n_pos); k0 + n > 2^31 - 1 (start and end have 32 bits); more than BRC_RUNS_MAX_LIB libraries; a role
 * above 1; no counted library; an unknown combine; unknown flags; n_cut outside 1 .. BRC_RUNS_MAX_CUT; cuts that are not strictly
 * ascending; keep == 0 or with a bit above n_cut + 1; BRC_RUNS_REF_N with a NULL indels view; cap < 0; a NULL workspace with n > 0.
 * n == 0 is BRC_OK: counts[0] = 0 and per_class is all zero.
 */
int  brc_runs_find(brc_runs*, const brc_device_view*, const brc_device_indels*, const brc_runs_params*, int64_t k0, int64_t n, int64_t cap,
                   int32_t* start, int32_t* end, uint32_t* cls, uint32_t* counts, uint64_t* per_class, void* workspace, void* stream);

/* The last brc_runs_find's account: seconds between the HIP events around its launches (hip: WAITS for the second event; sim: wall
 * time); the bytes its sweeps ask for — one word per position and counted library, the reference byte with BRC_RUNS_REF_N, the class
 * words read back for the list — and the scratch bytes it writes (what the host knows without the count: the list itself is not
 * counted).  (tools/runs_bench.py) */
void brc_runs_last_timing(const brc_runs*, double* kernel_s, uint64_t* bytes_read, uint64_t* bytes_written);

#ifdef __cplusplus
}
#endif
#endif
