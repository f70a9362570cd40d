/* brc_bins.h — C-ABI of the device-side WINDOW SUMMARIES: a computed region (brc_device_view + brc_device_indels, include/brc.h)
 * reduced over bins of its positions — per bin and library the sums of depth, covered columns and the six buckets' read counts, the
 * non-reference reads, the insertion and deletion reads, the deepest position, the positions at or above up to eight depth thresholds —
 * and a depth histogram per library, IN THE MEMORY THE VIEWS LIVE IN.  Exact integer arithmetic in 64 bits: means, fractions and
 * log-ratios are the caller's divisions.
 *
 * A library of its own (libbrc_bins_hip.so: the gfx950 kernels of bam_readcount_amd/csrc/brc_bins.hip; tests/sim_bins/
 * libbrc_bins_sim.so: the same per-lane functions, brc_bins_core.h, run lane for lane on host memory) with a handle of its own.
 * It links nothing of the engine: the views are plain data.  Error codes are the BRC_E_* of include/brc.h.
 *
 * What it stands in for: the reference prints every position and leaves any summary to whoever reads its text (bamreadcount.cpp:351-416);
 * a GPU consumer had to expand the whole region (brc_dense_expand: 312 bytes per position and library) and reduce that.  The reduction
 * reads the compact planes once: ncol, depth, slotid and the two slots' read counts, and the reference byte. */
#ifndef BRC_BINS_H
#define BRC_BINS_H

#include "brc.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct brc_bins brc_bins;

/* One handle per device (hip: BRC_E_NODEVICE without a GPU — the product library has no CPU path; sim: host views carry device 0).
 * The handle owns two timing events and nothing else: sources are the views', destinations the caller's; there is no scratch. */
int  brc_bins_create(int device, brc_bins** out);
void brc_bins_destroy(brc_bins*);
const char* brc_bins_kind(void);                           /* "hip-gfx950" | "sim" */
const char* brc_bins_last_error(const brc_bins*);

#define BRC_BINS_NSUM     12            /* values of `sums` per bin and library */
#define BRC_BINS_MAX_THR  8             /* depth thresholds of `covered` */
#define BRC_BINS_MAX_HIST 4096          /* bars of `hist` */
#define BRC_BINS_MAX_LIB  65535         /* libraries of a view the reduction takes */
/* index into sums[l][.][bin] */
#define BRC_BINS_S_DEPTH    0           /* sum of depth */
#define BRC_BINS_S_NCOL     1           /* sum of ncol */
#define BRC_BINS_S_BUCKET   2           /* 2..7: sum of istat[l][b][BRC_I_N] for the six buckets "=ACGTN" */
#define BRC_BINS_S_NONREF   8           /* reads of A C G T other than the reference base's */
#define BRC_BINS_S_INS      9           /* reads of the insertion records of the bin */
#define BRC_BINS_S_DEL     10           /* reads of the deletion records of the bin */
#define BRC_BINS_S_MAXDEPTH 11          /* the largest depth */
/* bits of the status word */
#define BRC_BINS_DESCENDS 1u            /* some edges[b + 1] < edges[b] */
#define BRC_BINS_OUTSIDE  2u            /* an edge below k0 or above k0 + n: it counts as k0 resp. k0 + n */

typedef struct brc_bins_params {
    const int32_t* edges;   /* an edge list: n_bins + 1 plane indices IN THE VIEWS' KIND OF MEMORY (the host never reads them); NULL: uniform bins */
    int64_t width;          /* uniform bins: positions per bin (> 0); 0 with an edge list */
    int64_t n_bins;         /* bins of the edge list; not read for uniform bins, whose number is ceil(n / width) */
    int32_t n_thr;          /* 0 .. BRC_BINS_MAX_THR thresholds of `covered` */
    int32_t n_hist;         /* 0 (no histogram) or 1 .. BRC_BINS_MAX_HIST bars */
    uint32_t thr[BRC_BINS_MAX_THR];
} brc_bins_params;

/*
 * THE BINS of the window [k0, k0 + n) of the planes:
 *   uniform   (width > 0, edges == NULL): bin b = [k0 + b * width, min(k0 + (b + 1) * width, k0 + n)), n_bins = ceil(n / width).
 *   edge list (width == 0, edges != NULL): plane index k of the window lies in bin b = the number of edges[1 .. n_bins] that are <= k,
 *             provided edges[0] <= k < edges[n_bins]; every other k lies in no bin.  Equal neighbouring edges make an empty bin, whose
 *             outputs are all zero.  An edge below k0 or above k0 + n counts as k0 resp. k0 + n (positions outside the window lie in
 *             no bin) and sets BRC_BINS_OUTSIDE.  A list that descends somewhere sets BRC_BINS_DESCENDS; the bin of a position is
 *             then what a binary search over the list finds — some bin of the list or none: no store leaves its destination.
 * THE VALUES are stated on the dense result (brc_result); an EMPTY position of a site-list axis (brc_region_windows) is a position of
 * depth 0 without counts.  For bin b and library l, over the positions k of the bin:
 *   sums[l][0][b]       sum of depth[l][k]
 *   sums[l][1][b]       sum of ncol[l][k]
 *   sums[l][2 + c][b]   sum of istat[l][c][BRC_I_N][k] for bucket c of "=ACGTN": a third-allele record's count takes the place of the
 *                       slots' (what brc_dense_expand writes)
 *   sums[l][8][b]       sum of the A C G T counts other than the reference base's, over the positions whose reference character R is one
 *                       of "ACGTacgt" — R by brc_select.h's rule: outside the slice, at or past ref_len, NUL or no reference => 'N';
 *                       any other character contributes 0
 *   sums[l][9][b]       sum of i[BRC_I_N] over the live records (len != 0) of brc_device_indels.slots with lib == l, len > 0 and
 *                       pos - pos0 in the bin
 *   sums[l][10][b]      the same with len < 0
 *   sums[l][11][b]      the largest depth[l][k] (0 for an empty bin)
 *   covered[l][t][b]    the number of positions with depth[l][k] >= thr[t], t < n_thr (thr[t] == 0 counts every position of the bin)
 *   hist[l][d]          the number of positions of the window that lie in SOME bin and have min(depth[l][k], n_hist - 1) == d
 *
 * Destinations: CALLER-owned memory of the views' kind, any of them NULL (not wanted), 8-byte aligned, uint64_t all:
 *   sums    [n_lib][BRC_BINS_NSUM][dst_stride]
 *   covered [n_lib][n_thr][dst_stride]
 *   hist    [n_lib][n_hist]
 *   status  [1]  uint32_t: cleared on the stream, then ORed by the kernels with BRC_BINS_* (always 0 for uniform bins)
 * Elements at or behind n_bins of a row (the padding up to dst_stride) are never touched.
 * stream: a hipStream_t, or NULL for the default stream (ignored by the sim library).  The hip library returns once its work is
 * enqueued on it and never waits; it allocates nothing and needs no scratch; no kernel waits for another workgroup.  The result is a
 * pure function of the views, the window and the parameters: two calls give identical bytes (the atomics inside add and take the
 * maximum of integers, and OR status bits: their order changes nothing).
 * Both views and the edge list must stay valid (include/brc.h) until that work has run; params is read before the call returns.
 * BRC_E_ARG, and nothing is written: a NULL handle, view, indels view or params; what brc_select_sites refuses about its views and the
 * window (k0 < 0, n < 0, k0 + n > n_pos, a view without planes, records without their arrays, memory that is not this library's —
 * BRC_MEM_DEVICE for hip, BRC_MEM_HOST for sim — or of another device than the handle's, the two views disagreeing in memory / device /
 * n_lib / pos0 / n_pos, k0 + n > 2^31 - 1: edges and a third-allele record's k have 32 bits); more than BRC_BINS_MAX_LIB libraries;
 * width < 0; width == 0 without edges; width > 0 with edges; n_bins < 0 or above 2^31 - 2; n_thr < 0 or > BRC_BINS_MAX_THR;
 * n_hist < 0 or > BRC_BINS_MAX_HIST; dst_stride < n_bins.
 * n == 0 or n_bins == 0 is BRC_OK: no position lies in a bin — every bin there is is empty (all zero), hist is all zero, and the status
 * word tells about the edge list as usual.
 */
int  brc_bins_reduce(brc_bins*, const brc_device_view*, const brc_device_indels*, const brc_bins_params*, int64_t k0, int64_t n,
                     uint64_t* sums, uint64_t* covered, uint64_t* hist, int64_t dst_stride, uint32_t* status, void* stream);

/* The last brc_bins_reduce's account: seconds between the HIP events around its launches (hip: WAITS for the second event; sim: wall
 * time); the bytes its sweeps ask for — up to five words per position and library and the reference byte, 64 bytes per third-allele
 * record, 72 per indel record, the edge list once — and the destination bytes it clears.  (tools/bins_bench.py) */
void brc_bins_last_timing(const brc_bins*, double* kernel_s, uint64_t* bytes_read, uint64_t* bytes_written);

#ifdef __cplusplus
}
#endif
#endif
