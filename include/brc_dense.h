/* brc_dense.h — C-ABI of the device-resident results: a computed region's compact planes (brc_device_view, include/brc.h) expanded
 * to the dense planes of brc_result, and to the thirteen columns the reference prints, IN THE MEMORY THE VIEW LIVES IN — nothing
 * crosses PCIe.
 *
 * A library of its own (libbrc_dense_hip.so: the gfx950 kernels of bam_readcount_amd/csrc/brc_dense.hip; tests/sim_dense/
 * libbrc_dense_sim.so: the same per-lane functions, brc_dense_core.h, run lane for lane on host memory) with a handle of its own.  It
 * links nothing of the engine: the view is plain data.  Error codes are the BRC_E_* of include/brc.h.
 *
 * What it stands in for: the reference has the BasicStat of every (position, library, base) in memory only while pileup_func prints
 * it (bamreadcount.cpp:351-416, operator<<(BasicStat), BasicStat.cpp:110-159); brc_fetch_result gives a caller the same numbers as
 * host arrays (expand_slots, brc_host.cpp); this gives them to a caller on the GPU.  Indel buckets are not covered here: include/brc_indels.h
 * gives them to the same kind of caller (brc_device_indels_get + brc_indels_gather). */
#ifndef BRC_DENSE_H
#define BRC_DENSE_H

#include "brc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* columns of `metrics`, in the order operator<<(BasicStat) prints them (BasicStat.cpp:117-140) */
#define BRC_NMETRIC 13
enum {
    BRC_M_COUNT = 0,       /* read_count */
    BRC_M_AVG_MAPQ,        /* sum_map_qualities / count */
    BRC_M_AVG_BQ,          /* sum_base_qualities / count */
    BRC_M_AVG_SE_MAPQ,     /* sum_single_ended_map_qualities / count */
    BRC_M_PLUS,            /* num_plus_strand */
    BRC_M_MINUS,           /* num_minus_strand */
    BRC_M_AVG_POS,         /* sum_event_location / count */
    BRC_M_AVG_NM,          /* sum_number_of_mismatches / count */
    BRC_M_AVG_MMQ,         /* sum_of_mismatch_qualities / count */
    BRC_M_NQ2,             /* num_q2_reads */
    BRC_M_AVG_Q2_DIST,     /* sum_q2_distance / num_q2_reads; 0 when there are none */
    BRC_M_AVG_CLIPPED,     /* sum_of_clipped_lengths / count */
    BRC_M_AVG_3P           /* sum_3p_distance / count */
};

typedef struct brc_dense brc_dense;

/* One handle per device (hip: BRC_E_NODEVICE without a GPU — the product library has no CPU path; sim: host views carry
 * device 0).  The
 * handle owns two timing events and nothing else: sources are the view's, destinations the caller's. */
int  brc_dense_create(int device, brc_dense** out);
void brc_dense_destroy(brc_dense*);
const char* brc_dense_kind(void);                         /* "hip-gfx950" | "sim" */
const char* brc_dense_last_error(const brc_dense*);

/*
 * Plane indices [k0, k0 + n) of the view -> CALLER-owned memory of the view's kind (device memory of the view's device for the hip
 * library, host memory for the sim library); element j of a destination plane is position view.pos0 + k0 + j, planes are dst_stride
 * (>= n) elements apart, elements [n, dst_stride) of a plane are not touched.  Any destination may be NULL (not wanted).
 *   ncol, depth   [Lp][.]          as brc_result
 *   unavail       [.]              as brc_result; 0xFFFFFFFF everywhere for an all-lib view (which has none)
 *   istat, fstat  [Lp][6][9][.], [Lp][6][4][.]   exactly brc_result.istat / fstat: every element of [0, n) of every plane is written — a
 *                 slot's integers land in the bucket slotid names where they are non-zero, its floats unconditionally, a bucket no
 *                 slot names is zero, and then every used XAgg record whose position lies in the window overwrites its bucket's 13 values
 *   metrics       [Lp][6][13][.]   BRC_M_*: what operator<<(BasicStat) prints for the bucket (as for a base: the base-quality column is
 *                 computed), as fp32.  Each average is (float)sum / (float)count, ONE correctly rounded fp32 division — the value the
 *                 reference hands to its "%.2f".  A bucket with count 0 is thirteen zeros.  The four integer columns (count, plus,
 *                 minus, q2 reads) are converted to float: exact below 2^24 reads in a bucket, rounded to nearest above.
 * stream: a hipStream_t, or NULL for the default stream (ignored by the sim library).  The hip library returns once its two launches
 * are enqueued on it — the planes, then one lane per XAgg record — and never waits: work queued on that stream afterwards sees the
 * result.  The view must stay valid (include/brc.h) until that work has run.
 * BRC_E_ARG, and nothing is written: a NULL handle or view, k0 < 0, n < 0, k0 + n > n_pos, dst_stride < n, a view whose `memory` is
 * not this library's (BRC_MEM_DEVICE for hip, BRC_MEM_HOST for sim) or that lies on another device than the handle's, a view without
 * its planes.  n == 0 is BRC_OK.
 */
int  brc_dense_expand(brc_dense*, const brc_device_view*, int64_t k0, int64_t n, int64_t dst_stride,
                      uint32_t* ncol, uint32_t* depth, uint32_t* unavail,          /* [Lp][.], [Lp][.], [.] */
                      uint32_t* istat, float* fstat,                               /* [Lp][6][9][.], [Lp][6][4][.] */
                      float* metrics,                                              /* [Lp][6][13][.] */
                      void* stream);

/* The last brc_dense_expand's account: seconds between the HIP events around its launches (hip: WAITS for the second event; sim: wall
 * time), the bytes its planes kernel reads and writes (the XAgg launch adds 64 bytes read per record and up to 104 written per used
 * one: counted as read, not as written — the host does not know how many are used).  (tools/dense_bench.py) */
void brc_dense_last_timing(const brc_dense*, double* kernel_s, uint64_t* bytes_read, uint64_t* bytes_written);

#ifdef __cplusplus
}
#endif
#endif
