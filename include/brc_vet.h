/* brc_vet.h — C-ABI of the device-side CANDIDATE FILTER: for a list of plane positions of a computed region (brc_device_view +
 * brc_device_indels, include/brc.h) and the bases asked about at each, the per-allele read-metric tests that false-positive filters
 * run on bam-readcount's thirteen columns — variant bucket against reference bucket of the same site, test by test — as one failure
 * word per (library, base, element), a keep mask per element and the numbers the tests compared, IN THE MEMORY THE VIEWS LIVE IN.
 * The list and the masks are what brc_select_sites (include/brc_select.h) writes; the elements it keeps are what brc_panel_gather
 * (include/brc_panel.h) takes: region -> select -> vet -> panel runs with no host in it.
 *
 * A library of its own (libbrc_vet_hip.so: the gfx950 kernels of bam_readcount_amd/csrc/brc_vet.hip; tests/sim_vet/
 * libbrc_vet_sim.so: the same per-lane functions, brc_vet_core.h, run lane for lane on host memory) with a handle of its own.
 * It links nothing of the engine: the views are plain data.  Error codes are the BRC_E_* of include/brc.h; the columns named below are
 * the BRC_M_* of include/brc_dense.h.
 *
 * What it stands in for: the reference prints the thirteen columns of every (position, base) and leaves the filter to whoever reads
 * its text (bamreadcount.cpp:351-416, operator<<(BasicStat), BasicStat.cpp:110-159); a GPU consumer had to gather six buckets x 13
 * columns per candidate and library (brc_panel_gather: 312 bytes written, four of the six buckets zero) and find the reference's and the
 * variant's bucket again with a dozen array operations.  The filter reads the compact planes once: depth, slotid and the two slots. */
#ifndef BRC_VET_H
#define BRC_VET_H

#include "brc_select.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct brc_vet brc_vet;

/* One handle per device (hip: BRC_E_NODEVICE without a GPU — the product library has no CPU path; sim: host views carry device 0).
 * The handle owns two timing events and nothing else: sources are the views', the lists, scratch and destinations the caller's. */
int  brc_vet_create(int device, brc_vet** out);
void brc_vet_destroy(brc_vet*);
const char* brc_vet_kind(void);                            /* "hip-gfx950" | "sim" */
const char* brc_vet_last_error(const brc_vet*);

#define BRC_VET_MAX_LIB 254             /* libraries of a view the filter takes: lib_on travels in the kernel arguments */
/* bits of a failure word, and of brc_vet_params.tests: one per test */
#define BRC_VET_DEPTH          1u
#define BRC_VET_VAR_COUNT      2u
#define BRC_VET_VAR_FREQ       4u
#define BRC_VET_STRAND         8u
#define BRC_VET_VAR_READPOS   16u
#define BRC_VET_VAR_DIST3     32u
#define BRC_VET_VAR_BQ        64u
#define BRC_VET_VAR_MAPQ     128u
#define BRC_VET_VAR_MMQS     256u
#define BRC_VET_VAR_RL       512u
#define BRC_VET_REF_READPOS 1024u
#define BRC_VET_REF_DIST3   2048u
#define BRC_VET_REF_BQ      4096u
#define BRC_VET_REF_MAPQ    8192u
#define BRC_VET_REF_RL     16384u
#define BRC_VET_MMQS_DIFF  32768u
#define BRC_VET_MAPQ_DIFF  65536u
#define BRC_VET_RL_DIFF   131072u
#define BRC_VET_ALL_TESTS 262143u       /* the eighteen bits above */
/* bits of a failure word that no test sets: nothing was judged (never "pass" for keep) */
#define BRC_VET_NOT_ASKED 1073741824u   /* 1 << 30: the library is off, the base is not in alt[j], or it is the reference's base */
#define BRC_VET_NO_SITE   2147483648u   /* 1 << 31: the index lies outside the planes, or the reference character is none of ACGTacgt */
/* bits of the status word (brc_panel.h's, under this library's names) */
#define BRC_VET_OUT_OF_RANGE   1u       /* some idx[j] lies outside [0, n_pos) */
#define BRC_VET_NOT_ASCENDING  2u       /* some idx[j] < idx[j - 1] */
/* columns of `vals` */
#define BRC_VET_NVAL 20
#define BRC_VET_V_CV         0          /* C_v as fp32 */
#define BRC_VET_V_CR         1          /* C_r as fp32 */
#define BRC_VET_V_D          2          /* D as fp32 */
#define BRC_VET_V_FREQ       3          /* (float)C_v / (float)D, 0 when D == 0 */
#define BRC_VET_V_STRAND     4          /* (float)P_v / (float)(P_v + M_v), 0 when P_v + M_v == 0 */
#define BRC_VET_V_MMQS_DIFF  5          /* m_v[AVG_MMQ] - m_r[AVG_MMQ] */
#define BRC_VET_V_MAPQ_DIFF  6          /* m_r[AVG_MAPQ] - m_v[AVG_MAPQ] */
#define BRC_VET_V_RL_DIFF    7          /* m_r[AVG_CLIPPED] - m_v[AVG_CLIPPED] */
#define BRC_VET_V_VAR        8          /* m_v of AVG_POS, AVG_3P, AVG_BQ, AVG_MAPQ, AVG_MMQ, AVG_CLIPPED: columns 8 .. 13 */
#define BRC_VET_V_REF       14          /* m_r of the same six: columns 14 .. 19 */

/* Thresholds.  The defaults bam_readcount_amd.tensors.vet documents (in the spirit of the published false-positive filters over
 * bam-readcount output; no test of the project depends on them): min_depth 8, min_var_count 4, freq 1/20, min_strand_reads 5, strand
 * 1/100, min_ref_reads 2, min_var_readpos 0.1, min_var_dist3 0.1, min_var_bq 15, min_var_mapq 15, max_var_mmqs 100, min_var_rl 90,
 * min_ref_readpos 0.1, min_ref_dist3 0.1, min_ref_bq 15, min_ref_mapq 15, min_ref_rl 90, max_mmqs_diff 50, max_mapq_diff 50,
 * max_rl_diff 0.25. */
typedef struct brc_vet_params {
    const uint8_t* lib_on;  /* HOST memory, view->n_lib entries: 0 the library is not judged, 1 it is; NULL = every library is judged */
    uint32_t tests;         /* mask of BRC_VET_DEPTH .. BRC_VET_RL_DIFF: a test outside the mask never sets its bit */
    uint32_t min_depth, min_var_count, freq_num, freq_den, min_strand_reads, strand_num, strand_den, min_ref_reads;
    float min_var_readpos, min_var_dist3, min_var_bq, min_var_mapq, max_var_mmqs, min_var_rl;
    float min_ref_readpos, min_ref_dist3, min_ref_bq, min_ref_mapq, min_ref_rl;
    float max_mmqs_diff, max_mapq_diff, max_rl_diff;
} brc_vet_params;

/* Bytes of scratch a call over a list of n elements needs: 4 * (n + n_xagg) for a view with third-allele records (the records are
 * linked onto the elements that list their position), 0 for a view without, for n <= 0 or a NULL view.  The scratch is the caller's, of
 * the views' kind of memory, 4-byte aligned; its contents before and after a call mean nothing. */
int64_t brc_vet_workspace(const brc_device_view*, int64_t n);

/*
 * idx: n plane indices of the view, in memory of the views' kind, NON-DECREASING, with brc_panel_gather's rules: equal neighbours are
 * allowed; an index outside [0, n_pos) reads nothing, judges nothing (BRC_VET_NO_SITE) and sets BRC_VET_OUT_OF_RANGE in `status`; a
 * descent (idx[j] < idx[j - 1]) sets BRC_VET_NOT_ASCENDING — every bucket WITHOUT a third-allele record is then still judged exactly,
 * a bucket that has such a record is judged on either the slots' values or the record's (unspecified which: the records find their
 * elements by a binary search over idx).  Whatever the list holds, every store stays inside [0, n) of its plane.
 * alt: n masks of BRC_WHY_A | C | G | T (include/brc_select.h), the bases asked about at element j — what brc_select_sites writes to
 * `why`; BRC_WHY_INS, BRC_WHY_DEL and every higher bit are ignored (indel candidates are not judged here).  NULL = all four bases.
 *
 * THE PREDICATE, stated on the dense result (brc_result).  For element j with k = idx[j], library l and base v in A C G T:
 *   R   = the reference character of position pos0 + k from brc_device_indels.ref / ref_lo / ref_hi / ref_len by brc_select.h's rule
 *         (outside the slice, at or past ref_len, a NUL character or no reference => 'N'); "acgt" count as "ACGT"; r = R's bucket
 *   fail[l][v][j] = BRC_VET_NOT_ASKED  when lib_on[l] == 0;
 *                   BRC_VET_NO_SITE    otherwise, when k is outside [0, n_pos) or R is none of "ACGTacgt";
 *                   BRC_VET_NOT_ASKED  otherwise, when v is not in alt[j] or v == r;
 *                   otherwise the OR of the tests below that are in `tests` and set.
 *   For a bucket x (buckets 1..4 of "=ACGTN"): i_x[9], f_x[4] are istat[l][x][.][k], fstat[l][x][.][k]: the slot-0, slot-1 or XAgg values
 *   with expand_slots' precedence (zero; slot 0; slot 1 — integers where non-zero, floats unconditionally; then the XAgg record).
 *   C_x = i_x[BRC_I_N], P_x = i_x[BRC_I_PLUS], M_x = i_x[BRC_I_MINUS], D = depth[l][k]; m_x = the thirteen columns of the bucket as
 *   include/brc_dense.h defines them: all 0 when C_x == 0, else every average ONE fp32 division fl((float)sum / (float)C_x) (float
 *   sums: fl(sum / (float)C_x)), conversions uint32 -> fp32 round to nearest even.
 *   Integer tests: every operand widened to uint64 first, sums and products in uint64 arithmetic (modulo 2^64, which only strand_num * S
 *   with S >= 2^32 can reach):
 *     DEPTH        D < min_depth
 *     VAR_COUNT    C_v < min_var_count
 *     VAR_FREQ     C_v * freq_den < freq_num * D
 *     STRAND       S = P_v + M_v;  S >= min_strand_reads  and  min(P_v, M_v) * strand_den < strand_num * S
 *   fp32 tests on the variant side, judged only when C_v > 0 (a comparison with a NaN is false: the bit stays clear):
 *     VAR_READPOS  m_v[AVG_POS] < min_var_readpos        VAR_DIST3  m_v[AVG_3P] < min_var_dist3       VAR_BQ  m_v[AVG_BQ] < min_var_bq
 *     VAR_MAPQ     m_v[AVG_MAPQ] < min_var_mapq          VAR_MMQS   m_v[AVG_MMQ] > max_var_mmqs       VAR_RL  m_v[AVG_CLIPPED] < min_var_rl
 *   fp32 tests on the reference side, judged only when C_r >= min_ref_reads:
 *     REF_READPOS  m_r[AVG_POS] < min_ref_readpos        REF_DIST3  m_r[AVG_3P] < min_ref_dist3       REF_BQ  m_r[AVG_BQ] < min_ref_bq
 *     REF_MAPQ     m_r[AVG_MAPQ] < min_ref_mapq          REF_RL     m_r[AVG_CLIPPED] < min_ref_rl
 *   Difference tests, judged only when both sides are judged (C_v > 0 and C_r >= min_ref_reads); fl() is ONE IEEE fp32 operation,
 *   rounded to nearest even, never fused with the next:
 *     MMQS_DIFF    fl(m_v[AVG_MMQ] - m_r[AVG_MMQ]) > max_mmqs_diff
 *     MAPQ_DIFF    fl(m_r[AVG_MAPQ] - m_v[AVG_MAPQ]) > max_mapq_diff
 *     RL_DIFF      fl(m_r[AVG_CLIPPED] - m_v[AVG_CLIPPED]) > fl(max_rl_diff * m_r[AVG_CLIPPED])
 *   numpy float32 / uint64 arrays reproduce every one of them bit for bit.
 *   keep[j] = the OR of BRC_WHY_<v> over the bases v with fail[l][v][j] == 0 in SOME library l.
 *   vals[l][v][c][j], c = BRC_VET_V_*: whatever `tests` and the "judged only when" conditions say, from the same i_x, f_x, m_x —
 *   (float)C_v, (float)C_r, (float)D, fl((float)C_v / (float)D) (0 when D == 0), fl((float)P_v / (float)S) with S converted from its
 *   64-bit sum (0 when S == 0), the three differences' left-hand sides, m_v and m_r of the six tested columns; all zero where fail is
 *   BRC_VET_NOT_ASKED or BRC_VET_NO_SITE.
 *
 * Destinations: CALLER-owned memory of the views' kind, planes dst_stride (>= n) elements apart, elements [n, dst_stride) of a plane
 * not touched, any of them NULL (not wanted):
 *   fail [Lp][4][.]   keep [.]   vals [Lp][4][BRC_VET_NVAL][.]
 * status: NULL, or ONE word in memory of the views' kind.  The library clears it on the stream before its launches, the kernels OR the
 * bits above into it, the host never reads it.
 * workspace: brc_vet_workspace(view, n) bytes of the caller's, of the views' kind.  It must be given with n > 0 even where that is 0
 * bytes (it is not dereferenced then): one rule for every view.
 * stream: a hipStream_t, or NULL for the default stream (ignored by the sim library).  The hip library returns once its work is
 * enqueued on it and never waits; it allocates nothing; no kernel waits for another workgroup.  The result is a pure function of the
 * views, the lists and the parameters: two calls give identical bytes (the atomics inside only link records and OR status bits).
 * Both views must stay valid (include/brc.h) until that work has run; params and lib_on are read before the call returns.
 * BRC_E_ARG, and nothing is written: a NULL handle, view, indels view or params; what brc_panel_gather and brc_select_sites refuse about
 * their views, the list and dst_stride (a NULL idx with n > 0, n < 0, dst_stride < n, a view without planes, records without their
 * arrays, the two views disagreeing in memory / device / n_lib / pos0 / n_pos, memory that is not this library's — BRC_MEM_DEVICE for
 * hip, BRC_MEM_HOST for sim — or of another device than the handle's, a list or record table too large for 32-bit indices); more than
 * BRC_VET_MAX_LIB libraries; a lib_on entry above 1; no judged library; freq_den == 0 or strand_den == 0; bits in `tests` outside
 * BRC_VET_ALL_TESTS; a threshold that is not finite; a NULL workspace with n > 0.
 * n == 0 is BRC_OK (a status word is cleared).
 */
int  brc_vet_sites(brc_vet*, const brc_device_view*, const brc_device_indels*, const brc_vet_params*,
                   const int32_t* idx, const uint32_t* alt, int64_t n, int64_t dst_stride,
                   uint32_t* fail, uint32_t* keep, float* vals,
                   uint32_t* status, void* workspace, void* stream);

/* The last brc_vet_sites's account: seconds between the HIP events around its launches (hip: WAITS for the second event; sim: wall
 * time); the bytes its kernels ask for — the list words, the reference byte, 28 words per element and judged library, the head word
 * and 64 bytes per third-allele record where the view has any — and the bytes it writes (destinations and scratch; an isolated site
 * costs a cache line per word read on top of that, which the host cannot know).  (tools/vet_bench.py) */
void brc_vet_last_timing(const brc_vet*, double* kernel_s, uint64_t* bytes_read, uint64_t* bytes_written);

#ifdef __cplusplus
}
#endif
#endif
