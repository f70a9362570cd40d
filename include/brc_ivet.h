/* brc_ivet.h — C-ABI of the device-side INDEL CANDIDATE FILTER: for every record of a sorted indel table of a computed region (what
 * brc_indels_gather, include/brc_indels.h, writes), the read-metric tests of include/brc_vet.h — the record's own sums against the
 * reference base's bucket at the record's pileup position — and an ALLELE-AWARE control veto: the record against the control libraries'
 * records of the same position, the same length and the same text.  One failure word per record, the numbers the tests compared, the
 * largest matching control count, and a keep mask per element of an optional site list, IN THE MEMORY THE VIEWS LIVE IN.  The list
 * and its reason words are what brc_select_sites (include/brc_select.h) writes: region -> select -> indel table -> ivet -> panel runs
 * with no host in it.
 *
 * A library of its own (libbrc_ivet_hip.so: the gfx950 kernels of bam_readcount_amd/csrc/brc_ivet.hip; tests/sim_ivet/
 * libbrc_ivet_sim.so: the same per-lane functions, brc_ivet_core.h, run lane for lane on host memory) with a handle of its own.
 * It links nothing of the engine or of its siblings: views and tables are plain data.  Error codes are the BRC_E_* of include/brc.h;
 * the test bits, the twenty columns of `vals` and the roles are those of brc_vet.h and brc_select.h.
 *
 * What it stands in for: brc_select_sites' control veto does not compare allele text, and brc_vet_sites does not judge indel
 * candidates; a GPU consumer gathered the table, six buckets x 13 columns at every record's position, found the reference's bucket
 * again and matched case against control records by text in a dozen array operations, or on the host. */
#ifndef BRC_IVET_H
#define BRC_IVET_H

#include "brc_vet.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct brc_ivet brc_ivet;

/* One handle per device (hip: BRC_E_NODEVICE without a GPU — the product library has no CPU path; sim: host views carry device 0).
 * The handle owns two timing events and nothing else: sources are the views' and the table's, scratch and destinations the caller's. */
int  brc_ivet_create(int device, brc_ivet** out);
void brc_ivet_destroy(brc_ivet*);
const char* brc_ivet_kind(void);                           /* "hip-gfx950" | "sim" */
const char* brc_ivet_last_error(const brc_ivet*);

#define BRC_IVET_MAX_LIB 254            /* libraries of a view the filter takes: the roles travel in the kernel arguments */
/* bits of a failure word and of brc_ivet_params.tests: the BRC_VET_* tests of brc_vet.h other than BRC_VET_VAR_BQ, and */
#define BRC_IVET_CTL_DEPTH    262144u   /* 1 << 18 */
#define BRC_IVET_CTL_ALLELE   524288u   /* 1 << 19 */
#define BRC_IVET_ALL_TESTS   1048511u   /* (BRC_VET_ALL_TESTS & ~BRC_VET_VAR_BQ) | CTL_DEPTH | CTL_ALLELE */
/* bits of a failure word that no test sets (brc_vet.h's values) */
#define BRC_IVET_NOT_ASKED 1073741824u  /* 1 << 30 */
#define BRC_IVET_NO_SITE   2147483648u  /* 1 << 31 */
/* bits of the status word */
#define BRC_IVET_LIST_OUT_OF_RANGE    1u   /* some idx[j] lies outside [0, n_pos) */
#define BRC_IVET_LIST_NOT_ASCENDING   2u   /* some idx[j] < idx[j - 1] */
#define BRC_IVET_TABLE_OUT_OF_RANGE   4u   /* some record with len != 0 has a position outside the planes or a library outside [0, n_lib) */
#define BRC_IVET_TABLE_NOT_ASCENDING  8u   /* some pos[r] < pos[r - 1] */
#define BRC_IVET_NVAL 20                /* columns of `vals`: BRC_VET_V_* */

/* The table brc_indels_gather writes, where it lies: CALLER-owned memory of the views' kind.  pos, lib, len [m]; istat [9][stride],
 * fstat [4][stride] (BRC_I_*, BRC_F_* planes `stride` >= m elements apart: brc_indels_gather's `cap`); allele_off [m + 1], alleles
 * [alleles_len].  allele_off and alleles may be NULL only when BRC_IVET_CTL_ALLELE is not in `tests`; nothing else of the table is
 * optional when m > 0. */
typedef struct brc_ivet_table {
    int64_t m, stride;
    const int32_t *pos, *lib, *len;
    const uint32_t* istat;
    const float* fstat;
    const uint32_t* allele_off;
    const uint8_t* alleles;
    int64_t alleles_len;
} brc_ivet_table;

/* Thresholds: brc_vet_params' (same names, same meaning) without min_var_bq — indel buckets carry no base-quality sum — and the
 * control test of brc_select_params under the record's count. */
typedef struct brc_ivet_params {
    const uint8_t* role;    /* HOST memory, view->n_lib entries of BRC_ROLE_IGNORE / CASE / CONTROL; NULL = every library is a case library */
    uint32_t tests;         /* mask of BRC_IVET_ALL_TESTS: a test outside the mask never sets its bit */
    uint32_t kinds;         /* mask of BRC_WHY_INS | BRC_WHY_DEL: the kinds of record that are judged */
    uint32_t min_depth, min_var_count, freq_num, freq_den, min_strand_reads, strand_num, strand_den, min_ref_reads;
    uint32_t ctl_min_depth, ctl_max_count, ctl_frac_num, ctl_frac_den;
    float min_var_readpos, min_var_dist3, min_var_mapq, max_var_mmqs, min_var_rl;
    float min_ref_readpos, min_ref_dist3, min_ref_bq, min_ref_mapq, min_ref_rl;
    float max_mmqs_diff, max_mapq_diff, max_rl_diff;
} brc_ivet_params;

/* Bytes of scratch a call over a table of m records needs: 4 * (m + n_xagg) for a view with third-allele records (the records are
 * linked onto the first table record of their position), 0 for a view without, for m <= 0 or a NULL view.  The scratch is the
 * caller's, of the views' kind of memory, 4-byte aligned; its contents before and after a call mean nothing. */
int64_t brc_ivet_workspace(const brc_device_view*, int64_t m);

/*
 * THE PREDICATE, stated on the dense result (brc_result) and the table.  For record r:
 *   p = pos[r], k = p - pos0, l = lib[r]; kind = BRC_WHY_INS when len[r] > 0, BRC_WHY_DEL when len[r] < 0
 *   fail[r] = the first rule that applies:
 *     BRC_IVET_NOT_ASKED  when len[r] == 0
 *     BRC_IVET_NO_SITE    when k is outside [0, n_pos) or l outside [0, n_lib); this sets BRC_IVET_TABLE_OUT_OF_RANGE in `status`
 *     BRC_IVET_NOT_ASKED  when role[l] != BRC_ROLE_CASE or the kind is not in `kinds`
 *     BRC_IVET_NO_SITE    when R, the reference character of position p by brc_select.h's rule (outside the slice, at or past ref_len,
 *                         a NUL character or no reference => 'N'), is none of "ACGTacgt"
 *     otherwise the OR of the tests below that are in `tests` and set.
 *   Variant side: the record's own sums i_v[9] = istat[.][r], f_v[4] = fstat[.][r]; C_v = i_v[BRC_I_N], P_v = i_v[BRC_I_PLUS], M_v =
 *     i_v[BRC_I_MINUS]; m_v = the thirteen columns of them as include/brc_dense.h defines them, EXCEPT m_v[AVG_BQ] = 0: indel buckets
 *     carry no base-quality sum (BasicStat.cpp:123), so VAR_BQ is not a test here and its column of `vals` is 0.
 *   Reference side: R's bucket r_b at (l, k) exactly as brc_vet.h defines a bucket: istat[l][r_b][.][k], fstat[l][r_b][.][k] — the
 *     slot-0, slot-1 or XAgg values with expand_slots' precedence —, C_r, m_r of them.  D = depth[l][k].
 *   The seventeen tests of brc_vet.h other than VAR_BQ, with its bit values, its "judged only when" conditions (the variant side when
 *     C_v > 0, the reference side when C_r >= min_ref_reads, the differences when both), its uint64 integer arithmetic and its
 *     single-rounding fp32 rules, unchanged: DEPTH, VAR_COUNT, VAR_FREQ, STRAND, VAR_READPOS, VAR_DIST3, VAR_MAPQ, VAR_MMQS, VAR_RL,
 *     REF_READPOS, REF_DIST3, REF_BQ, REF_MAPQ, REF_RL, MMQS_DIFF, MAPQ_DIFF, RL_DIFF.  (The library runs brc_vet_core.h's code.)
 *   BRC_IVET_CTL_DEPTH   some library c with role[c] == BRC_ROLE_CONTROL has depth[c][k] < ctl_min_depth
 *   BRC_IVET_CTL_ALLELE  some record r' other than r satisfies all of
 *       same run       r' lies in the RUN of r: the maximal stretch of consecutive table indices around r whose pos equals pos[r]
 *                      (whatever the table holds, sorted or not)
 *       control        lib[r'] lies in [0, n_lib) and role[lib[r']] == BRC_ROLE_CONTROL
 *       same allele    len[r'] == len[r] and text(r') == text(r) bytewise, where text(x) = alleles[min(allele_off[x], A) ..
 *                      min(allele_off[x + 1], A)) with A = alleles_len, empty when the second offset is below the first: no
 *                      content of allele_off makes a read leave `alleles`
 *       control fails  C' = istat[BRC_I_N][r'] fails  C' <= ctl_max_count && C' * ctl_frac_den <= ctl_frac_num * depth[lib[r']][k],
 *                      every operand widened to uint64 first
 *   ctl_count[r] = the largest C' over the records r' that satisfy the first three (0 when there is none, when the allele arrays are
 *     NULL, and wherever fail[r] is BRC_IVET_NOT_ASKED or BRC_IVET_NO_SITE); it does not depend on `tests`.
 *   vals[c][r], c = BRC_VET_V_* : brc_vet.h's twenty columns of the record, whatever `tests` and the "judged only when" conditions
 *     say; all zero where fail[r] is BRC_IVET_NOT_ASKED or BRC_IVET_NO_SITE.
 * On a table that is not sorted by position (BRC_IVET_TABLE_NOT_ASCENDING) a reference bucket that lives in a third-allele record is
 * judged on either the slots' values or that position's record's (unspecified which: the records find their run by a binary search over
 * pos, and a record takes a list only from a table record of its own position);
 * everything else stays exact, and every store stays in range.
 *
 * THE OPTIONAL LIST: idx [n] plane indices and why [n] reason words as brc_select_sites writes them (why NULL: every kind counts),
 * in memory of the views' kind.  keep[j] = the OR of the kind bits (BRC_WHY_INS / BRC_WHY_DEL) of the records r with pos[r] - pos0 ==
 * idx[j] and fail[r] == 0, restricted to the kinds in why[j].  Equal neighbours all receive it; an element without such a record is
 * 0; an element outside [0, n_pos) is 0 and sets BRC_IVET_LIST_OUT_OF_RANGE; idx[j] < idx[j - 1] sets BRC_IVET_LIST_NOT_ASCENDING
 * (the records find their elements by a binary search over idx: on a descending list an element may miss its bits, every store stays
 * inside [0, n)).  idx == NULL with n == 0 is the table-only call.
 *
 * Destinations: CALLER-owned memory of the views' kind, any of them NULL (not wanted):
 *   fail [m]   vals [BRC_IVET_NVAL][dst_stride] (planes dst_stride >= m elements apart, elements [m, dst_stride) not touched)
 *   ctl_count [m]   keep [n]
 * status: NULL, or ONE word in memory of the views' kind.  The library clears it — and keep — on the stream before its launches, the
 * kernels OR bits into them, the host never reads them.
 * workspace: brc_ivet_workspace(view, m) bytes of the caller's, of the views' kind; it must be given with m > 0 even where that is 0
 * bytes (it is not dereferenced then).
 * stream: a hipStream_t, or NULL for the default stream (ignored by the sim library).  The hip library returns once its work is
 * enqueued on it and never waits; it allocates nothing; no kernel waits for another workgroup.  The result is a pure function of the
 * views, the table, the list and the parameters: two calls give identical bytes (the atomics inside only link records and OR bits).
 * Views, table and list must stay valid until that work has run; params and role are read before the call returns.
 * BRC_E_ARG, and nothing is written: a NULL handle, view, indels view, params or table; everything brc_vet_sites refuses about its
 * views, its list and n; dst_stride < m; m < 0, stride < m, a table with m > 0 and a NULL pos, lib, len, istat or fstat; m or n too
 * large for 32-bit indices; alleles_len < 0; more than BRC_IVET_MAX_LIB libraries; kinds == 0 or with bits outside BRC_WHY_INS |
 * BRC_WHY_DEL; bits in `tests` outside BRC_IVET_ALL_TESTS (BRC_VET_VAR_BQ among them); freq_den, strand_den or ctl_frac_den == 0; a
 * role above 2; no case library; a threshold that is not finite; a NULL workspace with m > 0; a NULL allele_off or alleles with m > 0
 * and BRC_IVET_CTL_ALLELE in `tests`.
 * m == 0 and n == 0 is BRC_OK (a status word is cleared).
 */
int  brc_ivet_records(brc_ivet*, const brc_device_view*, const brc_device_indels*,
                      const brc_ivet_params*, const brc_ivet_table*,
                      const int32_t* idx, const uint32_t* why, int64_t n,
                      int64_t dst_stride,
                      uint32_t* fail, float* vals, uint32_t* ctl_count, uint32_t* keep,
                      uint32_t* status, void* workspace, void* stream);

/* The last brc_ivet_records's account: seconds between the HIP events around its launches (hip: WAITS for the second event; sim: wall
 * time); the bytes its kernels ask for that the host can count — per record four table words, the 13 sums, two offsets, 30 plane
 * words and the reference byte, per control library a depth word, the list words, 64 bytes per third-allele record where the view
 * has any (the text and the run's neighbours are data and are not counted) — and the bytes it writes (destinations and scratch).
 * (tools/ivet_bench.py) */
void brc_ivet_last_timing(const brc_ivet*, double* kernel_s, uint64_t* bytes_read, uint64_t* bytes_written);

#ifdef __cplusplus
}
#endif
#endif
