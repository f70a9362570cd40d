/* brc_join.h — C-ABI of the device-side JOIN of computed regions: the views of K engines (brc_device_view / brc_device_indels of
 * include/brc.h — a tumour and its normal are two BAM files, hence two engines) COPIED into ONE view of the same kind over a window
 * the caller chooses, the libraries of source s renumbered behind those of the sources before it — IN THE MEMORY THE VIEWS LIVE IN.
 * The joined view is plain data in caller-owned buffers: every consumer of a view (include/brc_dense.h, brc_indels.h, brc_panel.h,
 * brc_select.h, brc_bins.h, brc_runs.h, brc_vet.h, brc_ivet.h, brc_inorm.h) takes it as it takes an engine's, and it stays valid when
 * the source engines begin another region or are destroyed.
 *
 * A library of its own (libbrc_join_hip.so: the gfx950 kernels of bam_readcount_amd/csrc/brc_join.hip; tests/sim_join/
 * libbrc_join_sim.so: the same per-lane functions, brc_join_core.h, run lane for lane on host memory) with a handle of its own.  It
 * links nothing of the engine or of its siblings.  Error codes are the BRC_E_* of include/brc.h.
 *
 * What it stands in for: interleaving both files' reads into one per-library engine, or expanding both regions densely and redoing
 * every filter in the caller's own code. */
#ifndef BRC_JOIN_H
#define BRC_JOIN_H

#include "brc.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct brc_join brc_join;

/* One handle per device (hip: BRC_E_NODEVICE without a GPU — the product library has no CPU path; sim: host views carry device 0).
 * The handle owns two timing events and nothing else: sources are the views', scratch and destinations the caller's. */
int  brc_join_create(int device, brc_join** out);
void brc_join_destroy(brc_join*);
const char* brc_join_kind(void);                           /* "hip-gfx950" | "sim" */
const char* brc_join_last_error(const brc_join*);

#define BRC_JOIN_MAX_SOURCES 16
#define BRC_JOIN_MAX_LIB     254        /* the joined libraries: what brc_select.h and brc_ivet.h take */
/* bits of the status word */
#define BRC_JOIN_REF_DIFFERS 1u         /* two sources hold different non-NUL reference characters at one position: the first won */

/* One source: the two views of one engine as brc_device_view_get / brc_device_indels_get return them.  indels may be NULL: the source
 * then has no indel records and no reference slice. */
typedef struct brc_join_source {
    const brc_device_view* view;
    const brc_device_indels* indels;
} brc_join_source;

/* The destination buffers: CALLER-owned memory of the views' kind, 4-byte aligned (seq_off: 8-byte), of the byte sizes brc_join_sizes
 * gives.  A buffer whose size is 0 may be NULL. */
typedef struct brc_join_dest {
    uint32_t *ncol, *depth, *slotid;    /* [L][stride] */
    uint32_t* si;                       /* [L][2][9][stride] */
    float* sf;                          /* [L][2][4][stride] */
    void* xagg;                         /* n_xagg records of 64 bytes */
    void* slots;                        /* n_slots records of 72 bytes */
    uint64_t* seq_off;                  /* [n_slots] */
    int32_t* l_qseq;                    /* [n_slots] */
    uint8_t* seq4;                      /* [seq_cap] */
    char* ref;                          /* [ref_hi - ref_lo] */
} brc_join_dest;

/* What the host knows of a join before it runs: the joined libraries, record counts, reference slice, and the bytes of every
 * destination buffer (a plane buffer of R rows ends behind element n_pos of its last row: ((R - 1) * stride + n_pos) * 4 bytes, 0 for
 * n_pos == 0).  The bytes of seq4 are data: counts[1] of a first call. */
typedef struct brc_join_sizes {
    int32_t n_lib, has_ref;
    uint64_t n_xagg, n_slots;
    int64_t ref_lo, ref_hi, ref_len;
    uint64_t ncol_bytes, depth_bytes, slotid_bytes, si_bytes, sf_bytes, xagg_bytes, slots_bytes, seq_off_bytes, l_qseq_bytes, ref_bytes;
    uint64_t workspace_bytes;
} brc_join_sizes;
/* BRC_E_ARG for what brc_join_views refuses of K, the sources and the window (the first nine refusals below); `out` is then zeroed. */
int  brc_join_sizes_of(int32_t K, const brc_join_source* sources, int32_t pos0, int64_t n_pos, int64_t stride, brc_join_sizes* out);
/* Bytes of scratch a join with n_slots joined indel records needs: a function of n_slots alone, 0 for 0.  The scratch is the caller's,
 * of the views' kind of memory, 4-byte aligned; its contents before and after a call mean nothing. */
size_t brc_join_workspace(uint64_t n_slots);

/*
 * THE DEFINITION.  Sources s = 0 .. K - 1; L_s = n_lib of source s, base_s = L_0 + .. + L_(s-1), L = base_K (an all-lib view is one
 * library).  The window is [pos0, pos0 + n_pos), planes `stride` >= n_pos elements apart.  d_s = pos0 - pos0_s.
 *
 * PLANES.  Joined library base_s + l is library l of source s.  Its 29 rows — ncol, depth, slotid, si [2][9], sf [2][4] — hold at
 * element k the source row's element k + d_s where 0 <= k + d_s < n_pos_s, as a bit pattern (a float sum is not touched: a NaN or a
 * -0.0 stays what it was); elsewhere the engine's own EMPTY position: 0, and the slot word 1 | 7 << 8 (what lane2_store of
 * brc_core.h writes for a position no read covers).  Every element of [0, n_pos) of every row is written exactly once; elements
 * [n_pos, stride) are not touched.  The joined view's unavail is NULL: a per-engine read index means nothing across engines
 * (brc_dense_expand yields 0xFFFFFFFF for such a view).
 *
 * THIRD-ALLELE RECORDS.  n_xagg = the sum of the sources' n_xagg; record j of source s is joined record xbase_s + j (xbase_s = the
 * sum before s).  The 16 words are copied; k becomes k + pos0_s - pos0 and the library in lib_b becomes base_s + library (the bucket
 * byte stays as it is, valid or not).  A record that is unused (k == 0xFFFFFFFF), whose k is not below n_pos_s, whose library is not
 * below L_s, or whose position leaves the window becomes UNUSED: k = 0xFFFFFFFF, the other 15 words as they were.  No consumer depends
 * on the order of these records: brc_dense_core.h / brc_panel_core.h overlay each used record on its own cell, brc_select_core.h and
 * brc_ivet_core.h link each to its position — a view holds at most one used record per (position, library, bucket), and the join keeps
 * that: libraries of different sources never meet.
 *
 * INDEL RECORDS.  n_slots = the sum of the sources' n_slots (a source without an indels view has none); record j of source s is
 * joined record r = sbase_s + j.  A record is KEPT when len != 0, its pos lies in the window AND in [pos0_s, pos0_s + n_pos_s), and
 * 0 <= lib < L_s.  pos, i[9], f[4] are copied; lib = lib + base_s and len = len for a kept record, lib as it was and len = 0 (unused)
 * otherwise; rep_read = r and rep_qpos = -1 always.
 *
 * WHAT SPELLS AN INSERTION.  A joined view cannot point into K engines' read arenas: the join writes one synthetic read per joined
 * record.  n_reads = n_slots; l_qseq[r] = len for a kept insertion (len > 0), 0 otherwise; seq_off[r] = the sum over r' < r of
 * (l_qseq[r'] + 1) / 2; nibble j of read r (high nibble first; the low nibble behind an odd read is 0) is the SOURCE's raw 4-bit
 * code at offset q = rep_qpos + 1 + j of its read rep_read, and code 15 (N) where include/brc.h spells N: q < 0, q >= l_qseq[rep_read],
 * rep_read >= n_reads.  brc_indels_gather therefore spells every allele of the joined view as it does on the source.
 *   counts [2]   ALWAYS the true totals: kept records, bytes of seq4 (modulo 2^32: a join of 4 GiB of inserted bases is not served)
 *   seq_cap      the bytes of dst->seq4: when counts[1] > seq_cap NOTHING of seq4 is written (everything else is).  So a caller asks
 *                for the counts alone (dst == NULL: nothing but counts and status is written, the views are not filled in), reads
 *                them — the one host synchronisation —, allocates exactly and calls again.
 *
 * REFERENCE SLICE.  Over the sources that have one (an indels view with ref != NULL): [ref_lo, ref_hi) = [min ref_lo_s, max ref_hi_s),
 * ref_len = their common ref_len.  Byte p - ref_lo is the raw character of the FIRST source whose slice holds p with p < ref_len and
 * a non-NUL character, NUL where there is none (include/brc.h reads NUL as N).  A later source holding another non-NUL character at p
 * sets BRC_JOIN_REF_DIFFERS.  No source with a reference: ref = NULL, ref_lo = ref_hi = ref_len = 0.
 *
 * out_view, out_indels: HOST structs the call fills in over dst's buffers (memory and device the sources'; pointers of empty buffers
 * NULL).  Either may be NULL: that half is not joined and its buffers of dst are not looked at (out_view: the planes and third-allele
 * records; out_indels: indel records, synthetic reads, reference slice, counts).
 * status: NULL, or ONE word in memory of the views' kind.  The library clears it on the stream before its launches, the kernels OR
 * bits into it, the host never reads it.
 * stream: a hipStream_t, or NULL for the default stream (ignored by the sim library).  The hip library returns once its launches are
 * enqueued and never waits; it allocates nothing; no kernel waits for another workgroup.  The result is a pure function of the
 * sources and the window: two calls give identical bytes (the one atomic counts, the other ORs a bit).
 *
 * BRC_E_ARG, and nothing is written:
 *   a NULL handle or sources; K outside 1 .. BRC_JOIN_MAX_SOURCES; a source without a view;
 *   a view with n_lib < 1, n_pos < 0, stride < n_pos, or — n_pos > 0 — without planes, or with n_xagg and no records;
 *   an indels view that disagrees with its view in memory, device, n_lib, pos0 or n_pos, or has n_slots and no records, or n_reads < 0;
 *   views of mixed memory kind or device, or not of this library's kind / the handle's device;
 *   more than BRC_JOIN_MAX_LIB joined libraries;
 *   n_pos < 0, stride < n_pos, pos0 + n_pos beyond 2^31 - 1;
 *   n_pos, n_xagg, n_slots or the reference slice at or above 0x7ffffff0 (32-bit indices);
 *   sources with a reference whose ref_len differ;
 *   seq_cap < 0;
 *   — with dst — both out_view and out_indels NULL; a NULL buffer of dst whose size is not 0 (seq4: when seq_cap > 0);
 *   a NULL workspace, or one smaller than brc_join_workspace says, where out_indels (or dst == NULL) meets n_slots > 0;
 *   dst == NULL with NULL counts;
 *   a destination buffer OVERLAPPING a source: checked for every buffer of dst, the workspace, counts and status against every
 *   source array whose extent the host knows — the planes (rows * stride_s words), the records, seq_off and l_qseq, the reference
 *   slice.  A source's seq4 has no host-known length and is not checked.
 * n_pos == 0 is BRC_OK: counts = {0, 0}, status = 0, the views describe an empty region (n_pos, n_xagg, n_slots, n_reads 0, every
 * pointer NULL, no reference), nothing else is written.
 */
int  brc_join_views(brc_join*, int32_t K, const brc_join_source* sources, int32_t pos0, int64_t n_pos, int64_t stride,
                    const brc_join_dest* dst, brc_device_view* out_view, brc_device_indels* out_indels,
                    uint32_t* counts, int64_t seq_cap, uint32_t* status,
                    void* workspace, size_t workspace_bytes, void* stream);

/* The last brc_join_views' account: seconds between the HIP events around its launches (hip: WAITS for the second event; sim: wall
 * time); the bytes the host can count — 116 per position and joined library read (where a source covers the window) and written, 64
 * per third-allele record and 72 per indel record each way, the reference slice once per source and once out (the nibbles are data
 * and are not counted).  (tools/join_bench.py) */
void brc_join_last_timing(const brc_join*, double* kernel_s, uint64_t* bytes_read, uint64_t* bytes_written);

#ifdef __cplusplus
}
#endif
#endif
