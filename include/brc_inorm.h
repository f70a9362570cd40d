/* brc_inorm.h — C-ABI of the device-side INDEL NORMALISATION: every record of a sorted indel table of a computed region (what
 * brc_indels_gather, include/brc_indels.h, writes) LEFT-ALIGNED against the uploaded reference slice, and the records that became
 * identical in (position, library, length, text) MERGED into one — a new table in brc_indels_gather's format and order, plus, per
 * input record, where it went — IN THE MEMORY THE VIEW LIVES IN.  The new table is what brc_ivet_records (include/brc_ivet.h) takes:
 * its allele-aware control veto compares records of one position, and an aligner is free to place one event anywhere inside a
 * homopolymer or a tandem repeat.
 *
 * A library of its own (libbrc_inorm_hip.so: the gfx950 kernels of bam_readcount_amd/csrc/brc_inorm.hip; tests/sim_inorm/
 * libbrc_inorm_sim.so: the same per-lane functions, brc_inorm_core.h, run lane for lane on host memory) with a handle of its own.
 * It links nothing of the engine or of its siblings: the view and the table are plain data.  Error codes are the BRC_E_* of
 * include/brc.h; the metric columns are the BRC_M_* of include/brc_dense.h.
 *
 * What it stands in for: a consumer copied the table to the host and walked it there, as bcftools norm or vt normalize walk a VCF. */
#ifndef BRC_INORM_H
#define BRC_INORM_H

#include "brc.h"
#include "brc_dense.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct brc_inorm brc_inorm;

/* One handle per device (hip: BRC_E_NODEVICE without a GPU — the product library has no CPU path; sim: host views carry device 0).
 * The handle owns two timing events and nothing else: sources are the view's and the table's, scratch and destinations the caller's. */
int  brc_inorm_create(int device, brc_inorm** out);
void brc_inorm_destroy(brc_inorm*);
const char* brc_inorm_kind(void);                          /* "hip-gfx950" | "sim" */
const char* brc_inorm_last_error(const brc_inorm*);

#define BRC_INORM_MAX_SHIFT 1048576u    /* 1 << 20: the largest max_shift */
/* bits of a record's flags */
#define BRC_INORM_NOT_JUDGED 1u         /* the record is not part of the new table */
#define BRC_INORM_LIMIT      2u         /* the walk stopped at max_shift although a step was possible */
#define BRC_INORM_EDGE       4u         /* the walk stopped at the floor although a step was possible */
/* bits of the status word */
#define BRC_INORM_TABLE_BAD  1u         /* some record is not judged */
#define BRC_INORM_ANY_LIMIT  2u         /* some record carries BRC_INORM_LIMIT */
#define BRC_INORM_ANY_EDGE   4u         /* some record carries BRC_INORM_EDGE */

typedef struct brc_inorm_params {
    uint32_t max_shift;                 /* 0 .. BRC_INORM_MAX_SHIFT: the most left steps of a record; 0 merges without shifting */
    uint32_t reserved[3];               /* must be 0 */
} brc_inorm_params;

/* The input table, where it lies: CALLER-owned memory of the view's kind.  pos, lib, len [m]; rep_read, rep_qpos [m] or NULL (then
 * written as 0); istat [9][stride], fstat [4][stride] (BRC_I_*, BRC_F_* planes `stride` >= m elements apart: brc_indels_gather's
 * `cap`); allele_off [m + 1], alleles [alleles_len].  Nothing but rep_read and rep_qpos is optional when m > 0. */
typedef struct brc_inorm_source {
    int64_t m, stride;
    const int32_t *pos, *lib, *len;
    const uint32_t* rep_read;
    const int32_t* rep_qpos;
    const uint32_t* istat;
    const float* fstat;
    const uint32_t* allele_off;
    const uint8_t* alleles;
    int64_t alleles_len;
} brc_inorm_source;

/* Bytes of scratch a call over a window of n positions and a table of m records needs: a function of n and m alone, 0 when either is
 * 0 or below.  The scratch is the caller's, of the view's kind of memory, 4-byte aligned; its contents before and after a call mean
 * nothing. */
size_t brc_inorm_workspace(int64_t n, int64_t m);

/*
 * THE DEFINITION.
 *   R(p)      the raw reference character of contig position p as include/brc.h defines it for deleted bases: ref[p - ref_lo] for
 *             ref_lo <= p < ref_hi, p < ref_len, a non-NULL ref and a non-NUL character; otherwise NONE.
 *   base(c)   ASCII letters fold to upper case; one of A C G T, or NONE for anything else (N, IUPAC codes, '=', NONE).
 *   match     two characters match when both have a base and the bases are equal.
 *   window    [first, first + n) with first = pos0 + k0, as in brc_indels_gather; floor = max(first, ref_lo).
 *   text(r)   alleles[min(allele_off[r], A) .. min(allele_off[r + 1], A)) with A = alleles_len, empty when the second offset is below
 *             the first (brc_ivet.h's rule: no content of allele_off makes a read leave `alleles`).
 * Record r is JUDGED when len[r] != 0, first <= pos[r] < first + n, 0 <= lib[r] < n_lib, text(r) has |len[r]| + 1 bytes and its
 * first byte is '+' for len[r] > 0, '-' for len[r] < 0.  Any other record: flags[r] = BRC_INORM_NOT_JUDGED, npos[r] = pos[r],
 * shift[r] = 0, group[r] = -1; it is not part of the new table, and BRC_INORM_TABLE_BAD is set in `status`.
 *
 * LEFT STEPS of a judged record: p = pos[r], L = |len[r]|, t = the L bytes behind the sign, s = 0, flags = 0.  Repeat:
 *   1. if R(p) does not match t[L - 1]: stop.
 *   2. (a step is possible)  if s == max_shift: stop, flags = BRC_INORM_LIMIT.  If p - 1 < floor: stop, flags = BRC_INORM_EDGE.
 *   3. t <- c ++ t[0 .. L - 1) with c = t[L - 1] for an insertion, the raw R(p) for a deletion; p <- p - 1; s <- s + 1.
 * One rule for both kinds: an insertion's text rotates, a deletion's text becomes the raw reference characters of the stretch it now
 * deletes — what brc_indels_gather would have spelled there, soft-masked lower case included.  The case-folded haplotype (the
 * reference with the allele applied) is unchanged, and a second normalisation does nothing more.
 * npos[r] = p, shift[r] = s, flags[r]; BRC_INORM_ANY_LIMIT / BRC_INORM_ANY_EDGE in `status`.
 *
 * MERGING: two judged records are equal when npos, lib, len and the normalised text are bytewise equal — within a library: libraries
 * are never merged, the control veto needs them apart.  One merged record per class:
 *   pos = npos; lib, len and the text of the class
 *   istat[f]   the sum of the members' in uint32, modulo 2^32
 *   fstat[f]   the fp32 sum of the members', SEQUENTIAL IN ASCENDING INPUT INDEX, one rounding per addition, starting from the first
 *              member's value (not from 0)
 *   metrics    BRC_M_* of the merged sums, one correctly rounded fp32 division per average (brc_dense.h)
 *   rep_read, rep_qpos   those of the member with the smallest input index (0 when the source has none) — PROVENANCE ONLY: a rotated
 *              insertion is no longer spelled by those read bases
 *   members    the class's size
 * in brc_indels.h's order: ascending (pos, lib, text bytewise, sign included).  group[r] = the index of the merged record r went into.
 *
 * Destinations: CALLER-owned memory of the view's kind, any of them NULL (not wanted).
 *   per input record   npos, shift, flags, group [m]
 *   counts      [2]    ALWAYS the true totals: merged records, allele bytes (signs included)
 *   pos, lib, len, rep_read, rep_qpos, members   [cap]
 *   istat, fstat, metrics   [9][cap], [4][cap], [13][cap]
 *   allele_off  [cap + 1], alleles [alleles_cap]
 * cap and alleles_cap bound the writes exactly as in brc_indels_gather: records at index >= cap are not written, their text
 * included; a record whose text does not fit alleles_cap whole has none of its bytes written; allele_off is true wherever it is
 * written (indices 0 .. min(counts[0], cap)); nothing at or behind counts[0] of a per-record destination, counts[0] + 1 of allele_off,
 * counts[1] of alleles is touched.  So a caller asks for `counts` alone, reads them — the one host synchronisation — allocates exactly
 * and calls again.
 * status: NULL, or ONE word in memory of the view's kind.  The library clears it on the stream before its launches, the kernels OR
 * bits into it, the host never reads it.
 * Only the indels view is needed: it supplies the reference slice, pos0, n_pos and n_lib; its records are not read.
 * stream: a hipStream_t, or NULL for the default stream (ignored by the sim library).  The hip library returns once its launches are
 * enqueued and never waits; it allocates nothing; no kernel waits for another workgroup.  The result is a pure function of the view,
 * the table, the window and the parameters: two calls give identical bytes (the atomics inside only count, OR bits, and place
 * records in runs whose order is then fixed by rank).
 * BRC_E_ARG, and nothing is written: a NULL handle, view, params or source; k0 < 0, n < 0, k0 + n > n_pos; cap < 0, alleles_cap < 0;
 * a view whose `memory` is not this library's or that lies on another device than the handle's; m < 0, stride < m, alleles_len < 0;
 * m > 0 with a NULL pos, lib, len, istat, fstat, allele_off or alleles; m or n too large for 32-bit indices; max_shift above
 * BRC_INORM_MAX_SHIFT; a non-zero reserved word; — when m > 0 and n > 0 — a NULL workspace or one smaller than brc_inorm_workspace
 * says.
 * m == 0 or n == 0 is BRC_OK: counts = {0, 0}, allele_off[0] = 0, status = 0, and nothing else is written.
 */
int  brc_inorm_table(brc_inorm*, const brc_device_indels*, const brc_inorm_params*, const brc_inorm_source*,
                     int64_t k0, int64_t n,
                     void* workspace, size_t workspace_bytes,
                     uint32_t* counts,
                     int32_t* npos, uint32_t* shift, uint32_t* flags, int32_t* group,
                     int64_t cap, int64_t alleles_cap,
                     int32_t* pos, int32_t* lib, int32_t* len, uint32_t* rep_read, int32_t* rep_qpos, uint32_t* members,
                     uint32_t* istat, float* fstat, float* metrics,
                     uint32_t* allele_off, uint8_t* alleles,
                     uint32_t* status, void* stream);

/* The last brc_inorm_table's account: seconds between the HIP events around its launches (hip: WAITS for the second event; sim: wall
 * time); the bytes the host can count — per input record five table words, two offsets and the 13 sums read, per position and per
 * record the scratch words written (the reference and text bytes walked, and the merged table, are data and are not counted).
 * (tools/inorm_bench.py) */
void brc_inorm_last_timing(const brc_inorm*, double* kernel_s, uint64_t* bytes_read, uint64_t* bytes_written);

#ifdef __cplusplus
}
#endif
#endif
