/* brc_cons.h — C-ABI of the device-side CONSENSUS CALLER: a window of a computed region (brc_device_view + brc_device_indels,
 * include/brc.h) and its sorted indel table (what brc_indels_gather, include/brc_indels.h, or brc_inorm_table, include/brc_inorm.h,
 * writes) turned into a SEQUENCE — one call per position from the pooled read counts of A C G T and of the reads that carry a
 * deletion across it, accepted insertions placed behind their anchors —, the per-position calls and counts, and the offset of every
 * reference position in the sequence (the liftover map between reference and consensus coordinates), IN THE MEMORY THE VIEWS LIVE IN.
 *
 * A library of its own (libbrc_cons_hip.so: the gfx950 kernels of bam_readcount_amd/csrc/brc_cons.hip; tests/cpu_cons/
 * libbrc_cons_sim.so: the same per-lane functions, brc_cons_core.h, run lane for lane on host memory) with a handle of its own.
 * It links nothing of the engine or of its siblings: views and tables are plain data.  Error codes are the BRC_E_* of include/brc.h.
 *
 * What it stands in for: the reference prints counts and leaves the call to whoever reads its text; a GPU consumer expanded the whole
 * region (brc_dense_expand: 312 bytes per position and library) and rebuilt the rule in array operations — which cannot place
 * insertions, and cannot know how many reads carry a deletion ACROSS a position: the planes count such reads nowhere, only the
 * deletion records at their anchors do.  The caller reads the compact planes once: slotid and the two slots' read counts. */
#ifndef BRC_CONS_H
#define BRC_CONS_H

#include "brc.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct brc_cons brc_cons;

/* One handle per device (hip: BRC_E_NODEVICE without a GPU — the product library has no CPU path; sim: host views carry device 0).
 * The handle owns two timing events and nothing else: sources are the views' and the table's, scratch and destinations the caller's. */
int  brc_cons_create(int device, brc_cons** out);
void brc_cons_destroy(brc_cons*);
const char* brc_cons_kind(void);                           /* "hip-gfx950" | "sim" */
const char* brc_cons_last_error(const brc_cons*);

/* brc_cons_params.flags */
#define BRC_CONS_ALIGNED      1u        /* one byte per position, deletions as `gap`, no insertion emitted */
#define BRC_CONS_FILL_REF     2u        /* an uncalled position prints the reference's character, not `fill` */
#define BRC_CONS_INS_CENTRIC  4u        /* the region was computed insertion-centric: the anchor's base counts exclude the insertion's reads */
#define BRC_CONS_MAX_LIB 254            /* libraries of a view the caller takes: lib_on travels in the kernel arguments */
#define BRC_CONS_NCNT 6                 /* planes of `cnt`: BRC_CONS_C_* */
#define BRC_CONS_C_A   0
#define BRC_CONS_C_C   1
#define BRC_CONS_C_G   2
#define BRC_CONS_C_T   3
#define BRC_CONS_C_DEL 4
#define BRC_CONS_C_INS 5
#define BRC_CONS_NO_INS 4294967295u     /* ins_rec of a position without an accepted insertion */
/* bits of the status word */
#define BRC_CONS_TABLE_NOT_ASCENDING 1u /* some pos[r] < pos[r - 1] */
#define BRC_CONS_TABLE_OUT_OF_RANGE  2u /* some record with len != 0 has a library outside [0, n_lib) */

/* The sorted indel table, where it lies: CALLER-owned memory of the views' kind.  pos, lib, len [m]; count [m] = row BRC_I_N of the
 * table's istat (istat + BRC_I_N * stride of a brc_indels_gather / brc_inorm_table destination whose planes lie `stride` >= m elements
 * apart); allele_off [m + 1], alleles [alleles_len] (the text of record r, sign first).  A record's pos is its ANCHOR: the base BEFORE
 * the indel (include/brc.h).  m == 0: no pointer is read. */
typedef struct brc_cons_table {
    int64_t m, stride;
    const int32_t *pos, *lib, *len;
    const uint32_t* count;
    const uint32_t* allele_off;
    const uint8_t* alleles;
    int64_t alleles_len;
} brc_cons_table;

typedef struct brc_cons_params {
    const uint8_t* lib_on;  /* HOST memory, view->n_lib bytes of 0 / 1: the counted libraries; NULL = all of them */
    uint32_t flags;         /* BRC_CONS_ALIGNED | BRC_CONS_FILL_REF | BRC_CONS_INS_CENTRIC */
    uint32_t min_depth, min_count, num, den;           /* the call: q(x) below */
    uint32_t ins_min_count, ins_num, ins_den;          /* the insertion test */
    uint32_t fill, gap;     /* characters 0 .. 255: what an UNCALLED / a DELETED position prints */
} brc_cons_params;

/* Bytes of scratch a call over n positions and a table of m records needs (a function of n, m and the view's n_xagg alone; 0 for
 * n <= 0 or a NULL view).  The scratch is the caller's, of the views' kind of memory, 4-byte aligned; its contents before and after a
 * call mean nothing. */
int64_t brc_cons_workspace(const brc_device_view*, int64_t n, int64_t m);

/*
 * THE RULE is pure integer arithmetic, stated on the dense result (brc_result) and the table.  A library l is COUNTED when lib_on is
 * NULL or lib_on[l] != 0.  For plane index k in [k0, k0 + n), every operand widened to uint64 first:
 *   c[b], b = A C G T   the sum over the counted libraries of istat[l][b][BRC_I_N][k] (buckets 1..4 of "=ACGTN"), i.e. with
 *                       expand_slots' precedence: slot 0's count, slot 1's where that is non-zero, the third-allele record's on top.
 *   d                   the sum of count[r] over the table records r with all of
 *                           len[r] < 0;  lib[r] inside [0, n_lib) and counted;  pos[r] - pos0 < k <= pos[r] - pos0 + |len[r]|
 *                       — a deletion covers the |len| positions BEHIND its anchor, and a record whose anchor lies in front of the
 *                       window (or whose end lies behind it, or behind ref_len) still counts inside it.  d IS COMPUTED MODULO 2^32
 *                       (a 32-bit difference array and one scan: the cost of a record does not depend on its length).
 *   T = c[A] + c[C] + c[G] + c[T] + d
 *   q(x) := x >= min_count && x * den >= num * T
 *   the call is the first rule that applies:
 *     UNCALLED  when T < min_depth
 *     DELETED   when q(d) and d > c[b] for every b (a tie with a base is not deleted)
 *     UNCALLED  when no base satisfies q
 *     otherwise the IUPAC code, upper case, of the set S of bases that satisfy q:
 *         A: A   C: C   G: G   T: T   AC: M   AG: R   AT: W   CG: S   CT: Y   GT: K   ACG: V   ACT: H   AGT: D   CGT: B   ACGT: N
 *         ("=ACMGRSVTWYHKDBN"[mask], mask = 1 * [A in S] + 2 * [C in S] + 4 * [G in S] + 8 * [T in S])
 *   call byte: the code; `gap` for DELETED; for UNCALLED `fill`, or with BRC_CONS_FILL_REF the RAW reference character of position
 *     pos0 + k from brc_device_indels.ref / ref_lo / ref_hi / ref_len by brc_select.h's rule: outside the slice, at or past ref_len, a
 *     NUL character or no reference => 'N'.
 * THE INSERTION BEHIND k:
 *   run(r)       the maximal stretch of consecutive table indices around r whose pos equals pos[r]
 *   text(x)      alleles[min(allele_off[x], A) .. min(allele_off[x + 1], A)) with A = alleles_len, empty when the second offset is below
 *                the first (brc_ivet.h's rule): no content of allele_off makes a read leave `alleles`
 *   candidates   records r with len[r] > 0, lib[r] inside [0, n_lib) and counted, pos[r] - pos0 == k
 *   support(r)   the sum of count[x] over the x of run(r) with a counted library, len[x] == len[r] and text(x) == text(r) bytewise (r
 *                itself among them): one text in two libraries is pooled, a prefix or another text of the same length is another allele
 *   I            the sum of count[r] over all candidates
 *   T' = T + (BRC_CONS_INS_CENTRIC ? I : 0)      (on an insertion-centric engine the anchor's base counts exclude the insertion's
 *                reads, bamreadcount.cpp:343)
 *   chosen       the candidate with the largest support; a tie goes to the smallest table index
 *   accepted     when T' >= min_depth, support >= ins_min_count and support * ins_den >= ins_num * T'
 *   emitted      the chosen record's text behind its first byte (the sign), as it is ('=' and 'N' bytes pass through)
 *   support, I and the products are taken in uint64: exact while the counts of a run sum to less than 2^47.
 * On a table that is not sorted by position (BRC_CONS_TABLE_NOT_ASCENDING) c, d and the calls stay exact; the insertions of a position
 * are taken from the run of that position with the smallest first index alone; every store stays in range.
 * LIMIT: a deletion whose anchor lies in front of the view's first position is unknown to the view — it is in no table of this
 * region — and does not count.
 *
 * Destinations: CALLER-owned memory of the views' kind, any of them NULL (not wanted):
 *   counts  [1]                       ALWAYS the true number of sequence bytes, whatever seq_cap is (modulo 2^32: exact for a table as
 *                                     the two libraries above write it, whose texts do not overlap)
 *   call    [n]                       one byte per position: the call byte above
 *   cnt     [BRC_CONS_NCNT][dst_stride]  uint32 planes dst_stride >= n elements apart: the low 32 bits of c[A], c[C], c[G], c[T], d and
 *                                     of the chosen candidate's support (0 without a candidate); elements [n, dst_stride) not touched
 *   ins_rec [n]                       the accepted record's table index, BRC_CONS_NO_INS where none is accepted
 *   off     [n + 1]                   the offset of position k's first sequence byte; off[n] = the total
 *   seq     [seq_cap]                 for each k in order: the call byte unless DELETED, then the accepted insertion's emitted text.
 *                                     Each of the two is a PIECE: a piece is written iff it ends at or in front of min(seq_cap,
 *                                     counts[0]) — a piece that does not fit whole is not written at all, nothing else is touched.
 * With BRC_CONS_ALIGNED: seq[j] = call[j] (`gap` included), no insertion is emitted, off[j] = j, counts[0] = n — no count has to be
 * read first; cnt and ins_rec are what they are without the flag.  Otherwise a caller asks for `counts` alone, reads it — the one host
 * synchronisation — and supplies the exact capacity second, as with brc_indels_gather.
 * status: NULL, or ONE word in memory of the views' kind.  The library clears it on the stream before its launches, the kernels OR
 * bits into it, the host never reads it.
 * workspace: brc_cons_workspace(view, n, m) bytes of the caller's, of the views' kind.
 * stream: a hipStream_t, or NULL for the default stream (ignored by the sim library).  The hip library returns once its work is
 * enqueued on it and never waits; it allocates nothing; no kernel waits for another workgroup.  The result is a pure function of the
 * views, the table, the window and the parameters: two calls give identical bytes (the atomics inside are integer ones — they link
 * records, add counts, take a minimum and OR bits —, so order-free).
 * Views and table must stay valid until that work has run; params and lib_on are read before the call returns.
 * BRC_E_ARG, and nothing is written: a NULL handle, view, indels view, params or table; what brc_select_sites refuses about its
 * views and the window (k0 < 0, n < 0, k0 + n > n_pos, a view without planes, records without their arrays, the two views disagreeing
 * in memory / device / n_lib / pos0 / n_pos, memory that is not this library's — BRC_MEM_DEVICE for hip, BRC_MEM_HOST for sim — or of
 * another device than the handle's); more than BRC_CONS_MAX_LIB libraries; dst_stride < n; seq_cap < 0; m < 0, stride < m, a table
 * with m > 0 and a NULL pos, lib, len, count, allele_off or alleles; alleles_len < 0; m, n or n + alleles_len too large for 32-bit
 * indices; flags with unknown bits; den or ins_den outside [1, 65535], num > den, ins_num > ins_den (with these bounds every product
 * above fits in 64 bits); fill or gap above 255; a lib_on byte above 1; no counted library; a NULL workspace with n > 0.
 * n == 0 is BRC_OK: counts[0] = 0, off[0] = 0, a status word is cleared.
 */
int  brc_cons_call(brc_cons*, const brc_device_view*, const brc_device_indels*, const brc_cons_params*, const brc_cons_table*,
                   int64_t k0, int64_t n, int64_t dst_stride, int64_t seq_cap,
                   uint32_t* counts, uint8_t* call, uint32_t* cnt, uint32_t* ins_rec, uint32_t* off, uint8_t* seq,
                   uint32_t* status, void* workspace, void* stream);

/* The last brc_cons_call's account: seconds between the HIP events around its launches (hip: WAITS for the second event; sim: wall
 * time); the bytes its sweeps ask for that the host can count — three words per position and counted library, the scratch words and
 * the reference byte per position, 64 bytes per third-allele record, four words and two offsets per table record (texts and the
 * runs' neighbours are data and are not counted) — and the bytes it writes, destinations and scratch, the sequence counted as n bytes.
 * Neither depends on what the table holds: a deletion of 100 000 bases costs what a deletion of one base costs.
 * (tools/cons_bench.py) */
void brc_cons_last_timing(const brc_cons*, double* kernel_s, uint64_t* bytes_read, uint64_t* bytes_written);

#ifdef __cplusplus
}
#endif
#endif
