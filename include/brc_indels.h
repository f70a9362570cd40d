/* brc_indels.h — C-ABI of the device-resident INDEL table: the indel buckets of a computed region (brc_device_indels, include/brc.h:
 * 72-byte records in unspecified order) as brc_result.indel orders and spells them — sorted by (position, library, allele text
 * bytewise), structure-of-arrays, with the allele text and the thirteen printed columns — IN THE MEMORY THE VIEW LIVES IN: nothing
 * crosses PCIe and no host std::map is built.
 *
 * A library of its own (libbrc_indels_hip.so: the gfx950 kernels of bam_readcount_amd/csrc/brc_indels.hip; tests/sim_indels/
 * libbrc_indels_sim.so: the same per-lane functions, brc_indels_core.h, run lane for lane on host memory) with a handle of its own.
 * It links nothing of the engine: the view is plain data.  Error codes are the BRC_E_* of include/brc.h; the metric columns are the
 * BRC_M_* of include/brc_dense.h.
 *
 * What it stands in for: LibraryCounts::indel_stats, a std::map<std::string, BasicStat> per library that pileup_func fills and prints
 * in key order (bamreadcount.cpp:315-342, 389-401); brc_fetch_result gives a caller the same list as host structures (assemble_indels,
 * brc_host.cpp); this gives it to a caller on the GPU.  The table is the pileup position's own buckets, as brc_result.indel is: what
 * IndelQueue does with deletions when the lines are printed is not part of it. */
#ifndef BRC_INDELS_H
#define BRC_INDELS_H

#include "brc.h"
#include "brc_dense.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct brc_indels brc_indels;

/* One handle per device (hip: BRC_E_NODEVICE without a GPU — the product library has no CPU path; sim: host views carry device 0).
 * The handle owns two timing events and nothing else: sources are the view's, scratch and destinations the caller's. */
int  brc_indels_create(int device, brc_indels** out);
void brc_indels_destroy(brc_indels*);
const char* brc_indels_kind(void);                         /* "hip-gfx950" | "sim" */
const char* brc_indels_last_error(const brc_indels*);

/* Bytes of scratch a gather over n positions of the view needs (a function of n and the view's n_slots alone; 0 when n == 0 or the
 * view has no slots, or for a NULL view).  The scratch is the caller's, of the view's kind of memory, 4-byte aligned; its contents
 * before and after a call mean nothing. */
size_t brc_indels_workspace(const brc_device_indels*, int64_t n);

/*
 * The live records (len != 0) whose position lies in [pos0 + k0, pos0 + k0 + n) -> CALLER-owned memory of the view's kind, in
 * brc_result.indel's order: ascending (pos, lib, allele text bytewise) — '+' before '-', a prefix before the longer text: the
 * iteration order of the reference's std::map.  Record r lands at index r of every destination; any destination may be NULL.
 *   counts      [2]            ALWAYS the true totals of the window: records, allele bytes (signs included)
 *   pos, lib, len, rep_read, rep_qpos   [cap]   the record's fields (brc_indel)
 *   istat, fstat    [9][cap], [4][cap]   the record's accumulators, BRC_I_* / BRC_F_* planes `cap` elements apart
 *   metrics     [13][cap]      BRC_M_* of them, one correctly rounded fp32 division per average (brc_dense.h); indel buckets carry no
 *                              base-quality sum, so that column is 0 as the reference prints it (BasicStat.cpp:123)
 *   allele_off  [cap + 1], alleles [alleles_cap]   alleles[allele_off[r] .. allele_off[r + 1]) is record r's text, sign first ("+ACG",
 *                              "-TT"): an inserted base from "=ACGTN", N past the read's end; a deleted base the reference's raw
 *                              character, N where there is none (include/brc.h: brc_device_indels)
 * Records at index >= cap are not written, their text included (cap bounds `alleles` too); a record whose text does not fit
 * alleles_cap whole has none of its bytes written (allele_off is true wherever it is written: indices 0 .. min(counts[0], cap)).  Nothing at or behind index counts[0] of a
 * per-record destination, counts[0] + 1 of allele_off, counts[1] of alleles is touched.  So a caller asks for `counts` alone, reads
 * them — the one host synchronisation — allocates exactly and calls again.
 * stream: a hipStream_t, or NULL for the default stream (ignored by the sim library).  The hip library returns once its launches are
 * enqueued and never waits; no kernel waits for another workgroup.  The result is a pure function of the view and the window: two
 * calls give identical bytes (the atomics inside only count, and place records in runs whose order is then fixed by rank).
 * BRC_E_ARG, and nothing is written: a NULL handle or view, k0 < 0, n < 0, k0 + n > n_pos, cap < 0, alleles_cap < 0, a view whose
 * `memory` is not this library's (BRC_MEM_DEVICE for hip, BRC_MEM_HOST for sim) or that lies on another device than the handle's, a
 * view with slots but without reads arrays, and — when n > 0 and the view has slots — a NULL workspace or one smaller than
 * brc_indels_workspace says.  n == 0 or n_slots == 0 is BRC_OK: counts = {0, 0}, allele_off[0] = 0.
 */
int  brc_indels_gather(brc_indels*, const brc_device_indels*, int64_t k0, int64_t n,
                       void* workspace, size_t workspace_bytes,
                       uint32_t* counts,
                       int64_t cap, int64_t alleles_cap,
                       int32_t* pos, int32_t* lib, int32_t* len, uint32_t* rep_read, int32_t* rep_qpos,
                       uint32_t* istat, float* fstat, float* metrics,
                       uint32_t* allele_off, uint8_t* alleles,
                       void* stream);

/* The last brc_indels_gather's account: seconds between the HIP events around its launches (hip: WAITS for the second event; sim:
 * wall time); the bytes its two sweeps over the slots read and the scratch bytes every call writes — what the host knows without
 * the record count (the per-record traffic of ranking and emitting is not counted).  (tools/indels_bench.py) */
void brc_indels_last_timing(const brc_indels*, double* kernel_s, uint64_t* bytes_read, uint64_t* bytes_written);

#ifdef __cplusplus
}
#endif
#endif
