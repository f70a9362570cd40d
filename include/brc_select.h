/* brc_select.h — C-ABI of the device-side SITE SELECTION: the plane positions of a computed region (brc_device_view +
 * brc_device_indels, include/brc.h) that carry non-reference evidence — a base other than the reference's, an insertion, a deletion —
 * in "case" libraries and lack it in "control" libraries, as an ascending list of plane indices with a reason word per element, IN THE
 * MEMORY THE VIEWS LIVE IN.  The list is what brc_panel_gather (include/brc_panel.h) takes: region -> candidates -> panel runs without
 * the planes ever being expanded, and the only thing a host has to read is the count (a size).
 *
 * A library of its own (libbrc_select_hip.so: the gfx950 kernels of bam_readcount_amd/csrc/brc_select.hip; tests/sim_select/
 * libbrc_select_sim.so: the same per-lane functions, brc_select_core.h, run lane for lane on host memory) with a handle of its own.
 * It links nothing of the engine: the views are plain data.  Error codes are the BRC_E_* of include/brc.h.
 *
 * What it stands in for: the reference prints every position and leaves the filter over allele counts to whoever reads its text
 * (bamreadcount.cpp:351-416); a GPU consumer had to expand the whole region (brc_dense_expand: 312 bytes per position and library)
 * and filter that.  The selector reads the compact planes once: depth, slotid and the two slots' read counts. */
#ifndef BRC_SELECT_H
#define BRC_SELECT_H

#include "brc.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct brc_select brc_select;

/* One handle per device (hip: BRC_E_NODEVICE without a GPU — the product library has no CPU path; sim: host views carry device 0).
 * The handle owns two timing events and nothing else: sources are the views', scratch and destinations the caller's. */
int  brc_select_create(int device, brc_select** out);
void brc_select_destroy(brc_select*);
const char* brc_select_kind(void);                         /* "hip-gfx950" | "sim" */
const char* brc_select_last_error(const brc_select*);

/* brc_select_params.flags: what is looked for */
#define BRC_SELECT_SNV    1u
#define BRC_SELECT_INDEL  2u
/* brc_select_params.role[l] */
#define BRC_ROLE_IGNORE   0
#define BRC_ROLE_CASE     1
#define BRC_ROLE_CONTROL  2
#define BRC_SELECT_MAX_LIB 254          /* libraries of a view the selector takes: the roles travel in the kernel arguments */
/* bits of a reason word */
#define BRC_WHY_A    1u
#define BRC_WHY_C    2u
#define BRC_WHY_G    4u
#define BRC_WHY_T    8u
#define BRC_WHY_INS 16u
#define BRC_WHY_DEL 32u

typedef struct brc_select_params {
    const uint8_t* role;    /* HOST memory, view->n_lib entries: 0 ignore, 1 case, 2 control; NULL = every library is a case library */
    uint32_t flags;         /* BRC_SELECT_SNV | BRC_SELECT_INDEL */
    uint32_t min_depth, min_alt, frac_num, frac_den;                  /* case test */
    uint32_t ctl_min_depth, ctl_max_alt, ctl_frac_num, ctl_frac_den;  /* control test */
} brc_select_params;

/* Bytes of scratch a selection over n positions needs (a function of n and the view's n_xagg alone; 0 for n <= 0 or a NULL view).
 * The scratch is the caller's, of the views' kind of memory, 4-byte aligned; its contents before and after a call mean nothing. */
int64_t brc_select_workspace(const brc_device_view*, const brc_device_indels*, int64_t n);

/*
 * THE PREDICATE is pure integer arithmetic, stated on the dense result (brc_result).  For plane index k in [k0, k0 + n), library l:
 *   D   = depth[l][k]
 *   C_b = istat[l][b][BRC_I_N][k] for b in A C G T (buckets 1..4 of "=ACGTN"; '=' and 'N' are never evidence)
 *   R   = the reference character of position pos0 + k from brc_device_indels.ref / ref_lo / ref_hi / ref_len, by the rule brc.h gives
 *         for deleted bases: outside the slice, at or past ref_len, a NUL character or no reference => 'N'
 *   case_ok(l, c): D >= min_depth     && c >= min_alt     && c * frac_den     >= frac_num     * D      (products in 64 bits)
 *   ctl_ok(l, c):  D >= ctl_min_depth && c <= ctl_max_alt && c * ctl_frac_den <= ctl_frac_num * D
 * Bits of why:
 *   BRC_WHY_A / C / G / T (flags & BRC_SELECT_SNV): R is one of "ACGTacgt", b is not R's base, SOME case library has case_ok(l, C_b) and
 *         EVERY control library has ctl_ok(l, C_b).  A position whose R is anything else (N, IUPAC codes, NUL) sets none of them.
 *   BRC_WHY_INS / BRC_WHY_DEL (flags & BRC_SELECT_INDEL): some live record (len != 0) of brc_device_indels.slots with pos == pos0 + k,
 *         that sign of len, a case library and case_ok(lib, i[BRC_I_N]) against depth[lib][k] sets the bit; it is cleared again when a
 *         control library has D < ctl_min_depth, or has a live record of the same position and sign whose count fails the last two
 *         terms of ctl_ok.  ALLELE TEXT IS NOT COMPARED: a control insertion of any spelling and length vetoes an insertion candidate
 *         of that position, a control deletion of any length a deletion candidate; an insertion never vetoes a deletion or the reverse.
 * A position is selected iff why != 0.  EMPTY positions of a site-list axis (brc_region_windows) have no counts and are never selected.
 *
 * Destinations: CALLER-owned memory of the views' kind, any of them NULL (not wanted):
 *   counts  [1]     the number of selected positions of the window: the true total whatever cap is
 *   idx     [cap]   for j < min(total, cap): the plane index (k0 <= idx[j] < k0 + n), strictly ascending
 *   why     [cap]   for j < min(total, cap): the reason word of idx[j]
 * Nothing at or behind index min(total, cap) is touched.  So a caller asks for `counts` alone, reads it — the one host
 * synchronisation — allocates exactly and calls again; idx is then what brc_panel_gather takes.
 * workspace: brc_select_workspace(view, indels, n) bytes of the caller's, of the views' kind.
 * stream: a hipStream_t, or NULL for the default stream (ignored by the sim library).  The hip library returns once its work is
 * enqueued on it and never waits; it allocates nothing; no kernel waits for another workgroup.  The result is a pure function of the
 * views, the window and the parameters: two calls give identical bytes (the atomics inside only link records and OR flag bits).
 * Both views must stay valid (include/brc.h) until that work has run; params and role are read before the call returns.
 * BRC_E_ARG, and nothing is written: a NULL handle, view, indels view or params; what brc_dense_expand and brc_indels_gather refuse
 * about their views and the window (k0 < 0, n < 0, k0 + n > n_pos, a view without planes, records without their arrays, memory that is
 * not this library's — BRC_MEM_DEVICE for hip, BRC_MEM_HOST for sim — or of another device than the handle's); the two views
 * disagreeing in memory / device / n_lib / pos0 / n_pos; more than BRC_SELECT_MAX_LIB libraries; flags == 0 or with unknown bits;
 * min_alt == 0, frac_den == 0 or ctl_frac_den == 0; a role above 2; no case library; cap < 0; a NULL workspace with n > 0;
 * k0 + n > 2^31 - 1 (idx has 32 bits, like the k of a third-allele record).
 * n == 0 is BRC_OK: counts[0] = 0.
 */
int  brc_select_sites(brc_select*, const brc_device_view*, const brc_device_indels*, const brc_select_params*,
                      int64_t k0, int64_t n, int64_t cap,
                      int32_t* idx, uint32_t* why, uint32_t* counts, void* workspace, void* stream);

/* The last brc_select_sites's account: seconds between the HIP events around its launches (hip: WAITS for the second event; sim: wall
 * time); the bytes its sweeps ask for — 4 words per position and library, the scratch words and the reference byte per position, 64
 * bytes per third-allele record, 72 per indel record — and the scratch bytes it writes (what the host knows without the count: the
 * list itself is not counted).  (tools/select_bench.py) */
void brc_select_last_timing(const brc_select*, double* kernel_s, uint64_t* bytes_read, uint64_t* bytes_written);

#ifdef __cplusplus
}
#endif
#endif
