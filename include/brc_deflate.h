/* brc_deflate.h — C-ABI of the BGZF deflater: any bytes in, whole BGZF members out (the output text of the command line, compressed
 * where it was written: --brc-bgzf-output).
 *
 * A library of its own (libbrc_deflate_hip.so: the gfx950 kernels of bam_readcount_amd/csrc/brc_deflate.hip; tests/sim_deflate/
 * libbrc_deflate_sim.so: the same compressor, brc_deflate_core.h, run lane for lane on host threads) with a handle of its own: it
 * shares nothing with brc_engine or with the inflater, and include/brc.h does not know it.  Error codes are the BRC_E_* of
 * include/brc.h.
 *
 * What it stands in for: the reference prints plain text (bamreadcount.cpp:301-352, std::cout); whoever keeps that text pipes it
 * through bgzip.  The members written here are what `bgzip` would write at its block size of 0xff00 input bytes, each an independent
 * deflate stream: zcat, bgzip -d and tabix -s1 -b2 -e2 read them.  The bytes are a pure function of the input bytes. */
#ifndef BRC_DEFLATE_H
#define BRC_DEFLATE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef BRC_OK
#define BRC_OK            0
#define BRC_E_ARG        -1
#define BRC_E_NODEVICE   -2
#define BRC_E_HIP        -3
#define BRC_E_NOMEM      -4
#endif

#define BRC_DEFLATE_MEMBER_INPUT 0xff00   /* input bytes of every member but the last of a call */

typedef struct brc_deflater brc_deflater;

/* One deflater per device; BRC_E_NODEVICE without a GPU — the product library has no CPU path.  Its copies and launches run on a
 * stream of its own.  Calls on one handle are serialised; several handles may be alive and used side by side. */
int  brc_deflater_create(int device, brc_deflater** out);
void brc_deflater_destroy(brc_deflater* h);
/* "hip-gfx950" | "sim" */
const char* brc_deflater_kind(void);
const char* brc_deflater_last_error(const brc_deflater* h);

/* The most bytes brc_deflate_bgzf writes for src_len bytes: every member stored (src_len + 31 per member). */
size_t brc_deflate_bound(size_t src_len);

/* src[0, src_len) is cut into consecutive members of BRC_DEFLATE_MEMBER_INPUT bytes, the last one shorter; dst receives the members
 * back to back (*dst_len bytes, *n_members members; no end-of-file member).  src_len == 0: no member, *dst_len == 0.
 * BRC_E_ARG: a NULL handle or pointer, or dst_cap below brc_deflate_bound(src_len) — nothing is written then. */
int  brc_deflate_bgzf(brc_deflater* h, const void* src, size_t src_len, void* dst, size_t dst_cap, size_t* dst_len, size_t* n_members);

/* The 28-byte BGZF end-of-file member (SAMv1 4.1.2), to be written once behind the last member of a file. */
const uint8_t* brc_deflate_eof_block(size_t* len);

/* Page-locked host memory (the brc_host_alloc idiom of include/brc.h): src / dst that lie in it are copied by the device straight
 * from / to where they are; any other memory goes through the handle's own staging.  NULL when none can be had. */
void* brc_deflate_host_alloc(size_t bytes);
void  brc_deflate_host_free(void* p);

/* The last call's account: seconds between the events around the device work (clearing the slots, the compressor, the scan of the
 * member sizes, the gather), seconds of the whole call (H2D, device work, D2H), bytes in and out.  (tools/deflate_bench.py,
 * BRC_CLI_TIMING) */
void brc_deflater_last_timing(const brc_deflater* h, double* kernel_s, double* call_s, uint64_t* bytes_in, uint64_t* bytes_out);

#ifdef __cplusplus
}
#endif
#endif
