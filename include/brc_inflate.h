/* brc_inflate.h — C-ABI of the BGZF inflater: raw BGZF bytes in, inflated and CRC-checked bytes out.
 *
 * A library of its own (libbrc_inflate_hip.so: the gfx950 kernel of bam_readcount_amd/csrc/brc_inflate.hip; tests/sim_inflate/
 * libbrc_inflate_sim.so: the same decoder, brc_inflate_core.h, run lane for lane on host threads) with a handle of its own: it
 * shares nothing with brc_engine, and include/brc.h does not know it.  Error codes are the BRC_E_* of include/brc.h.
 *
 * What it stands in for: the reference reads its BAM through samtools' bgzf layer under samfetch (bamreadcount.cpp:602,
 * bam_fetch -> bam_read1 -> bgzf_read -> inflate of one block at a time); here a caller hands over the compressed bytes of many
 * blocks at once. */
#ifndef BRC_INFLATE_H
#define BRC_INFLATE_H

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

/* per-member status (status[i] of brc_inflate_bgzf) */
#define BRC_INF_OK            0
#define BRC_INF_BAD_HEADER    1   /* ISIZE above 65536, or a member shorter than its own header and trailer */
#define BRC_INF_BAD_STREAM    2   /* not a deflate stream: block type 3, LEN != ~NLEN, over-subscribed or incomplete code lengths, a
                                     reserved symbol (286, 287, 30, 31), a distance that reaches before the member's output */
#define BRC_INF_SIZE_MISMATCH 3   /* the stream yields more or fewer bytes than ISIZE */
#define BRC_INF_CRC_MISMATCH  4
#define BRC_INF_TRUNCATED     5   /* the payload ends inside the stream */

typedef struct brc_inflater brc_inflater;

/* (the bgzf handle samopen creates, bamreadcount.cpp:513) One inflater per device; BRC_E_NODEVICE without a GPU — the product
 * library has no CPU path.  Its copies and launches run on a stream of its own, so a call overlaps whatever an engine of the same
 * process computes.  Calls on one handle are serialised; several handles may be alive and used side by side. */
int  brc_inflater_create(int device, brc_inflater** out);
void brc_inflater_destroy(brc_inflater* h);
/* "hip-gfx950" | "sim" */
const char* brc_inflater_kind(void);
const char* brc_inflater_last_error(const brc_inflater* h);

/* (bgzf_read's block loop under samfetch, bamreadcount.cpp:602) src[0, src_len): whole BGZF members back to back (gzip header with
 * the BC subfield ... CRC32, ISIZE).  The host walks the BSIZE chain and reads each ISIZE.
 *   *n_members  in: the capacity of status[] (dst_off[] has one entry more); out: the members found.
 *   dst_off[i]  prefix sum of ISIZE: member i's bytes are dst[dst_off[i], dst_off[i + 1]); a BAD_HEADER member takes no room.
 *   status[i]   BRC_INF_*; the slot of a member that failed is left as it was (nothing partial is written).  Payload bytes behind
 *               the final deflate block are ignored: ISIZE and CRC32 decide, the member is ok (as with both of htslib's back ends).
 * Returns BRC_OK when the call itself ran, whatever the members' statuses.  BRC_E_ARG: dst_cap is below dst_off[n] or the
 * capacity below n (both are still reported, nothing is inflated), or src is not a chain of whole members — a header without
 * magic or BC subfield, a BSIZE that points beyond src: the whole members in front of it are inflated and reported as usual. */
int  brc_inflate_bgzf(brc_inflater* h, const void* src, size_t src_len, void* dst, size_t dst_cap,
                      uint64_t* dst_off, uint8_t* status, size_t* n_members);

/* Page-locked host memory (the brc_host_alloc idiom of include/brc.h): src / dst that lie in it are copied by the device straight
 * from / to where they are; any other memory goes through the handle's own staging.  NULL when none can be had. */
void* brc_inflate_host_alloc(size_t bytes);
void  brc_inflate_host_free(void* p);

/* The last call's account: seconds between the events around the kernel launch, seconds of the whole call (chain walk, H2D, kernel,
 * D2H), bytes in and out.  (tools/inflate_bench.py, BRC_CLI_TIMING) */
void brc_inflater_last_timing(const brc_inflater* h, double* kernel_s, double* call_s, uint64_t* bytes_in, uint64_t* bytes_out);

#ifdef __cplusplus
}
#endif
#endif
