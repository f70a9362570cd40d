// brc_ivet.hip — device-side indel candidate filter for gfx950 behind the C-ABI of include/brc_ivet.h (libbrc_ivet_hip.so; a translation
// unit and a library of its own: the engine's libraries and its siblings keep exactly the device code they had, and this one links
// none of them).
//
// Per call, on the caller's stream: the status word's clear and keep's clear, then
//   memset head | k_ivet_link   lane == third-allele record: a binary search over the table's pos, then itself onto the list of the first
//                               record of its position.  Only when the view has records and a destination is wanted.
//   k_ivet_records              lane i < m == table record i, wave == 64 consecutive records, block == 256: coalesced loads of pos, lib,
//                               len, the 13 sums and the two offsets; the reference byte and the 28 plane words of the dense expansion at
//                               (lib, pos - pos0) (the records of a run share their cache lines); the SNV filter's tests
//                               (brc_vet_core.h's judge); the control depths; the walk over the run, left and right of the record; the
//                               stores at i — every store of a wave is one run of 256 contiguous bytes, non-temporal — and an atomic OR
//                               into keep at the list elements a binary search finds.  Lane i < n also checks list element i.  No LDS.
// No workgroup ever waits for another, the launches' order on the stream is the only dependency, and every launch is sized by m, n
// or n_xagg.  The per-lane work is brc_ivet_core.h, shared with the CPU build the tests run.  DESIGN.md 6k has the reasoning.
#include <hip/hip_runtime.h>

#include "brc_ivet_core.h"
#include "brc_side_hip.h"

using namespace brcivet;

__global__ __launch_bounds__(BLOCK) void k_ivet_link(const Job J) {
    const uint64_t r = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (r < J.V.n_xagg) link_lane(J, r);
}

__global__ __launch_bounds__(BLOCK) void k_ivet_records(const Job J) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i < J.n) list_lane(J, i);
    if (i < J.m) record_lane(J, i);
}

struct brc_ivet : brcside::Handle {};

extern "C" {

const char* brc_ivet_kind(void) { return "hip-gfx950"; }
int brc_ivet_create(int device, brc_ivet** out) { return brcside::create(device, (const void*)k_ivet_records, out); }
void brc_ivet_destroy(brc_ivet* h) { brcside::destroy(h); }
const char* brc_ivet_last_error(const brc_ivet* h) { return brcside::last_error(h); }
void brc_ivet_last_timing(const brc_ivet* h, double* kernel_s, uint64_t* bytes_read, uint64_t* bytes_written) { brcside::last_timing(h, kernel_s, bytes_read, bytes_written); }
int64_t brc_ivet_workspace(const brc_device_view* v, int64_t m) { return workspace_bytes(v, m); }

int brc_ivet_records(brc_ivet* h, const brc_device_view* v, const brc_device_indels* d, const brc_ivet_params* p, const brc_ivet_table* t, const int32_t* idx,
                     const uint32_t* why, int64_t n, int64_t dst_stride, uint32_t* fail, float* vals, uint32_t* ctl_count, uint32_t* keep, uint32_t* status,
                     void* workspace, void* stream_) {
    if (!h) return BRC_E_ARG;
    brcside::clear(h);
    const char* said = "";
    if (check_job(v, d, p, t, idx, n, dst_stride, workspace, &said)) return brcside::refuse(h, said);
    if (int rc = brcside::resident(h, v, brcside::TWO_VIEWS)) return rc;
    const Job J = make_job(v, d, p, t, idx, why, n, dst_stride, fail, vals, ctl_count, keep, status, workspace);
    if (!status && !(keep && n > 0) && !(wants_dests(J) && J.m > 0)) return BRC_OK;
    hipStream_t stream = (hipStream_t)stream_;
    HIPOK(hipSetDevice(h->device));
    if (status) HIPOK(hipMemsetAsync(status, 0, sizeof(uint32_t), stream));
    if (keep && n > 0) HIPOK(hipMemsetAsync(keep, 0, (size_t)n * sizeof(uint32_t), stream));
    const bool lanes = (status && lanes_of(J) > 0) || (wants_dests(J) && J.m > 0);
    if (!lanes) return BRC_OK;
    if (int rc = brcside::start(h, stream)) return rc;
    if (walks_records(J)) {
        HIPOK(hipMemsetAsync(J.V.head, 0xff, (size_t)J.m * sizeof(uint32_t), stream));
        LAUNCH(k_ivet_link, dim3((unsigned)blocks_of(J.V.n_xagg)), dim3(BLOCK), 0, stream, J);
    }
    LAUNCH(k_ivet_records, dim3((unsigned)blocks_of(lanes_of(J))), dim3(BLOCK), 0, stream, J);
    return brcside::done(h, stream, J);
}

}  // extern "C"
