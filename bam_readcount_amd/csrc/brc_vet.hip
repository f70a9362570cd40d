// brc_vet.hip — device-side candidate filter for gfx950 behind the C-ABI of include/brc_vet.h (libbrc_vet_hip.so; a translation unit and
// a library of its own: the engine's libraries keep exactly the device code they had, and this one links nothing of the engine).
//
// Per call, on the caller's stream: the status word's clear, then
//   memset head | k_vet_link   lane == third-allele record: a binary search over idx, then itself onto the list of the first element that
//                              lists its position.  Only when the view has records and a destination is wanted.
//   k_vet_sites                lane == list element j, wave == 64 consecutive elements: one coalesced load of idx[j] and alt[j], the
//                              reference byte, then per library the 28 plane loads of the dense expansion at that index (listed
//                              neighbours share their cache lines, an isolated site pays a line per word), the four base buckets'
//                              tested columns, the tests, and the stores at j: every store of a wave is one run of 256 contiguous
//                              bytes, non-temporal.  keep is the lane's OR over its loop of libraries.  No LDS.
// No workgroup ever waits for another, the launches' order on the stream is the only dependency, and every launch is sized by n or
// n_xagg.  The per-lane work is brc_vet_core.h, shared with the CPU build the tests run.  DESIGN.md 6j has the reasoning.
#include <hip/hip_runtime.h>

#include "brc_vet_core.h"
#include "brc_side_hip.h"

using namespace brcvet;

__global__ __launch_bounds__(BLOCK) void k_vet_link(const Job J) {
    const uint64_t r = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (r < J.n_xagg) link_lane(J, r);
}

__global__ __launch_bounds__(BLOCK) void k_vet_sites(const Job J) {
    const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j < J.n) sites_lane(J, j);
}

struct brc_vet : brcside::Handle {};

extern "C" {

const char* brc_vet_kind(void) { return "hip-gfx950"; }
int brc_vet_create(int device, brc_vet** out) { return brcside::create(device, (const void*)k_vet_sites, out); }
void brc_vet_destroy(brc_vet* h) { brcside::destroy(h); }
const char* brc_vet_last_error(const brc_vet* h) { return brcside::last_error(h); }
void brc_vet_last_timing(const brc_vet* h, double* kernel_s, uint64_t* bytes_read, uint64_t* bytes_written) { brcside::last_timing(h, kernel_s, bytes_read, bytes_written); }
int64_t brc_vet_workspace(const brc_device_view* v, int64_t n) { return workspace_bytes(v, n); }

int brc_vet_sites(brc_vet* h, const brc_device_view* v, const brc_device_indels* d, const brc_vet_params* p, const int32_t* idx, const uint32_t* alt, int64_t n,
                  int64_t dst_stride, uint32_t* fail, uint32_t* keep, float* vals, uint32_t* status, void* workspace, void* stream_) {
    if (!h) return BRC_E_ARG;
    brcside::clear(h);
    const char* why = "";
    if (check_job(v, d, p, idx, n, dst_stride, workspace, &why)) return brcside::refuse(h, why);
    if (int rc = brcside::resident(h, v, brcside::TWO_VIEWS)) return rc;
    const bool dests = fail || keep || vals;
    if (!status && (n == 0 || !dests)) return BRC_OK;
    hipStream_t stream = (hipStream_t)stream_;
    HIPOK(hipSetDevice(h->device));
    if (status) HIPOK(hipMemsetAsync(status, 0, sizeof(uint32_t), stream));
    if (n == 0) return BRC_OK;
    const Job J = make_job(v, d, p, idx, alt, n, dst_stride, fail, keep, vals, status, workspace);
    if (int rc = brcside::start(h, stream)) return rc;
    if (walks_records(J)) {
        HIPOK(hipMemsetAsync(J.head, 0xff, (size_t)n * sizeof(uint32_t), stream));
        LAUNCH(k_vet_link, dim3((unsigned)blocks_of(J.n_xagg)), dim3(BLOCK), 0, stream, J);
    }
    LAUNCH(k_vet_sites, dim3((unsigned)blocks_of((uint64_t)n)), dim3(BLOCK), 0, stream, J);
    return brcside::done(h, stream, J);
}

}  // extern "C"
