// brc_select.hip — device-side site selection for gfx950 behind the C-ABI of include/brc_select.h (libbrc_select_hip.so; a translation
// unit and a library of its own: the engine's libraries keep exactly the device code they had, and this one links nothing of the engine).
//
// Per call, on the caller's stream:
//   memset head, flag | k_select_link | k_select_flag | k_select_why | k_select_parts | k_select_emit
//   k_select_link   lane == third-allele record: pushes itself onto its position's list (only when the view has records)
//   k_select_flag   lane == indel record: ORs its candidate / veto bit into its position's flag word (only when indels are asked for)
//   k_select_why    lane == position, wave == 64 consecutive positions: four plane loads per library, each one run of 256 bytes per
//                   wave; the reason word goes to the scratch, the workgroup's count of non-zero ones (ballots) to part[]
//   k_select_parts  ONE workgroup: part[] -> its exclusive scan, the total -> counts[0]
//   k_select_emit   lane == position: reason word back from the scratch, ballot + the waves' counts -> its place; idx / why stores
// This is the reduce-then-scan of brc_indels.hip: no workgroup ever waits for another, the launches' order on the stream is the only
// dependency, and every launch is sized by n — the host never learns the count.  A call that wants the count alone ends after
// k_select_parts.  The per-lane work is brc_select_core.h, shared with the CPU build the tests run.  DESIGN.md 6f has the reasoning.
#include <hip/hip_runtime.h>

#include "brc_select_core.h"
#include "brc_side_hip.h"

using namespace brcselect;

__global__ __launch_bounds__(BLOCK) void k_select_link(const Job J) {
    const uint64_t r = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (r < J.n_xagg) link_lane(J, r);
}
__global__ __launch_bounds__(BLOCK) void k_select_flag(const Job J) {
    const uint64_t s = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s < J.n_slots) flag_lane(J, s);
}

// selected lanes of the wave, and of them those in front of this lane
__device__ inline uint32_t wave_rank(bool sel, uint32_t& total) {
    const unsigned long long m = __ballot(sel);
    total = (uint32_t)__popcll(m);
    return (uint32_t)__popcll(m & ((1ull << (threadIdx.x & (WAVE - 1))) - 1ull));
}

__global__ __launch_bounds__(BLOCK) void k_select_why(const Job J) {
    __shared__ uint32_t wsum[BLOCK / WAVE];
    const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t why = j < J.n ? why_lane(J, j) : 0u;
    uint32_t total;
    (void)wave_rank(why != 0u, total);
    if ((threadIdx.x & (WAVE - 1)) == 0) wsum[threadIdx.x / WAVE] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int w = 0; w < BLOCK / WAVE; ++w) s += wsum[w];
        J.part[blockIdx.x] = s;
    }
}

// exclusive scan of one value per lane over the workgroup (Hillis-Steele in LDS: 8 steps for 256 lanes); total = the workgroup's sum
__device__ inline uint32_t block_scan(uint32_t v, uint32_t* sh, uint32_t& total) {
    const unsigned t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (unsigned d = 1; d < BLOCK; d <<= 1) {
        const uint32_t x = t >= d ? sh[t - d] : 0u;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    const uint32_t incl = sh[t];
    total = sh[BLOCK - 1];
    __syncthreads();
    return incl - v;
}
// ONE workgroup: part[0 .. nb) -> its exclusive scan, BLOCK partials at a time with a running carry; the total to the scratch and the caller
__global__ __launch_bounds__(BLOCK) void k_select_parts(const Job J, uint64_t nb) {
    __shared__ uint32_t sh[BLOCK];
    uint32_t carry = 0;
    for (uint64_t base = 0; base < nb; base += BLOCK) {
        const uint64_t i = base + threadIdx.x;
        const uint32_t v = i < nb ? J.part[i] : 0u;
        uint32_t total;
        const uint32_t ex = block_scan(v, sh, total);
        if (i < nb) J.part[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) { *J.tot = carry; if (J.o_counts) *J.o_counts = carry; }
}

__global__ __launch_bounds__(BLOCK) void k_select_emit(const Job J) {
    __shared__ uint32_t wsum[BLOCK / WAVE];
    const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t why = j < J.n ? J.flag[j] : 0u;
    uint32_t total;
    const uint32_t rank = wave_rank(why != 0u, total);
    if ((threadIdx.x & (WAVE - 1)) == 0) wsum[threadIdx.x / WAVE] = total;
    __syncthreads();
    uint64_t at = (uint64_t)J.part[blockIdx.x] + rank;
    for (unsigned w = 0; w < threadIdx.x / WAVE; ++w) at += wsum[w];
    emit_lane(J, j, why, at);
}

struct brc_select : brcside::Handle {};

extern "C" {

const char* brc_select_kind(void) { return "hip-gfx950"; }
int brc_select_create(int device, brc_select** out) { return brcside::create(device, (const void*)k_select_why, out); }
void brc_select_destroy(brc_select* h) { brcside::destroy(h); }
const char* brc_select_last_error(const brc_select* h) { return brcside::last_error(h); }
void brc_select_last_timing(const brc_select* h, double* kernel_s, uint64_t* bytes_read, uint64_t* bytes_written) { brcside::last_timing(h, kernel_s, bytes_read, bytes_written); }
int64_t brc_select_workspace(const brc_device_view* v, const brc_device_indels*, int64_t n) { return workspace_bytes(v, n); }

int brc_select_sites(brc_select* h, const brc_device_view* v, const brc_device_indels* d, const brc_select_params* p, int64_t k0, int64_t n, int64_t cap,
                     int32_t* idx, uint32_t* why_, uint32_t* counts, void* workspace, void* stream_) {
    if (!h) return BRC_E_ARG;
    brcside::clear(h);
    const char* why = "";
    if (check_job(v, d, p, k0, n, cap, workspace, &why)) return brcside::refuse(h, why);
    if (int rc = brcside::resident(h, v, brcside::TWO_VIEWS)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    HIPOK(hipSetDevice(h->device));
    if (n == 0) {
        if (counts) HIPOK(hipMemsetAsync(counts, 0, sizeof(uint32_t), stream));
        return BRC_OK;
    }
    const Job J = make_job(v, d, p, k0, n, cap, idx, why_, counts, workspace);
    if (!counts && !wants_list(J)) return BRC_OK;
    const unsigned nb = (unsigned)blocks_of((uint64_t)n);
    if (int rc = brcside::start(h, stream)) return rc;
    if (walks_records(J)) {
        HIPOK(hipMemsetAsync(J.head, 0xff, (size_t)n * sizeof(uint32_t), stream));
        LAUNCH(k_select_link, dim3((unsigned)blocks_of(J.n_xagg)), dim3(BLOCK), 0, stream, J);
    }
    if (walks_slots(J)) {
        HIPOK(hipMemsetAsync(J.flag, 0, (size_t)n * sizeof(uint32_t), stream));
        LAUNCH(k_select_flag, dim3((unsigned)blocks_of(J.n_slots)), dim3(BLOCK), 0, stream, J);
    }
    LAUNCH(k_select_why, dim3(nb), dim3(BLOCK), 0, stream, J);
    LAUNCH(k_select_parts, dim3(1), dim3(BLOCK), 0, stream, J, (uint64_t)nb);
    if (wants_list(J)) LAUNCH(k_select_emit, dim3(nb), dim3(BLOCK), 0, stream, J);
    return brcside::done(h, stream, J);
}

}  // extern "C"
