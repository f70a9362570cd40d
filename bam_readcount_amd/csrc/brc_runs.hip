// brc_runs.hip — device-side depth-class intervals for gfx950 behind the C-ABI of include/brc_runs.h (libbrc_runs_hip.so; a translation
// unit and a library of its own: the engine's libraries keep exactly the device code they had, and this one links nothing of the engine).
//
// Per call, on the caller's stream:
//   memset per_class | k_runs_class | k_runs_parts | k_runs_emit
//   k_runs_class   lane == position, wave == 64 consecutive positions: one depth word per counted library, each load of a wave one run
//                  of 256 bytes; the class goes to the scratch and, with the two positions next to the workgroup (recomputed by one lane
//                  each, of two different waves), into LDS: 256 + 2 words.  A lane compares its class with its neighbours'; the
//                  workgroup's emitted starts and emitted ends are counted with two ballots per wave.  per_class: one ballot per class,
//                  lane c keeps the count of class c, one 64-bit atomic add per non-zero class and wave
//   k_runs_parts   ONE workgroup: the workgroups' two counts, packed into one 64-bit word -> their exclusive scans, 256 per pass with
//                  a carry; the total of starts -> counts[0]
//   k_runs_emit    lane == position: its class and its neighbours' back from the scratch, two ballot ranks + the waves' counts + the
//                  workgroup's two offsets -> start / cls at the start rank, end at the end rank
// This is the reduce-then-scan of brc_select.hip: no look-back, no flags, no workgroup ever waits for another, the launches' order on
// the stream is the only dependency, every launch is sized by n and every loop is bounded by n, n_lib or n_cut.  A call that wants
// counts / per_class alone ends after k_runs_parts.  The per-lane work is brc_runs_core.h, shared with the CPU build the tests run.
// DESIGN.md 6h has the reasoning.
#include <hip/hip_runtime.h>

#include "brc_runs_core.h"
#include "brc_side_hip.h"

using namespace brcruns;

// set lanes of the wave, and of them those in front of this lane
__device__ inline uint32_t wave_rank(bool set, uint32_t& total) {
    const unsigned long long m = __ballot(set);
    total = (uint32_t)__popcll(m);
    return (uint32_t)__popcll(m & ((1ull << (threadIdx.x & (WAVE - 1))) - 1ull));
}

__global__ __launch_bounds__(BLOCK) void k_runs_class(const Job J, int ranks) {
    __shared__ uint32_t sh[BLOCK + 2];                                  // sh[t + 1]: the class of lane t; sh[0], sh[BLOCK + 1]: the halo
    __shared__ uint32_t wsum[BLOCK / WAVE][2];
    const unsigned t = threadIdx.x, lane = t & (WAVE - 1);
    const int64_t j0 = (int64_t)blockIdx.x * BLOCK, j = j0 + t;
    const bool in = j < J.n;
    const uint32_t c = in ? class_lane(J, j) : NO_CLASS;
    if (in) J.w_cls[j] = c;
    if (J.o_per) {
        uint32_t mine = 0u;
        for (uint32_t x = 0; x < n_class(J); ++x) {                     // (uniform: n_cut is a kernel argument)
            const uint32_t cnt = (uint32_t)__popcll(__ballot(c == x));
            if (lane == x) mine = cnt;
        }
        if (lane < n_class(J) && mine) add64(J.o_per + lane, mine);
    }
    if (!ranks) return;                                                 // (uniform)
    sh[t + 1] = c;
    if (t == 0) sh[0] = j0 > 0 ? class_lane(J, j0 - 1) : NO_CLASS;
    if (t == WAVE) sh[BLOCK + 1] = j0 + BLOCK < J.n ? class_lane(J, j0 + BLOCK) : NO_CLASS;
    __syncthreads();
    uint32_t ns, ne;
    (void)wave_rank(starts_run(J, sh[t], c), ns);
    (void)wave_rank(ends_run(J, c, sh[t + 2]), ne);
    if (lane == 0) { wsum[t / WAVE][0] = ns; wsum[t / WAVE][1] = ne; }
    __syncthreads();
    if (t == 0) {
        uint32_t s = 0, e = 0;
        for (int w = 0; w < BLOCK / WAVE; ++w) { s += wsum[w][0]; e += wsum[w][1]; }
        J.part_s[blockIdx.x] = s; J.part_e[blockIdx.x] = e;
    }
}

// exclusive scan of one value per lane over the workgroup (Hillis-Steele in LDS: 8 steps for 256 lanes); total = the workgroup's sum
__device__ inline uint64_t block_scan(uint64_t v, uint64_t* sh, uint64_t& total) {
    const unsigned t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (unsigned d = 1; d < BLOCK; d <<= 1) {
        const uint64_t x = t >= d ? sh[t - d] : 0u;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    const uint64_t incl = sh[t];
    total = sh[BLOCK - 1];
    __syncthreads();
    return incl - v;
}
// ONE workgroup: part_s / part_e [0 .. nb) -> their exclusive scans, BLOCK pairs at a time with a running carry; the total to the caller
__global__ __launch_bounds__(BLOCK) void k_runs_parts(const Job J, uint64_t nb) {
    __shared__ uint64_t sh[BLOCK];
    uint64_t carry = 0;
    for (uint64_t base = 0; base < nb; base += BLOCK) {
        const uint64_t i = base + threadIdx.x;
        const uint64_t v = i < nb ? pack(J.part_s[i], J.part_e[i]) : 0u;
        uint64_t total;
        const uint64_t ex = carry + block_scan(v, sh, total);
        if (i < nb) { J.part_s[i] = starts_of(ex); J.part_e[i] = ends_of(ex); }
        carry += total;
    }
    if (threadIdx.x == 0 && J.o_counts) *J.o_counts = starts_of(carry);
}

__global__ __launch_bounds__(BLOCK) void k_runs_emit(const Job J) {
    __shared__ uint32_t wsum[BLOCK / WAVE][2];
    const unsigned t = threadIdx.x;
    const int64_t j = (int64_t)blockIdx.x * BLOCK + t;
    const bool in = j < J.n;
    const uint32_t c = in ? J.w_cls[j] : NO_CLASS;
    const uint32_t left = in && j > 0 ? J.w_cls[j - 1] : NO_CLASS, right = in && j + 1 < J.n ? J.w_cls[j + 1] : NO_CLASS;
    const bool is_start = starts_run(J, left, c), is_end = ends_run(J, c, right);
    uint32_t ns, ne;
    const uint32_t rs = wave_rank(is_start, ns), re = wave_rank(is_end, ne);
    if ((t & (WAVE - 1)) == 0) { wsum[t / WAVE][0] = ns; wsum[t / WAVE][1] = ne; }
    __syncthreads();
    uint64_t at_s = (uint64_t)J.part_s[blockIdx.x] + rs, at_e = (uint64_t)J.part_e[blockIdx.x] + re;
    for (unsigned w = 0; w < t / WAVE; ++w) { at_s += wsum[w][0]; at_e += wsum[w][1]; }
    if (in) emit_lane(J, j, c, is_start, at_s, is_end, at_e);
}

struct brc_runs : brcside::Handle {};

extern "C" {

const char* brc_runs_kind(void) { return "hip-gfx950"; }
int brc_runs_create(int device, brc_runs** out) { return brcside::create(device, (const void*)k_runs_class, out); }
void brc_runs_destroy(brc_runs* h) { brcside::destroy(h); }
const char* brc_runs_last_error(const brc_runs* h) { return brcside::last_error(h); }
void brc_runs_last_timing(const brc_runs* h, double* kernel_s, uint64_t* bytes_read, uint64_t* bytes_written) { brcside::last_timing(h, kernel_s, bytes_read, bytes_written); }
int64_t brc_runs_workspace(int64_t n) { return workspace_bytes(n); }

int brc_runs_find(brc_runs* h, const brc_device_view* v, const brc_device_indels* d, const brc_runs_params* p, int64_t k0, int64_t n, int64_t cap,
                  int32_t* start, int32_t* end, uint32_t* cls, uint32_t* counts, uint64_t* per_class, void* workspace, void* stream_) {
    if (!h) return BRC_E_ARG;
    brcside::clear(h);
    const char* why = "";
    if (check_job(v, d, p, k0, n, cap, workspace, &why)) return brcside::refuse(h, why);
    if (int rc = brcside::resident(h, v, d ? brcside::TWO_VIEWS : brcside::ONE_VIEW)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    HIPOK(hipSetDevice(h->device));
    const Job J = make_job(v, d, p, k0, n, cap, start, end, cls, counts, per_class, workspace);
    if (n == 0) {
        if (counts) HIPOK(hipMemsetAsync(counts, 0, sizeof(uint32_t), stream));
        if (per_class) HIPOK(hipMemsetAsync(per_class, 0, n_class(J) * sizeof(uint64_t), stream));
        return BRC_OK;
    }
    if (!per_class && !wants_ranks(J)) return BRC_OK;
    const unsigned nb = (unsigned)blocks_of((uint64_t)n);
    if (int rc = brcside::start(h, stream)) return rc;
    if (per_class) HIPOK(hipMemsetAsync(per_class, 0, n_class(J) * sizeof(uint64_t), stream));
    LAUNCH(k_runs_class, dim3(nb), dim3(BLOCK), 0, stream, J, wants_ranks(J) ? 1 : 0);
    if (wants_ranks(J)) LAUNCH(k_runs_parts, dim3(1), dim3(BLOCK), 0, stream, J, (uint64_t)nb);
    if (wants_list(J)) LAUNCH(k_runs_emit, dim3(nb), dim3(BLOCK), 0, stream, J);
    return brcside::done(h, stream, J);
}

}  // extern "C"
