// brc_bins.hip — device-side window summaries for gfx950 behind the C-ABI of include/brc_bins.h (libbrc_bins_hip.so; a translation unit
// and a library of its own: the engine's libraries keep exactly the device code they had, and this one links nothing of the engine).
//
// Per call, on the caller's stream:
//   k_bins_clear | k_bins_edges | k_bins_planes | k_bins_records | k_bins_indels
//   k_bins_clear    lane == destination element (grid-stride): the n_bins elements of every wanted row, the histogram, the status word
//   k_bins_edges    lane == edge of an edge list: the status bits (only with an edge list)
//   k_bins_planes   lane == position, wave == 64 consecutive positions, blockIdx.y == library: every plane load of a wave is one run of
//                   256 bytes.  A wave whose positions share one bin — every wave of a bin of 64 positions or more that does not hold an
//                   edge — reduces its nine sums across the lanes with a reduce-scatter (17 exchanges instead of 54), the maximum with a
//                   butterfly, the thresholds with one ballot each, and issues ONE 64-bit atomic per non-zero value; a wave that holds
//                   an edge lets every lane add its own non-zero values.  The depth histogram is counted in LDS per workgroup and
//                   flushed with one 64-bit atomic per non-zero bar
//   k_bins_records  lane == third-allele record: corrects its bucket's sum in its bin (only when the view has records)
//   k_bins_indels   lane == indel record: its reads into the insertion / deletion sum of its bin (only when there are records)
// No workgroup ever waits for another; the launches' order on the stream is the only dependency — and of it only "clear first" matters:
// everything behind is an integer add, maximum or OR.  No scratch memory.  The per-lane work is brc_bins_core.h, shared with the CPU
// build the tests run.  DESIGN.md 6g has the reasoning.
#include <hip/hip_runtime.h>

#include "brc_bins_core.h"
#include "brc_side_hip.h"

using namespace brcbins;

enum { CLEAR_BLOCKS = 4096 };

__global__ __launch_bounds__(BLOCK) void k_bins_clear(const Job J) {
    const uint64_t total = clear_total(J);
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < total; i += (uint64_t)gridDim.x * BLOCK) clear_lane(J, i);
}
__global__ __launch_bounds__(BLOCK) void k_bins_edges(const Job J) {
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i <= (uint64_t)J.n_bins) edge_lane(J, i);
}
__global__ __launch_bounds__(BLOCK) void k_bins_records(const Job J) {
    const uint64_t r = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (r < J.n_xagg) record_lane(J, r);
}
__global__ __launch_bounds__(BLOCK) void k_bins_indels(const Job J) {
    const uint64_t s = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s < J.n_slots) indel_lane(J, s);
}

__device__ inline uint64_t xor64(uint64_t v, int m) { return (uint64_t)__shfl_xor((unsigned long long)v, m, WAVE); }

// The wave's 64 positions lie in ONE bin: their values summed across the lanes, one atomic per non-zero value.
// Reduce-scatter over 16 slots (the nine sums, seven zeros the compiler folds): the lanes exchange across bit 32, 16, 8, 4 of the lane
// number and halve the slots they keep each time, so a lane ends with one slot summed over the 16 lanes that share its bits 0 and 1;
// two more exchanges complete it.  Slot of lane x: bit 5 -> 8, bit 4 -> 4, bit 3 -> 2, bit 2 -> 1.
__device__ inline void wave_commit(const Job& J, int l, int64_t bin, const Lane& o, bool in) {
    const unsigned lane = threadIdx.x & (WAVE - 1);
    if (wants_sums(J)) {
        uint64_t v[8];
        {   // first exchange on the 32-bit values a lane starts with
            const bool up = lane & 32u;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const uint32_t a = i < NADD ? o.add[i] : 0u, b = i + 8 < NADD ? o.add[i + 8] : 0u;
                const uint32_t keep = up ? b : a, send = up ? a : b;
                v[i] = (uint64_t)keep + (uint64_t)(uint32_t)__shfl_xor(send, 32, WAVE);
            }
        }
#pragma unroll
        for (int h = 4; h >= 1; h >>= 1) {
            const int m = h * 4;                                       // 16, 8, 4
            const bool up = lane & (unsigned)m;
#pragma unroll
            for (int i = 0; i < h; ++i) {
                const uint64_t keep = up ? v[i + h] : v[i], send = up ? v[i] : v[i + h];
                v[i] = keep + xor64(send, m);
            }
        }
        v[0] += xor64(v[0], 2);
        v[0] += xor64(v[0], 1);
        const unsigned slot = ((lane >> 5) & 1u) * 8u + ((lane >> 4) & 1u) * 4u + ((lane >> 3) & 1u) * 2u + ((lane >> 2) & 1u);
        uint64_t* base = J.o_sums + ((int64_t)l * NSUM) * J.DS + bin;
        if ((lane & 3u) == 0u && slot < (unsigned)NADD && v[0]) add64(base + (int64_t)slot * J.DS, v[0]);
        uint32_t mx = o.depth;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) { const uint32_t x = (uint32_t)__shfl_xor(mx, m, WAVE); mx = x > mx ? x : mx; }
        if (lane == 0u && mx) max64(base + (int64_t)BRC_BINS_S_MAXDEPTH * J.DS, mx);
    }
    if (wants_cov(J)) {
        uint32_t mine = 0u;
        for (int t = 0; t < J.n_thr; ++t) {                             // (uniform: the thresholds are kernel arguments)
            const uint32_t c = (uint32_t)__popcll(__ballot(in && o.depth >= J.thr[t]));
            if (lane == (unsigned)t) mine = c;
        }
        if (lane < (unsigned)J.n_thr && mine) add64(J.o_cov + ((int64_t)l * J.n_thr + lane) * J.DS + bin, mine);
    }
}

__global__ __launch_bounds__(BLOCK) void k_bins_planes(const Job J) {
    extern __shared__ uint32_t bars[];                                  // n_hist words when the histogram is wanted
    const int l = (int)blockIdx.y;
    const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool hist = wants_hist(J), in = j < J.n;
    if (hist) {
        for (int i = (int)threadIdx.x; i < J.n_hist; i += BLOCK) bars[i] = 0u;
        __syncthreads();
    }
    Lane o;
    o.bin = -1; o.depth = 0u;
#pragma unroll
    for (int s = 0; s < NADD; ++s) o.add[s] = 0u;
    if (in) o = plane_lane(J, l, j);
    if (hist && o.bin >= 0) atomicAdd(&bars[hist_bar(J, o.depth)], 1u);
    if (wants_sums(J) || wants_cov(J)) {
        // lane 0 of a wave is inside the window whenever any of its lanes is: the positions ascend with the lanes
        const int64_t bin0 = (int64_t)__shfl((long long)o.bin, 0, WAVE);
        if (__all(!in || o.bin == bin0)) {
            if (bin0 >= 0) wave_commit(J, l, bin0, o, in);
        } else {
            commit_lane(J, l, o);
        }
    }
    if (hist) {
        __syncthreads();
        for (int i = (int)threadIdx.x; i < J.n_hist; i += BLOCK) {
            const uint32_t c = bars[i];
            if (c) add64(J.o_hist + (int64_t)l * J.n_hist + i, c);
        }
    }
}

struct brc_bins : brcside::Handle {};

extern "C" {

const char* brc_bins_kind(void) { return "hip-gfx950"; }
int brc_bins_create(int device, brc_bins** out) { return brcside::create(device, (const void*)k_bins_planes, out); }
void brc_bins_destroy(brc_bins* h) { brcside::destroy(h); }
const char* brc_bins_last_error(const brc_bins* h) { return brcside::last_error(h); }
void brc_bins_last_timing(const brc_bins* h, double* kernel_s, uint64_t* bytes_read, uint64_t* bytes_written) { brcside::last_timing(h, kernel_s, bytes_read, bytes_written); }

int brc_bins_reduce(brc_bins* h, const brc_device_view* v, const brc_device_indels* d, const brc_bins_params* p, int64_t k0, int64_t n,
                    uint64_t* sums, uint64_t* covered, uint64_t* hist, int64_t dst_stride, uint32_t* status, void* stream_) {
    if (!h) return BRC_E_ARG;
    brcside::clear(h);
    const char* why = "";
    if (check_job(v, d, p, k0, n, dst_stride, &why)) return brcside::refuse(h, why);
    if (int rc = brcside::resident(h, v, brcside::TWO_VIEWS)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    HIPOK(hipSetDevice(h->device));
    const Job J = make_job(v, d, p, k0, n, dst_stride, sums, covered, hist, status);
    if (!wants_sums(J) && !wants_cov(J) && !wants_hist(J) && !status) return BRC_OK;
    if (int rc = brcside::start(h, stream)) return rc;
    const uint64_t cb = blocks_of(clear_total(J));
    LAUNCH(k_bins_clear, dim3((unsigned)(cb < CLEAR_BLOCKS ? cb : CLEAR_BLOCKS)), dim3(BLOCK), 0, stream, J);
    if (J.edges && status) LAUNCH(k_bins_edges, dim3((unsigned)blocks_of((uint64_t)J.n_bins + 1u)), dim3(BLOCK), 0, stream, J);
    if (sweeps(J)) {
        LAUNCH(k_bins_planes, dim3((unsigned)blocks_of((uint64_t)n), (unsigned)J.Lp), dim3(BLOCK), wants_hist(J) ? (size_t)J.n_hist * sizeof(uint32_t) : 0, stream, J);
        if (walks_records(J)) LAUNCH(k_bins_records, dim3((unsigned)blocks_of(J.n_xagg)), dim3(BLOCK), 0, stream, J);
        if (walks_slots(J)) LAUNCH(k_bins_indels, dim3((unsigned)blocks_of(J.n_slots)), dim3(BLOCK), 0, stream, J);
    }
    return brcside::done(h, stream, J);
}

}  // extern "C"
