// brc_side_scan.h — an exclusive scan of 32-bit words on the caller's stream, for the gfx950 side libraries whose sizes are data:
// reduce-then-scan in three launches — every workgroup's sum, ONE workgroup scanning the sums, every workgroup scanning its tile onto
// its sum — so no workgroup ever waits for another: the launches' order on the stream is the only dependency.  The element count is
// the host's (n_host, which sizes the launches) or, where the host does not know it, a word in device memory that never exceeds it.
// Include it behind brc_side_hip.h (HIPOK, LAUNCH).  brc_indels.hip carries the same three kernels of its own.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace brcside {

enum { SCAN_BLOCK = 256 };       // four waves: elements per workgroup of a scan

// exclusive scan of one value per lane over the workgroup (Hillis-Steele in LDS: 8 steps for 256 lanes); total = the workgroup's sum
__device__ inline uint32_t block_scan(uint32_t v, uint32_t* sh, uint32_t& total) {
    const unsigned t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (unsigned d = 1; d < SCAN_BLOCK; d <<= 1) {
        const uint32_t x = t >= d ? sh[t - d] : 0u;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    const uint32_t incl = sh[t];
    total = sh[SCAN_BLOCK - 1];
    __syncthreads();
    return incl - v;
}
// elements of a scan: n_host, or the device-side count (never above n_host: the launch is sized by it)
__device__ inline uint64_t scan_count(const uint32_t* n_dev, uint64_t n_host) {
    if (!n_dev) return n_host;
    const uint64_t c = *n_dev;
    return c < n_host ? c : n_host;
}

}  // namespace brcside

// 1. part[b] = sum of tile b (0 for a tile behind the count)
__global__ __launch_bounds__(brcside::SCAN_BLOCK) void k_side_scan_reduce(const uint32_t* __restrict__ in, const uint32_t* n_dev, uint64_t n_host,
                                                                           uint32_t* __restrict__ part) {
    __shared__ uint32_t sh[brcside::SCAN_BLOCK];
    const uint64_t count = brcside::scan_count(n_dev, n_host), i = (uint64_t)blockIdx.x * brcside::SCAN_BLOCK + threadIdx.x;
    uint32_t total;
    (void)brcside::block_scan(i < count ? in[i] : 0u, sh, total);
    if (threadIdx.x == 0) part[blockIdx.x] = total;
}
// 2. ONE workgroup: part[] -> its exclusive scan, a block of partials at a time with a running carry; the total to the scratch and to the caller
__global__ __launch_bounds__(brcside::SCAN_BLOCK) void k_side_scan_parts(uint32_t* part, uint64_t nb, uint32_t* tot_ws, uint32_t* tot_dst) {
    __shared__ uint32_t sh[brcside::SCAN_BLOCK];
    uint32_t carry = 0;
    for (uint64_t base = 0; base < nb; base += brcside::SCAN_BLOCK) {
        const uint64_t i = base + threadIdx.x;
        const uint32_t v = i < nb ? part[i] : 0u;
        uint32_t total;
        const uint32_t ex = brcside::block_scan(v, sh, total);
        if (i < nb) part[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) { *tot_ws = carry; if (tot_dst) *tot_dst = carry; }
}
// 3. out[i] = part[b] + the exclusive scan inside tile b; out[count] = the total
__global__ __launch_bounds__(brcside::SCAN_BLOCK) void k_side_scan_apply(const uint32_t* __restrict__ in, const uint32_t* n_dev, uint64_t n_host,
                                                                          const uint32_t* __restrict__ part, uint32_t* __restrict__ out) {
    __shared__ uint32_t sh[brcside::SCAN_BLOCK];
    const uint64_t count = brcside::scan_count(n_dev, n_host), i = (uint64_t)blockIdx.x * brcside::SCAN_BLOCK + threadIdx.x;
    const uint32_t v = i < count ? in[i] : 0u;
    uint32_t total;
    const uint32_t ex = brcside::block_scan(v, sh, total) + part[blockIdx.x];
    if (i < count) out[i] = ex;
    if (i + 1 == count) out[count] = ex + v;
    if (count == 0 && i == 0) out[0] = 0u;
}

namespace brcside {

// the three launches of one scan: `in` [n_host at the most; *n_dev of them when n_dev] -> out [count + 1]; part: (n_host + 255) / 256 words
// of scratch (one at the least)
static inline int scan(Handle* h, hipStream_t stream, uint32_t* part, const uint32_t* in, const uint32_t* n_dev, uint64_t n_host, uint32_t* out,
                       uint32_t* tot_ws, uint32_t* tot_dst) {
    const uint64_t nb = n_host ? (n_host + SCAN_BLOCK - 1) / SCAN_BLOCK : 1;
    LAUNCH(k_side_scan_reduce, dim3((unsigned)nb), dim3(SCAN_BLOCK), 0, stream, in, n_dev, n_host, part);
    LAUNCH(k_side_scan_parts, dim3(1), dim3(SCAN_BLOCK), 0, stream, part, nb, tot_ws, tot_dst);
    LAUNCH(k_side_scan_apply, dim3((unsigned)nb), dim3(SCAN_BLOCK), 0, stream, in, n_dev, n_host, (const uint32_t*)part, out);
    return BRC_OK;
}

}  // namespace brcside
