// The length limiter of brc_deflate_core.h on the device, as the kernel runs it (make limit_check_hip; limit_check.cpp is its host
// counterpart): no input of the suite brings a block's own histogram beyond 13 bits, so the counts go to the function
// itself.  One workgroup of 256 lanes per case holds a brcdef::Shared in LDS and takes the steps of deflate_member() between the
// histogram and the run-length coding, on the same arrays: every lane ranks the used symbols of both alphabets by (count, symbol)
// into A / sorted, lane 0 runs limited_lengths() at 15 bits on the literal/length alphabet (num[0], lens) while lane 64 runs it on
// the distance alphabet (num[1], lens + DBASE), then lane 0 sorts the code-length counts by insertion and runs the 7-bit call
// (clA, clsorted, num[2], cllens).
//   usage: limit_check_hip cases.txt     one case per line: 286 literal/length counts, 30 distance counts, 19 code-length counts
//   prints per case one line of 335 code lengths in the same order
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../bam_readcount_amd/csrc/brc_deflate_core.h"

using namespace brcdef;

constexpr uint32_t NLIT = 286, NDIST = 30, NCL = 19, PER_CASE = NLIT + NDIST + NCL;
static_assert(sizeof(Shared) <= 160 * 1024 && NLIT <= DBASE && DBASE + NDIST <= 320, "one workgroup's LDS; both alphabets in hist / lens");

__global__ __launch_bounds__(LANES) void k_limit(const uint32_t* __restrict__ counts, uint8_t* __restrict__ lens_out, uint32_t ncases) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    Shared& sh = *reinterpret_cast<Shared*>(lds_raw);
    if (blockIdx.x >= ncases) return;
    const uint32_t* c = counts + (size_t)blockIdx.x * PER_CASE;
    uint8_t* o = lens_out + (size_t)blockIdx.x * PER_CASE;
    const uint32_t l = threadIdx.x;
    for (uint32_t i = l; i < 320; i += LANES) {
        sh.hist[i] = i < NLIT ? c[i] : (i >= DBASE && i < DBASE + NDIST) ? c[NLIT + (i - DBASE)] : 0u;
        sh.lens[i] = 0;
    }
    if (l < 2) sh.nused[l] = 0;
    __syncthreads();
    // (the ranking of deflate_member)
    for (uint32_t i = l; i < 320; i += LANES) {
        const uint32_t base = i < DBASE ? 0u : DBASE, ns = i < DBASE ? NLIT : NDIST, f = sh.hist[i];
        if (i - base >= ns || !f) continue;
        uint32_t rank = 0;
        for (uint32_t j = 0; j < ns; ++j) { const uint32_t g = sh.hist[base + j]; rank += (g && (g < f || (g == f && base + j < i))) ? 1u : 0u; }
        sh.sorted[base + rank] = (uint16_t)(i - base); sh.A[base + rank] = f;
        atomicAdd(&sh.nused[base ? 1 : 0], 1u);
    }
    __syncthreads();
    if (l == 0) limited_lengths(sh.A, sh.sorted, sh.num[0], sh.lens, (int)sh.nused[0], 15);
    if (l == 64) limited_lengths(sh.A + DBASE, sh.sorted + DBASE, sh.num[1], sh.lens + DBASE, (int)sh.nused[1], 15);
    __syncthreads();
    if (l == 0) {
        int nu = 0;
        for (uint32_t s = 0; s < NCL; ++s) {
            sh.cllens[s] = 0;
            const uint32_t f = c[NLIT + NDIST + s];
            if (!f) continue;
            int k = nu++;
            while (k > 0 && sh.clA[k - 1] > f) { sh.clA[k] = sh.clA[k - 1]; sh.clsorted[k] = sh.clsorted[k - 1]; --k; }
            sh.clA[k] = f; sh.clsorted[k] = (uint16_t)s;
        }
        limited_lengths(sh.clA, sh.clsorted, sh.num[2], sh.cllens, nu, 7);
    }
    __syncthreads();
    for (uint32_t i = l; i < PER_CASE; i += LANES) o[i] = i < NLIT ? sh.lens[i] : i < NLIT + NDIST ? sh.lens[DBASE + (i - NLIT)] : sh.cllens[i - NLIT - NDIST];
}

#define OK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_)); return 1; } } while (0)

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: limit_check_hip cases.txt\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint32_t> counts;
    unsigned long v;
    while (fscanf(f, "%lu", &v) == 1) counts.push_back((uint32_t)v);
    fclose(f);
    const size_t ncases = counts.size() / PER_CASE;
    if (!ncases || counts.size() % PER_CASE || ncases > 65536) { fprintf(stderr, "%zu counts: not whole cases of %u\n", counts.size(), PER_CASE); return 2; }
    uint32_t* d_counts = nullptr; uint8_t* d_lens = nullptr;
    std::vector<uint8_t> lens(ncases * PER_CASE);
    OK(hipMalloc((void**)&d_counts, counts.size() * sizeof(uint32_t)));
    OK(hipMalloc((void**)&d_lens, lens.size()));
    OK(hipMemcpy(d_counts, counts.data(), counts.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    OK(hipMemset(d_lens, 0xff, lens.size()));
    OK(hipFuncSetAttribute((const void*)k_limit, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(Shared)));
    hipLaunchKernelGGL(k_limit, dim3((unsigned)ncases), dim3(LANES), sizeof(Shared), 0, d_counts, d_lens, (uint32_t)ncases);
    OK(hipGetLastError());
    OK(hipDeviceSynchronize());
    OK(hipMemcpy(lens.data(), d_lens, lens.size(), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < ncases; ++k)
        for (uint32_t i = 0; i < PER_CASE; ++i) printf("%d%c", lens[k * PER_CASE + i], i + 1 < PER_CASE ? ' ' : '\n');
    OK(hipFree(d_counts)); OK(hipFree(d_lens));
    return 0;
}
