// brc_indels.hip — the device-resident indel table for gfx950 behind the C-ABI of include/brc_indels.h (libbrc_indels_hip.so; a
// translation unit and a library of its own: the engine's libraries keep exactly the device code they had, and this one links nothing
// of the engine).
//
// A gather is a counting sort by position followed by a rank inside each position's run (brc_indels_core.h), all on the caller's stream:
//   memset cnt | k_count | scan(cnt -> off, counts[0]) | k_place | k_rank | scan(alen -> aoff, counts[1]) | k_emit
// A scan is reduce-then-scan in three launches — every workgroup's sum, ONE workgroup scanning the sums, every workgroup scanning its
// tile onto its sum — so no workgroup ever waits for another: the launches' order on the stream is the only dependency.  The host
// does not know the record count M (it never waits): the launches behind the first scan are sized by the slot count, an upper bound,
// and their lanes read M from the scratch.  DESIGN.md 6d has the reasoning.
#include <hip/hip_runtime.h>

#include "brc_indels_core.h"
#include "brc_side_hip.h"

using namespace brcindels;

enum { BLOCK = SCAN_TILE };      // four waves

__global__ __launch_bounds__(BLOCK) void k_count(const Job J) {
    const uint64_t s = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s < J.n_slots) count_lane(J, s);
}
__global__ __launch_bounds__(BLOCK) void k_place(const Job J) {
    const uint64_t s = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s < J.n_slots) place_lane(J, s);
}
__global__ __launch_bounds__(BLOCK) void k_rank(const Job J) {
    const uint64_t j = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j < J.n_slots) rank_lane(J, j);
}
__global__ __launch_bounds__(BLOCK) void k_emit(const Job J) {
    const uint64_t r = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (r <= J.n_slots) emit_lane(J, r);
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
// elements of a scan: n_host, or the device-side count (never above n_host: the launch is sized by it)
__device__ inline uint64_t scan_count(const uint32_t* n_dev, uint64_t n_host) {
    if (!n_dev) return n_host;
    const uint64_t c = *n_dev;
    return c < n_host ? c : n_host;
}
// 1. part[b] = sum of tile b (0 for a tile behind the count)
__global__ __launch_bounds__(BLOCK) void k_scan_reduce(const uint32_t* __restrict__ in, const uint32_t* n_dev, uint64_t n_host, uint32_t* __restrict__ part) {
    __shared__ uint32_t sh[BLOCK];
    const uint64_t count = scan_count(n_dev, n_host), i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    uint32_t total;
    (void)block_scan(i < count ? in[i] : 0u, sh, total);
    if (threadIdx.x == 0) part[blockIdx.x] = total;
}
// 2. ONE workgroup: part[] -> its exclusive scan, BLOCK partials at a time with a running carry; the total to the scratch and to the caller
__global__ __launch_bounds__(BLOCK) void k_scan_parts(uint32_t* part, uint64_t nb, uint32_t* tot_ws, uint32_t* tot_dst) {
    __shared__ uint32_t sh[BLOCK];
    uint32_t carry = 0;
    for (uint64_t base = 0; base < nb; base += BLOCK) {
        const uint64_t i = base + threadIdx.x;
        const uint32_t v = i < nb ? part[i] : 0u;
        uint32_t total;
        const uint32_t ex = block_scan(v, sh, total);
        if (i < nb) part[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) { *tot_ws = carry; if (tot_dst) *tot_dst = carry; }
}
// 3. out[i] = part[b] + the exclusive scan inside tile b; out[count] = the total
__global__ __launch_bounds__(BLOCK) void k_scan_apply(const uint32_t* __restrict__ in, const uint32_t* n_dev, uint64_t n_host, const uint32_t* __restrict__ part,
                                                      uint32_t* __restrict__ out) {
    __shared__ uint32_t sh[BLOCK];
    const uint64_t count = scan_count(n_dev, n_host), i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t v = i < count ? in[i] : 0u;
    uint32_t total;
    const uint32_t ex = block_scan(v, sh, total) + part[blockIdx.x];
    if (i < count) out[i] = ex;
    if (i + 1 == count) out[count] = ex + v;
    if (count == 0 && i == 0) out[0] = 0u;
}

struct brc_indels : brcside::Handle {};

// the three launches of one scan: `in` [n_host at the most; *n_dev of them when n_dev] -> out [count + 1]
static int scan(brc_indels* h, hipStream_t stream, const Job& J, const uint32_t* in, const uint32_t* n_dev, uint64_t n_host, uint32_t* out, uint32_t* tot_ws, uint32_t* tot_dst) {
    const uint64_t nb = scan_blocks(n_host);
    LAUNCH(k_scan_reduce, dim3((unsigned)nb), dim3(BLOCK), 0, stream, in, n_dev, n_host, J.part);
    LAUNCH(k_scan_parts, dim3(1), dim3(BLOCK), 0, stream, J.part, nb, tot_ws, tot_dst);
    LAUNCH(k_scan_apply, dim3((unsigned)nb), dim3(BLOCK), 0, stream, in, n_dev, n_host, (const uint32_t*)J.part, out);
    return BRC_OK;
}

extern "C" {

const char* brc_indels_kind(void) { return "hip-gfx950"; }
int brc_indels_create(int device, brc_indels** out) { return brcside::create(device, (const void*)k_emit, out); }
void brc_indels_destroy(brc_indels* h) { brcside::destroy(h); }
const char* brc_indels_last_error(const brc_indels* h) { return brcside::last_error(h); }
void brc_indels_last_timing(const brc_indels* h, double* kernel_s, uint64_t* bytes_read, uint64_t* bytes_written) { brcside::last_timing(h, kernel_s, bytes_read, bytes_written); }
size_t brc_indels_workspace(const brc_device_indels* v, int64_t n) { return workspace_bytes(v, n); }

int brc_indels_gather(brc_indels* h, const brc_device_indels* v, int64_t k0, int64_t n, void* workspace, size_t workspace_bytes_, uint32_t* counts,
                      int64_t cap, int64_t alleles_cap, int32_t* pos, int32_t* lib, int32_t* len, uint32_t* rep_read, int32_t* rep_qpos,
                      uint32_t* istat, float* fstat, float* metrics, uint32_t* allele_off, uint8_t* alleles, void* stream_) {
    if (!h) return BRC_E_ARG;
    brcside::clear(h);
    const char* why = "";
    if (check_job(v, k0, n, cap, alleles_cap, workspace, workspace_bytes_, &why)) return brcside::refuse(h, why);
    if (int rc = brcside::resident(h, v, brcside::ONE_VIEW)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    HIPOK(hipSetDevice(h->device));
    if (n == 0 || v->n_slots == 0) {
        if (counts) HIPOK(hipMemsetAsync(counts, 0, 2 * sizeof(uint32_t), stream));
        if (allele_off) HIPOK(hipMemsetAsync(allele_off, 0, sizeof(uint32_t), stream));
        return BRC_OK;
    }
    const Job J = make_job(v, k0, n, workspace, counts, cap, alleles_cap, pos, lib, len, rep_read, rep_qpos, istat, fstat, metrics, allele_off, alleles);
    if (!counts && !wants_records(J)) return BRC_OK;
    const unsigned slot_blocks = (unsigned)scan_blocks(J.n_slots);
    if (int rc = brcside::start(h, stream)) return rc;
    HIPOK(hipMemsetAsync(J.cnt, 0, (size_t)n * sizeof(uint32_t), stream));
    LAUNCH(k_count, dim3(slot_blocks), dim3(BLOCK), 0, stream, J);
    int rc = scan(h, stream, J, J.cnt, nullptr, (uint64_t)n, J.off, J.tot, counts);
    if (rc) return rc;
    LAUNCH(k_place, dim3(slot_blocks), dim3(BLOCK), 0, stream, J);
    LAUNCH(k_rank, dim3(slot_blocks), dim3(BLOCK), 0, stream, J);
    rc = scan(h, stream, J, J.alen, J.tot, J.n_slots, J.aoff, J.tot + 1, counts ? counts + 1 : nullptr);
    if (rc) return rc;
    if (wants_records(J)) LAUNCH(k_emit, dim3((unsigned)scan_blocks(J.n_slots + 1)), dim3(BLOCK), 0, stream, J);
    return brcside::done(h, stream, J);
}

}  // extern "C"
