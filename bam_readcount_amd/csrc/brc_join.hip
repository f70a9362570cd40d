// brc_join.hip — device-side join of computed regions for gfx950 behind the C-ABI of include/brc_join.h (libbrc_join_hip.so; a
// translation unit and a library of its own: the engine's libraries and its siblings keep exactly the device code they had, and this
// one links none of them).
//
// Per call, on the caller's stream: the status word's and the counts' clear, then
//   k_join_planes   THE HOT ONE: grid (groups of a row / 256, 29 * L rows); lane = four consecutive destination elements behind the
//                   row's first 16-byte boundary: one non-temporal 16-byte store, fed by one 16-byte load where the source's offset
//                   allows it and by four 4-byte loads otherwise (a wave's lanes read one contiguous kilobyte either way); positions no
//                   source covers are stored as the engine's empty position in the same pass — no memset, no second launch.  The source
//                   table travels in the kernel arguments and is looked up once per row, on the scalar unit.  No LDS, no scratch memory.
//   k_join_xagg | k_join_slots | scan(bytes -> offs, counts[1]) | k_join_reads | k_join_ref
// lane = one record (one byte of the reference slice), 256 to a workgroup.  No workgroup ever waits for another, the launches' order on
// the stream is the only dependency, and every launch is sized by host-known numbers.  DESIGN.md 6n has the reasoning.
#include <hip/hip_runtime.h>

#include "brc_join_core.h"
#include "brc_side_hip.h"
#include "brc_side_scan.h"

using namespace brcjoin;

__global__ __launch_bounds__(BLOCK) void k_join_planes(const Job J) {
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g < row_groups(J.n)) planes_lane(J, (int64_t)blockIdx.y, g);
}
__global__ __launch_bounds__(BLOCK) void k_join_xagg(const Job J) {
    const uint64_t t = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t < J.xbase[J.K]) xagg_lane(J, t);
}
__global__ __launch_bounds__(BLOCK) void k_join_slots(const Job J) {
    const uint64_t t = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t < J.sbase[J.K]) slots_lane(J, t);
}
__global__ __launch_bounds__(BLOCK) void k_join_reads(const Job J) {
    const uint64_t t = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t < J.sbase[J.K]) reads_lane(J, t);
}
__global__ __launch_bounds__(BLOCK) void k_join_ref(const Job J) {
    const int64_t x = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (x < J.ref_hi - J.ref_lo) ref_lane(J, x);
}

struct brc_join : brcside::Handle {};

extern "C" {

const char* brc_join_kind(void) { return "hip-gfx950"; }
int brc_join_create(int device, brc_join** out) { return brcside::create(device, (const void*)k_join_planes, out); }
void brc_join_destroy(brc_join* h) { brcside::destroy(h); }
const char* brc_join_last_error(const brc_join* h) { return brcside::last_error(h); }
void brc_join_last_timing(const brc_join* h, double* kernel_s, uint64_t* bytes_read, uint64_t* bytes_written) { brcside::last_timing(h, kernel_s, bytes_read, bytes_written); }
size_t brc_join_workspace(uint64_t n_slots) { return workspace_bytes(n_slots); }
int brc_join_sizes_of(int32_t K, const brc_join_source* sources, int32_t pos0, int64_t n_pos, int64_t stride, brc_join_sizes* out) {
    if (!out) return BRC_E_ARG;
    const char* why = ""; int32_t memory = 0, device = 0;
    const int rc = check_sources(K, sources, pos0, n_pos, stride, out, &memory, &device, &why);
    if (rc) memset(out, 0, sizeof *out);
    return rc;
}

int brc_join_views(brc_join* h, int32_t K, const brc_join_source* sources, int32_t pos0, int64_t n_pos, int64_t stride, const brc_join_dest* dst,
                   brc_device_view* out_view, brc_device_indels* out_indels, uint32_t* counts, int64_t seq_cap, uint32_t* status, void* workspace,
                   size_t workspace_bytes_, void* stream_) {
    if (!h) return BRC_E_ARG;
    brcside::clear(h);
    const char* why = ""; brc_join_sizes z; int32_t memory = 0, device = 0;
    if (check_job(K, sources, pos0, n_pos, stride, dst, out_view, out_indels, counts, seq_cap, status, workspace, workspace_bytes_, &z, &memory, &device, &why))
        return brcside::refuse(h, why);
    if (int rc = brcside::resident(h, sources[0].view, brcside::TWO_VIEWS)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    HIPOK(hipSetDevice(h->device));
    const bool planes = dst && out_view, indels = !dst || out_indels;
    const Job J = make_job(K, sources, pos0, n_pos, stride, dst, planes, indels, counts, seq_cap, status, workspace, z);
    if (status) HIPOK(hipMemsetAsync(status, 0, sizeof(uint32_t), stream));
    if (counts && indels) HIPOK(hipMemsetAsync(counts, 0, 2 * sizeof(uint32_t), stream));
    if (dst) fill_views(J, z, memory, device, out_view, out_indels);
    if (n_pos == 0) return BRC_OK;
    if (int rc = brcside::start(h, stream)) return rc;
    if (planes) {
        LAUNCH(k_join_planes, dim3((unsigned)scan_blocks((uint64_t)row_groups(n_pos)), (unsigned)(ROWS * J.L)), dim3(BLOCK), 0, stream, J);
        if (z.n_xagg) LAUNCH(k_join_xagg, dim3((unsigned)scan_blocks(z.n_xagg)), dim3(BLOCK), 0, stream, J);
    }
    if (indels && z.n_slots) {
        const uint64_t S = z.n_slots;
        LAUNCH(k_join_slots, dim3((unsigned)scan_blocks(S)), dim3(BLOCK), 0, stream, J);
        if (int rc = brcside::scan(h, stream, J.part, J.bytes, nullptr, S, J.offs, J.tot, counts ? counts + 1 : nullptr)) return rc;
        if (dst) LAUNCH(k_join_reads, dim3((unsigned)scan_blocks(S)), dim3(BLOCK), 0, stream, J);
    }
    if (indels && dst && z.ref_bytes) LAUNCH(k_join_ref, dim3((unsigned)scan_blocks(z.ref_bytes)), dim3(BLOCK), 0, stream, J);
    return brcside::done(h, stream, J);
}

}  // extern "C"
