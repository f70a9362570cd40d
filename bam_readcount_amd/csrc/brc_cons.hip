// brc_cons.hip — device-side consensus caller for gfx950 behind the C-ABI of include/brc_cons.h (libbrc_cons_hip.so; a translation unit
// and a library of its own: the engine's and the siblings' libraries keep exactly the device code they had, and this one links nothing
// of them).
//
// Per call, on the caller's stream:
//   memset status, head, diff, run | k_cons_link | k_cons_records | scan diff -> dcov | k_cons_sites | scan lens -> offs | k_cons_emit
//   k_cons_link     lane == third-allele record: pushes itself onto its position's list (only when the view has records)
//   k_cons_records  lane == table record: status bits; a deletion adds its count at the two ends of its cover (two 32-bit atomic adds
//                   whatever its length); a run's first record marks its position; an insertion leaves its support in the scratch
//   k_cons_sites    lane == position, wave == 64 consecutive positions: three plane loads per counted library, each one run of 256
//                   bytes per wave; the call bytes of a workgroup are packed in LDS and leave as dwords (64 lanes x 4 bytes instead of
//                   256 byte stores); with BRC_CONS_ALIGNED that is the sequence, and the call ends here
//   k_cons_emit     lane == position: its offset from the scan; its call byte and its insertion's text to the sequence (byte stores:
//                   the offsets are data, a workgroup's bytes start anywhere)
// The scans are brc_side_scan.h's reduce-then-scan: no workgroup ever waits for another, the launches' order on the stream is the only
// dependency, and every launch is sized by n or m — the host never learns the count.  The per-lane work is brc_cons_core.h, shared
// with the CPU build the tests run.  DESIGN.md 6o has the reasoning.
#include <hip/hip_runtime.h>

#include "brc_cons_core.h"
#include "brc_side_hip.h"
#include "brc_side_scan.h"

using namespace brccons;

static_assert((int)BLOCK == (int)brcside::SCAN_BLOCK, "a scan tile is a workgroup of the sweeps");

__global__ __launch_bounds__(BLOCK) void k_cons_link(const Job J) {
    const uint64_t r = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (r < J.n_xagg) link_lane(J, r);
}
__global__ __launch_bounds__(BLOCK) void k_cons_records(const Job J) {
    const int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (r < J.m) record_lane(J, r);
}

// The workgroup's `valid` bytes in sh -> dst[0 .. valid): whole dwords from the first lanes where dst is 4-byte aligned, bytes otherwise
// and for the tail.  (dst is uniform over the workgroup.)
__device__ inline void store_packed(uint8_t* dst, const uint32_t* sh, uint32_t valid) {
    const uint32_t t = threadIdx.x;
    const uint32_t words = (((uintptr_t)dst & 3u) == 0u) ? valid / 4u : 0u;
    if (t < words) ((uint32_t*)dst)[t] = sh[t];
    else if (t >= words * 4u && t < valid) dst[t] = ((const uint8_t*)sh)[t];
}

__global__ __launch_bounds__(BLOCK) void k_cons_sites(const Job J) {
    __shared__ uint32_t sh[BLOCK / 4];
    const int64_t j0 = (int64_t)blockIdx.x * BLOCK, j = j0 + threadIdx.x;
    const uint32_t ch = j < J.n ? site_lane(J, j) : 0u;
    ((uint8_t*)sh)[threadIdx.x] = (uint8_t)ch;
    __syncthreads();
    const uint32_t valid = (uint32_t)(J.n - j0 < (int64_t)BLOCK ? J.n - j0 : (int64_t)BLOCK);
    if (J.o_call) store_packed(J.o_call + j0, sh, valid);
    if (aligned(J)) {
        if (J.o_seq) {                                      // seq[j] = call[j] in front of seq_cap
            const int64_t room = J.cap - j0;
            if (room > 0) store_packed(J.o_seq + j0, sh, room < (int64_t)valid ? (uint32_t)room : valid);
        }
    } else {
        store_packed(J.wcall + j0, sh, valid);
    }
}

__global__ __launch_bounds__(BLOCK) void k_cons_emit(const Job J) {
    const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j < J.n) emit_lane(J, j);
}

struct brc_cons : brcside::Handle {};

extern "C" {

const char* brc_cons_kind(void) { return "hip-gfx950"; }
int brc_cons_create(int device, brc_cons** out) { return brcside::create(device, (const void*)k_cons_sites, out); }
void brc_cons_destroy(brc_cons* h) { brcside::destroy(h); }
const char* brc_cons_last_error(const brc_cons* h) { return brcside::last_error(h); }
void brc_cons_last_timing(const brc_cons* h, double* kernel_s, uint64_t* bytes_read, uint64_t* bytes_written) { brcside::last_timing(h, kernel_s, bytes_read, bytes_written); }
int64_t brc_cons_workspace(const brc_device_view* v, int64_t n, int64_t m) { return workspace_bytes(v, n, m); }

int brc_cons_call(brc_cons* h, const brc_device_view* v, const brc_device_indels* d, const brc_cons_params* p, const brc_cons_table* t, int64_t k0, int64_t n,
                  int64_t dst_stride, int64_t seq_cap, uint32_t* counts, uint8_t* call, uint32_t* cnt, uint32_t* ins_rec, uint32_t* off, uint8_t* seq,
                  uint32_t* status, void* workspace, void* stream_) {
    if (!h) return BRC_E_ARG;
    brcside::clear(h);
    const char* why = "";
    if (check_job(v, d, p, t, k0, n, dst_stride, seq_cap, workspace, &why)) return brcside::refuse(h, why);
    if (int rc = brcside::resident(h, v, brcside::TWO_VIEWS)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    HIPOK(hipSetDevice(h->device));
    if (status) HIPOK(hipMemsetAsync(status, 0, sizeof(uint32_t), stream));
    if (n == 0) {
        if (counts) HIPOK(hipMemsetAsync(counts, 0, sizeof(uint32_t), stream));
        if (off) HIPOK(hipMemsetAsync(off, 0, sizeof(uint32_t), stream));
        return BRC_OK;
    }
    const Job J = make_job(v, d, p, t, k0, n, dst_stride, seq_cap, counts, call, cnt, ins_rec, off, seq, status, workspace);
    if (!wants_sites(J) && !(status && walks_table(J))) return BRC_OK;
    const unsigned nb = (unsigned)blocks_of((uint64_t)n);
    if (int rc = brcside::start(h, stream)) return rc;
    if (walks_records(J) && wants_sites(J)) {
        HIPOK(hipMemsetAsync(J.head, 0xff, (size_t)n * sizeof(uint32_t), stream));
        LAUNCH(k_cons_link, dim3((unsigned)blocks_of(J.n_xagg)), dim3(BLOCK), 0, stream, J);
    }
    if (walks_table(J)) {
        HIPOK(hipMemsetAsync(J.diff, 0, (size_t)n * sizeof(uint32_t), stream));
        HIPOK(hipMemsetAsync(J.run, 0xff, (size_t)n * sizeof(uint32_t), stream));
        LAUNCH(k_cons_records, dim3((unsigned)blocks_of((uint64_t)J.m)), dim3(BLOCK), 0, stream, J);
        if (wants_sites(J))
            if (int rc = brcside::scan(h, stream, J.part, J.diff, nullptr, (uint64_t)n, J.dcov, J.tot, nullptr)) return rc;
    }
    if (wants_sites(J)) {
        LAUNCH(k_cons_sites, dim3(nb), dim3(BLOCK), 0, stream, J);
        if (wants_scan(J))
            if (int rc = brcside::scan(h, stream, J.part, J.lens, nullptr, (uint64_t)n, J.offs, J.tot, J.o_counts)) return rc;
        if (wants_emit(J)) LAUNCH(k_cons_emit, dim3(nb), dim3(BLOCK), 0, stream, J);
    }
    return brcside::done(h, stream, J);
}

}  // extern "C"
