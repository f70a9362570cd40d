// CPU build of the join's C-ABI (include/brc_join.h) over brc_join_core.h: the test counterpart of libbrc_join_hip.so, as libbrc_sim.so
// is the engine's.  The launches of the gfx950 library run here as loops in the same order — every (row, group) lane of the planes,
// every record lane of the third-allele records and of the indel records, a serial scan, every record lane of the synthetic reads,
// every byte lane of the reference slice — on host memory: views with memory == BRC_MEM_HOST (what libbrc_sim.so hands out), scratch
// and destinations in host memory.  Every loop runs from the LAST lane to the first: nothing may depend on the order of the lanes.
// Test infrastructure only.
#include "../../bam_readcount_amd/csrc/brc_join_core.h"
#include "../sim_side.h"

using namespace brcjoin;

struct brc_join : brcside::Handle {};

extern "C" {

const char* brc_join_kind(void) { return "sim"; }
int brc_join_create(int device, brc_join** out) { return brcside::create(device, out); }
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
                   size_t workspace_bytes_, void*) {
    if (!h) return BRC_E_ARG;
    brcside::clear(h);
    const char* why = ""; brc_join_sizes z; int32_t memory = 0, device = 0;
    if (check_job(K, sources, pos0, n_pos, stride, dst, out_view, out_indels, counts, seq_cap, status, workspace, workspace_bytes_, &z, &memory, &device, &why))
        return brcside::refuse(h, why);
    if (int rc = brcside::resident(h, sources[0].view, brcside::TWO_VIEWS)) return rc;
    const bool planes = dst && out_view, indels = !dst || out_indels;
    const Job J = make_job(K, sources, pos0, n_pos, stride, dst, planes, indels, counts, seq_cap, status, workspace, z);
    if (status) *status = 0;
    if (counts && indels) counts[0] = counts[1] = 0;
    if (dst) fill_views(J, z, memory, device, out_view, out_indels);
    if (n_pos == 0) return BRC_OK;
    brcside::start(h);
    if (planes) {
        for (int64_t y = (int64_t)ROWS * J.L; y-- > 0;) for (int64_t g = row_groups(n_pos); g-- > 0;) planes_lane(J, y, g);
        for (uint64_t t = z.n_xagg; t-- > 0;) xagg_lane(J, t);
    }
    if (indels && z.n_slots) {
        const uint64_t S = z.n_slots;
        for (uint64_t t = S; t-- > 0;) slots_lane(J, t);
        uint32_t acc = 0;
        for (uint64_t t = 0; t < S; ++t) { J.offs[t] = acc; acc += J.bytes[t]; }
        J.offs[S] = acc; J.tot[0] = acc;
        if (counts) counts[1] = acc;
        if (dst) for (uint64_t t = S; t-- > 0;) reads_lane(J, t);
    }
    if (indels && dst) for (int64_t x = (int64_t)z.ref_bytes; x-- > 0;) ref_lane(J, x);
    return brcside::done(h, J);
}

}  // extern "C"
