// CPU build of the device-resident indel table's C-ABI (include/brc_indels.h) over brc_indels_core.h: the test counterpart of
// libbrc_indels_hip.so, as libbrc_sim.so is the engine's.  The launches of the gfx950 library run here as loops in the same order —
// every slot lane of the count, a serial scan, every slot lane of the placement, every record lane of the rank, a serial scan, every
// record lane of the emission — on host memory: a view with memory == BRC_MEM_HOST (what libbrc_sim.so hands out).  Slot lanes run
// from the LAST slot to the first, so that the order inside a position's run is not the slots' own: the rank has to make it.
// Test infrastructure only.
#include "../../bam_readcount_amd/csrc/brc_indels_core.h"
#include "../sim_side.h"

using namespace brcindels;

struct brc_indels : brcside::Handle {};

// in[0 .. count) -> out[0 .. count]: the exclusive scan and, behind it, the total
static uint32_t scan(const uint32_t* in, uint64_t count, uint32_t* out) {
    uint32_t acc = 0;
    for (uint64_t i = 0; i < count; ++i) { out[i] = acc; acc += in[i]; }
    out[count] = acc;
    return acc;
}

extern "C" {

const char* brc_indels_kind(void) { return "sim"; }
int brc_indels_create(int device, brc_indels** out) { return brcside::create(device, out); }
void brc_indels_destroy(brc_indels* h) { brcside::destroy(h); }
const char* brc_indels_last_error(const brc_indels* h) { return brcside::last_error(h); }
void brc_indels_last_timing(const brc_indels* h, double* kernel_s, uint64_t* bytes_read, uint64_t* bytes_written) { brcside::last_timing(h, kernel_s, bytes_read, bytes_written); }
size_t brc_indels_workspace(const brc_device_indels* v, int64_t n) { return workspace_bytes(v, n); }

int brc_indels_gather(brc_indels* h, const brc_device_indels* v, int64_t k0, int64_t n, void* workspace, size_t workspace_bytes_, uint32_t* counts,
                      int64_t cap, int64_t alleles_cap, int32_t* pos, int32_t* lib, int32_t* len, uint32_t* rep_read, int32_t* rep_qpos,
                      uint32_t* istat, float* fstat, float* metrics, uint32_t* allele_off, uint8_t* alleles, void*) {
    if (!h) return BRC_E_ARG;
    brcside::clear(h);
    const char* why = "";
    if (check_job(v, k0, n, cap, alleles_cap, workspace, workspace_bytes_, &why)) return brcside::refuse(h, why);
    if (int rc = brcside::resident(h, v, brcside::ONE_VIEW)) return rc;
    if (n == 0 || v->n_slots == 0) {
        if (counts) counts[0] = counts[1] = 0;
        if (allele_off) allele_off[0] = 0;
        return BRC_OK;
    }
    const Job J = make_job(v, k0, n, workspace, counts, cap, alleles_cap, pos, lib, len, rep_read, rep_qpos, istat, fstat, metrics, allele_off, alleles);
    if (!counts && !wants_records(J)) return BRC_OK;
    brcside::start(h);
    for (int64_t d = 0; d < n; ++d) J.cnt[d] = 0;
    for (uint64_t s = J.n_slots; s-- > 0;) count_lane(J, s);
    J.tot[0] = scan(J.cnt, (uint64_t)n, J.off);
    if (counts) counts[0] = J.tot[0];
    for (uint64_t s = J.n_slots; s-- > 0;) place_lane(J, s);
    for (uint64_t j = 0; j < J.n_slots; ++j) rank_lane(J, j);
    J.tot[1] = scan(J.alen, J.tot[0], J.aoff);
    if (counts) counts[1] = J.tot[1];
    if (wants_records(J)) for (uint64_t r = 0; r <= J.n_slots; ++r) emit_lane(J, r);
    return brcside::done(h, J);
}

}  // extern "C"
