// CPU build of the indel normalisation's C-ABI (include/brc_inorm.h) over brc_inorm_core.h: the test counterpart of libbrc_inorm_hip.so,
// as libbrc_sim.so is the engine's.  The launches of the gfx950 library run here as loops in the same order — every record lane of the
// walk, a serial scan, every record lane of the placement, of the rank and of the heads, two serial scans, every record lane of the
// merge — on host memory: a view with memory == BRC_MEM_HOST (what libbrc_sim.so hands out), table, scratch and destinations in host
// memory.  Every loop runs from the LAST lane to the first: nothing may depend on the order of the lanes, and the order inside a
// position's run is not the table's own: the rank has to make it.  Test infrastructure only.
#include "../../bam_readcount_amd/csrc/brc_inorm_core.h"
#include "../sim_side.h"

using namespace brcinorm;

struct brc_inorm : brcside::Handle {};

// in[0 .. count) -> out[0 .. count]: the exclusive scan and, behind it, the total
static uint32_t scan(const uint32_t* in, uint64_t count, uint32_t* out) {
    uint32_t acc = 0;
    for (uint64_t i = 0; i < count; ++i) { out[i] = acc; acc += in[i]; }
    out[count] = acc;
    return acc;
}

extern "C" {

const char* brc_inorm_kind(void) { return "sim"; }
int brc_inorm_create(int device, brc_inorm** out) { return brcside::create(device, out); }
void brc_inorm_destroy(brc_inorm* h) { brcside::destroy(h); }
const char* brc_inorm_last_error(const brc_inorm* h) { return brcside::last_error(h); }
void brc_inorm_last_timing(const brc_inorm* h, double* kernel_s, uint64_t* bytes_read, uint64_t* bytes_written) { brcside::last_timing(h, kernel_s, bytes_read, bytes_written); }
size_t brc_inorm_workspace(int64_t n, int64_t m) { return workspace_bytes(n, m); }

int brc_inorm_table(brc_inorm* h, const brc_device_indels* v, const brc_inorm_params* p, const brc_inorm_source* t, int64_t k0, int64_t n, void* workspace,
                    size_t workspace_bytes_, uint32_t* counts, int32_t* npos, uint32_t* shift, uint32_t* flags, int32_t* group, int64_t cap, int64_t alleles_cap,
                    int32_t* pos, int32_t* lib, int32_t* len, uint32_t* rep_read, int32_t* rep_qpos, uint32_t* members, uint32_t* istat, float* fstat,
                    float* metrics, uint32_t* allele_off, uint8_t* alleles, uint32_t* status, void*) {
    if (!h) return BRC_E_ARG;
    brcside::clear(h);
    const char* why = "";
    if (check_job(v, p, t, k0, n, cap, alleles_cap, workspace, workspace_bytes_, &why)) return brcside::refuse(h, why);
    if (int rc = brcside::resident(h, v, brcside::ONE_VIEW)) return rc;
    if (n == 0 || t->m == 0) {
        if (counts) counts[0] = counts[1] = 0;
        if (allele_off) allele_off[0] = 0;
        if (status) *status = 0;
        return BRC_OK;
    }
    const Job J = make_job(v, p, t, k0, n, workspace, counts, npos, shift, flags, group, cap, alleles_cap, pos, lib, len, rep_read, rep_qpos, members, istat,
                           fstat, metrics, allele_off, alleles, status);
    if (!wants_anything(J)) return BRC_OK;
    if (status) *status = 0;
    brcside::start(h);
    if (J.cnt) for (int64_t d = 0; d < n; ++d) J.cnt[d] = 0;
    for (int64_t r = J.m; r-- > 0;) shift_lane(J, r);
    if (wants_table(J)) {
        J.tot[0] = scan(J.cnt, (uint64_t)n, J.start);
        for (int64_t r = J.m; r-- > 0;) place_lane(J, r);
        for (int64_t j = J.m; j-- > 0;) rank_lane(J, j);
        for (int64_t j = J.m; j-- > 0;) heads_lane(J, j);
        J.tot[1] = scan(J.head, J.tot[0], J.gidx);
        if (counts) counts[0] = J.tot[1];
        J.tot[2] = scan(J.alen, J.tot[0], J.aoff);
        if (counts) counts[1] = J.tot[2];
        if (J.o_group || wants_records(J)) for (int64_t j = J.m + 1; j-- > 0;) merge_lane(J, j);
    }
    return brcside::done(h, J);
}

}  // extern "C"
