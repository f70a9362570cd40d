// CPU build of the depth-class intervals' C-ABI (include/brc_runs.h) over brc_runs_core.h: the test counterpart of libbrc_runs_hip.so,
// as libbrc_sim.so is the engine's.  The launches of the gfx950 library run here as loops on host memory: views with memory ==
// BRC_MEM_HOST (what libbrc_sim.so hands out), scratch and destinations in host memory.  The position loops run from the LAST lane to
// the first: nothing may depend on the order of the lanes.  The ranks are serial loops per workgroup, the scan of the workgroups'
// counts a serial loop without the device's carry.  Test infrastructure only.
#include <string.h>

#include "../../bam_readcount_amd/csrc/brc_runs_core.h"
#include "../sim_side.h"

using namespace brcruns;

struct brc_runs : brcside::Handle {};

// the class of window element j's neighbours, from the scratch (NO_CLASS outside the window): what the device's halo and k_runs_emit read
static inline uint32_t left_of(const Job& J, int64_t j) { return j > 0 ? J.w_cls[j - 1] : NO_CLASS; }
static inline uint32_t right_of(const Job& J, int64_t j) { return j + 1 < J.n ? J.w_cls[j + 1] : NO_CLASS; }

extern "C" {

const char* brc_runs_kind(void) { return "sim"; }
int brc_runs_create(int device, brc_runs** out) { return brcside::create(device, out); }
void brc_runs_destroy(brc_runs* h) { brcside::destroy(h); }
const char* brc_runs_last_error(const brc_runs* h) { return brcside::last_error(h); }
void brc_runs_last_timing(const brc_runs* h, double* kernel_s, uint64_t* bytes_read, uint64_t* bytes_written) { brcside::last_timing(h, kernel_s, bytes_read, bytes_written); }
int64_t brc_runs_workspace(int64_t n) { return workspace_bytes(n); }

int brc_runs_find(brc_runs* h, const brc_device_view* v, const brc_device_indels* d, const brc_runs_params* p, int64_t k0, int64_t n, int64_t cap,
                  int32_t* start, int32_t* end, uint32_t* cls, uint32_t* counts, uint64_t* per_class, void* workspace, void*) {
    if (!h) return BRC_E_ARG;
    brcside::clear(h);
    const char* why = "";
    if (check_job(v, d, p, k0, n, cap, workspace, &why)) return brcside::refuse(h, why);
    if (int rc = brcside::resident(h, v, d ? brcside::TWO_VIEWS : brcside::ONE_VIEW)) return rc;
    const Job J = make_job(v, d, p, k0, n, cap, start, end, cls, counts, per_class, workspace);
    if (n == 0) {
        if (counts) *counts = 0;
        if (per_class) memset(per_class, 0, n_class(J) * sizeof(uint64_t));
        return BRC_OK;
    }
    if (!per_class && !wants_ranks(J)) return BRC_OK;
    brcside::start(h);
    if (per_class) memset(per_class, 0, n_class(J) * sizeof(uint64_t));
    for (int64_t j = n - 1; j >= 0; --j) {
        const uint32_t c = class_lane(J, j);
        J.w_cls[j] = c;
        if (per_class) add64(per_class + c, 1u);
    }
    if (wants_ranks(J)) {
        // the launches of the compaction: every workgroup's two counts, their exclusive scans, the stores
        const uint64_t nb = blocks_of((uint64_t)n);
        for (uint64_t b = nb; b-- > 0;) {
            uint32_t s = 0, e = 0;
            for (int64_t j = (int64_t)b * BLOCK; j < n && j < (int64_t)(b + 1) * BLOCK; ++j) {
                s += starts_run(J, left_of(J, j), J.w_cls[j]); e += ends_run(J, J.w_cls[j], right_of(J, j));
            }
            J.part_s[b] = s; J.part_e[b] = e;
        }
        uint64_t carry = 0;
        for (uint64_t b = 0; b < nb; ++b) {
            const uint64_t x = pack(J.part_s[b], J.part_e[b]);
            J.part_s[b] = starts_of(carry); J.part_e[b] = ends_of(carry);
            carry += x;
        }
        if (counts) *counts = starts_of(carry);
        if (wants_list(J)) {
            for (uint64_t b = nb; b-- > 0;) {
                uint64_t at_s = J.part_s[b], at_e = J.part_e[b];
                for (int64_t j = (int64_t)b * BLOCK; j < n && j < (int64_t)(b + 1) * BLOCK; ++j) {
                    const uint32_t c = J.w_cls[j];
                    const bool is_start = starts_run(J, left_of(J, j), c), is_end = ends_run(J, c, right_of(J, j));
                    emit_lane(J, j, c, is_start, at_s, is_end, at_e);
                    at_s += is_start; at_e += is_end;
                }
            }
        }
    }
    return brcside::done(h, J);
}

}  // extern "C"
