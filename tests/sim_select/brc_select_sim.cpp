// CPU build of the site selection's C-ABI (include/brc_select.h) over brc_select_core.h: the test counterpart of libbrc_select_hip.so,
// as libbrc_sim.so is the engine's.  The launches of the gfx950 library run here as loops on host memory: views with memory ==
// BRC_MEM_HOST (what libbrc_sim.so hands out), scratch and destinations in host memory.  The record, slot and position loops run from the
// LAST lane to the first: nothing may depend on the order of the lanes (a position's list of records comes out reversed against an
// ascending run); with BRC_SIM_LANES=forward in the environment the record loop runs from the first record to the last, so that a test
// can show a result under both orders.  The compaction is a serial loop.  Test infrastructure only.
#include <stdlib.h>
#include <string.h>

#include "../../bam_readcount_amd/csrc/brc_select_core.h"
#include "../sim_side.h"

using namespace brcselect;

struct brc_select : brcside::Handle {};

extern "C" {

const char* brc_select_kind(void) { return "sim"; }
int brc_select_create(int device, brc_select** out) { return brcside::create(device, out); }
void brc_select_destroy(brc_select* h) { brcside::destroy(h); }
const char* brc_select_last_error(const brc_select* h) { return brcside::last_error(h); }
void brc_select_last_timing(const brc_select* h, double* kernel_s, uint64_t* bytes_read, uint64_t* bytes_written) { brcside::last_timing(h, kernel_s, bytes_read, bytes_written); }

int64_t brc_select_workspace(const brc_device_view* v, const brc_device_indels*, int64_t n) { return workspace_bytes(v, n); }

int brc_select_sites(brc_select* h, const brc_device_view* v, const brc_device_indels* d, const brc_select_params* p, int64_t k0, int64_t n, int64_t cap,
                     int32_t* idx, uint32_t* why_, uint32_t* counts, void* workspace, void*) {
    if (!h) return BRC_E_ARG;
    brcside::clear(h);
    const char* why = "";
    if (check_job(v, d, p, k0, n, cap, workspace, &why)) return brcside::refuse(h, why);
    if (int rc = brcside::resident(h, v, brcside::TWO_VIEWS)) return rc;
    if (n == 0) { if (counts) *counts = 0; return BRC_OK; }
    const Job J = make_job(v, d, p, k0, n, cap, idx, why_, counts, workspace);
    if (!counts && !wants_list(J)) return BRC_OK;
    brcside::start(h);
    if (walks_records(J)) {
        memset(J.head, 0xff, (size_t)n * sizeof(uint32_t));
        const char* order = getenv("BRC_SIM_LANES");
        if (order && !strcmp(order, "forward")) { for (uint64_t r = 0; r < J.n_xagg; ++r) link_lane(J, r); }
        else for (uint64_t r = J.n_xagg; r-- > 0;) link_lane(J, r);
    }
    if (walks_slots(J)) {
        memset(J.flag, 0, (size_t)n * sizeof(uint32_t));
        for (uint64_t s = J.n_slots; s-- > 0;) flag_lane(J, s);
    }
    for (int64_t j = n - 1; j >= 0; --j) (void)why_lane(J, j);
    // the three launches of the compaction: every workgroup's count, their exclusive scan, the stores
    const uint64_t nb = blocks_of((uint64_t)n);
    for (uint64_t b = 0; b < nb; ++b) {
        uint32_t s = 0;
        for (int64_t j = (int64_t)b * BLOCK; j < n && j < (int64_t)(b + 1) * BLOCK; ++j) s += J.flag[j] != 0u;
        J.part[b] = s;
    }
    uint32_t carry = 0;
    for (uint64_t b = 0; b < nb; ++b) { const uint32_t s = J.part[b]; J.part[b] = carry; carry += s; }
    *J.tot = carry;
    if (counts) *counts = carry;
    if (wants_list(J)) {
        for (uint64_t b = nb; b-- > 0;) {
            uint64_t at = J.part[b];
            for (int64_t j = (int64_t)b * BLOCK; j < n && j < (int64_t)(b + 1) * BLOCK; ++j) { emit_lane(J, j, J.flag[j], at); at += J.flag[j] != 0u; }
        }
    }
    return brcside::done(h, J);
}

}  // extern "C"
