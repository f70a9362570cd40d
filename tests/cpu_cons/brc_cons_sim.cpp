// CPU build of the consensus caller's C-ABI (include/brc_cons.h) over brc_cons_core.h: the test counterpart of libbrc_cons_hip.so, as
// libbrc_sim.so is the engine's.  The launches of the gfx950 library run here as loops in the same order — every lane of the
// third-allele records, every lane of the table records, a serial scan of the difference array, every position lane, a serial scan
// of the lengths, every position lane of the emit — on host memory: views with memory == BRC_MEM_HOST (what libbrc_sim.so hands out),
// table, scratch and destinations in host memory.  Every lane loop runs from the LAST lane to the first: nothing may depend on the
// order of the lanes.  Test infrastructure only.
#include <string.h>

#include "../../bam_readcount_amd/csrc/brc_cons_core.h"
#include "../sim_side.h"

using namespace brccons;

struct brc_cons : brcside::Handle {};

// out[i] = the sum of in[0 .. i) modulo 2^32, out[n] = the total (brc_side_scan.h's contract)
static uint32_t scan(const uint32_t* in, int64_t n, uint32_t* out) {
    uint32_t acc = 0;
    for (int64_t i = 0; i < n; ++i) { out[i] = acc; acc += in[i]; }
    out[n] = acc;
    return acc;
}

extern "C" {

const char* brc_cons_kind(void) { return "sim"; }
int brc_cons_create(int device, brc_cons** out) { return brcside::create(device, out); }
void brc_cons_destroy(brc_cons* h) { brcside::destroy(h); }
const char* brc_cons_last_error(const brc_cons* h) { return brcside::last_error(h); }
void brc_cons_last_timing(const brc_cons* h, double* kernel_s, uint64_t* bytes_read, uint64_t* bytes_written) { brcside::last_timing(h, kernel_s, bytes_read, bytes_written); }
int64_t brc_cons_workspace(const brc_device_view* v, int64_t n, int64_t m) { return workspace_bytes(v, n, m); }

int brc_cons_call(brc_cons* h, const brc_device_view* v, const brc_device_indels* d, const brc_cons_params* p, const brc_cons_table* t, int64_t k0, int64_t n,
                  int64_t dst_stride, int64_t seq_cap, uint32_t* counts, uint8_t* call, uint32_t* cnt, uint32_t* ins_rec, uint32_t* off, uint8_t* seq,
                  uint32_t* status, void* workspace, void*) {
    if (!h) return BRC_E_ARG;
    brcside::clear(h);
    const char* why = "";
    if (check_job(v, d, p, t, k0, n, dst_stride, seq_cap, workspace, &why)) return brcside::refuse(h, why);
    if (int rc = brcside::resident(h, v, brcside::TWO_VIEWS)) return rc;
    if (status) *status = 0;
    if (n == 0) {
        if (counts) *counts = 0;
        if (off) *off = 0;
        return BRC_OK;
    }
    const Job J = make_job(v, d, p, t, k0, n, dst_stride, seq_cap, counts, call, cnt, ins_rec, off, seq, status, workspace);
    if (!wants_sites(J) && !(status && walks_table(J))) return BRC_OK;
    brcside::start(h);
    if (walks_records(J) && wants_sites(J)) {
        memset(J.head, 0xff, (size_t)n * sizeof(uint32_t));
        for (uint64_t r = J.n_xagg; r-- > 0;) link_lane(J, r);
    }
    if (walks_table(J)) {
        memset(J.diff, 0, (size_t)n * sizeof(uint32_t));
        memset(J.run, 0xff, (size_t)n * sizeof(uint32_t));
        for (int64_t r = J.m; r-- > 0;) record_lane(J, r);
        if (wants_sites(J)) *J.tot = scan(J.diff, n, J.dcov);
    }
    if (wants_sites(J)) {
        for (int64_t j = n; j-- > 0;) {
            const uint8_t ch = (uint8_t)site_lane(J, j);
            if (J.o_call) J.o_call[j] = ch;
            if (aligned(J)) { if (J.o_seq && j < J.cap) J.o_seq[j] = ch; }
            else J.wcall[j] = ch;
        }
        if (wants_scan(J)) {
            *J.tot = scan(J.lens, n, J.offs);
            if (J.o_counts) *J.o_counts = *J.tot;
        }
        if (wants_emit(J)) for (int64_t j = n; j-- > 0;) emit_lane(J, j);
    }
    return brcside::done(h, J);
}

}  // extern "C"
