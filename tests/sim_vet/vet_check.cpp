// Driver of the sanitizer build (make asan): runs brc_vet_sites of the CPU build over one serialized pair of views and a list of calls.
//   in : the two views as tests/sim_select/select_check.cpp reads them —
//        i32 Lp, i32 pos0, i64 P, i64 PS, u64 n_xagg, i32 has_unavail, i32 n_calls,
//        u32 ncol[Lp*PS], depth[Lp*PS], slotid[Lp*PS], si[Lp*2*9*PS], f32 sf[Lp*2*4*PS], u32 unavail[PS] (has_unavail), n_xagg records of 64 bytes,
//        u64 n_slots, n_slots records of 72 bytes, i32 has_ref, i64 ref_lo, ref_hi, ref_len, i64 ref_bytes, the slice —
//        n_calls x { i64 n, i32 has_alt, i32 has_lib_on, i32 want (1 fail | 2 keep | 4 vals | 8 status), u32 tests, u32 x 8 and f32 x 14: the
//                    thresholds in brc_vet_params' order, i32 idx[n], u32 alt[n] (has_alt), u8 lib_on[Lp] (has_lib_on) }
//   out: per call { i32 rc, u32 status, u32 fail[Lp*4*n], keep[n], vals[Lp*4*20*n] } — a destination that was not wanted comes back as it was filled
// Sources are heap blocks of exactly the views' sizes; idx and alt have exactly n elements, lib_on exactly Lp bytes, the scratch exactly
// brc_vet_workspace bytes, every destination exactly [planes][n] elements (dst_stride == n) — the least the contract allows — pre-filled
// with 0xA5 bytes: a load outside the views or the lists, or a store outside the scratch or a destination, is a report.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/brc_vet.h"

template <class T> static T* slurp(FILE* in, size_t n) {
    T* p = (T*)malloc(n ? n * sizeof(T) : 1);
    if (n && fread(p, sizeof(T), n, in) != n) { fprintf(stderr, "short case file\n"); exit(2); }
    return p;
}
static void* filled(size_t bytes) { void* p = malloc(bytes ? bytes : 1); memset(p, 0xA5, bytes ? bytes : 1); return p; }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: vet_check_asan case.bin results.bin\n"); return 2; }
    FILE* in = fopen(argv[1], "rb"); FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open files\n"); return 2; }
    int32_t Lp, pos0, has_unavail, n_calls; int64_t P, PS; uint64_t n_xagg;
    if (fread(&Lp, 4, 1, in) != 1 || fread(&pos0, 4, 1, in) != 1 || fread(&P, 8, 1, in) != 1 || fread(&PS, 8, 1, in) != 1 || fread(&n_xagg, 8, 1, in) != 1 ||
        fread(&has_unavail, 4, 1, in) != 1 || fread(&n_calls, 4, 1, in) != 1) return 2;
    const size_t L = (size_t)Lp, S = (size_t)PS;
    brc_device_view v; memset(&v, 0, sizeof v);
    v.memory = BRC_MEM_HOST; v.n_lib = Lp; v.pos0 = pos0; v.n_pos = P; v.stride = PS;
    uint32_t* ncol = slurp<uint32_t>(in, L * S); uint32_t* depth = slurp<uint32_t>(in, L * S); uint32_t* slotid = slurp<uint32_t>(in, L * S);
    uint32_t* si = slurp<uint32_t>(in, L * 2 * BRC_NI * S); float* sf = slurp<float>(in, L * 2 * BRC_NF * S);
    uint32_t* unavail = has_unavail ? slurp<uint32_t>(in, S) : nullptr;
    void* xagg = aligned_alloc(64, n_xagg ? n_xagg * 64 : 64);      // (records: 16-byte aligned as in the engine)
    if (n_xagg && fread(xagg, 64, n_xagg, in) != n_xagg) return 2;
    v.ncol = ncol; v.depth = depth; v.slotid = slotid; v.si = si; v.sf = sf; v.unavail = unavail; v.xagg = n_xagg ? xagg : nullptr; v.n_xagg = n_xagg;
    brc_device_indels d; memset(&d, 0, sizeof d);
    d.memory = BRC_MEM_HOST; d.n_lib = Lp; d.pos0 = pos0; d.n_pos = P;
    int32_t has_ref; int64_t ref_bytes;
    if (fread(&d.n_slots, 8, 1, in) != 1) return 2;
    char* slots = slurp<char>(in, (size_t)d.n_slots * 72);
    if (fread(&has_ref, 4, 1, in) != 1 || fread(&d.ref_lo, 8, 1, in) != 1 || fread(&d.ref_hi, 8, 1, in) != 1 || fread(&d.ref_len, 8, 1, in) != 1 ||
        fread(&ref_bytes, 8, 1, in) != 1 || ref_bytes < 0) return 2;
    char* ref = slurp<char>(in, (size_t)ref_bytes);
    // (the filter reads no indel record and spells no allele: those arrays are one byte each, and any load from them is a report)
    uint8_t* seq4 = (uint8_t*)malloc(1); uint64_t* seq_off = (uint64_t*)malloc(1); int32_t* l_qseq = (int32_t*)malloc(1);
    if (d.n_slots) { d.slots = slots; d.seq4 = seq4; d.seq_off = seq_off; d.l_qseq = l_qseq; }
    d.ref = has_ref ? ref : nullptr;
    brc_vet* h = nullptr;
    if (brc_vet_create(0, &h) != BRC_OK) return 2;
    for (int w = 0; w < n_calls; ++w) {
        int64_t n; int32_t has_alt, has_on, want; brc_vet_params p; memset(&p, 0, sizeof p);
        if (fread(&n, 8, 1, in) != 1 || fread(&has_alt, 4, 1, in) != 1 || fread(&has_on, 4, 1, in) != 1 || fread(&want, 4, 1, in) != 1 ||
            fread(&p.tests, 4, 1, in) != 1 || fread(&p.min_depth, 4, 8, in) != 8 || fread(&p.min_var_readpos, 4, 14, in) != 14 || n < 0) return 2;
        int32_t* idx = slurp<int32_t>(in, (size_t)n);
        uint32_t* alt = slurp<uint32_t>(in, has_alt ? (size_t)n : 0);
        uint8_t* on = slurp<uint8_t>(in, has_on ? L : 0);
        p.lib_on = has_on ? on : nullptr;
        const int64_t wsb = brc_vet_workspace(&v, n);
        void* ws = filled((size_t)wsb);
        const size_t N = (size_t)n;
        uint32_t* fail = (uint32_t*)filled(L * 4 * N * 4); uint32_t* keep = (uint32_t*)filled(N * 4); float* vals = (float*)filled(L * 4 * BRC_VET_NVAL * N * 4);
        uint32_t* status = (uint32_t*)filled(4);
        const int32_t rc = brc_vet_sites(h, &v, &d, &p, idx, has_alt ? alt : nullptr, n, n, (want & 1) ? fail : nullptr, (want & 2) ? keep : nullptr,
                                         (want & 4) ? vals : nullptr, (want & 8) ? status : nullptr, ws, nullptr);
        fwrite(&rc, 4, 1, out); fwrite(status, 4, 1, out);
        fwrite(fail, 4, L * 4 * N, out); fwrite(keep, 4, N, out); fwrite(vals, 4, L * 4 * BRC_VET_NVAL * N, out);
        free(ws); free(fail); free(keep); free(vals); free(status); free(idx); free(alt); free(on);
    }
    brc_vet_destroy(h);
    free(ncol); free(depth); free(slotid); free(si); free(sf); free(unavail); free(xagg); free(slots); free(ref); free(seq4); free(seq_off); free(l_qseq);
    fclose(in); fclose(out);
    printf("%d calls\n", n_calls);
    return 0;
}
