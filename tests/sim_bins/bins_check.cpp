// Driver of the sanitizer build (make asan): runs brc_bins_reduce of the CPU build over one serialized pair of views and a list of calls.
//   in : the two views as tests/sim_select/select_check.cpp reads them —
//        i32 Lp, i32 pos0, i64 P, i64 PS, u64 n_xagg, i32 has_unavail, i32 n_calls,
//        u32 ncol[Lp*PS], depth[Lp*PS], slotid[Lp*PS], si[Lp*2*9*PS], f32 sf[Lp*2*4*PS], u32 unavail[PS] (has_unavail), n_xagg records of 64 bytes,
//        u64 n_slots, n_slots records of 72 bytes, i32 has_ref, i64 ref_lo, ref_hi, ref_len, i64 ref_bytes, the slice —
//        then n_calls x { i64 k0, n, width, n_bins, dst_stride, i32 n_thr, n_hist, u32 thr[8], i32 want (1 sums | 2 covered | 4 hist | 8 status),
//                         i32 has_edges, i32 edges[n_bins + 1] (has_edges) }
//   out: per call { i32 rc, u32 status, u64 sums[Lp*12*dst_stride], u64 covered[Lp*n_thr*dst_stride], u64 hist[Lp*n_hist] } — a destination that
//        was not wanted comes back as it was filled
// Sources are heap blocks of exactly the views' sizes, the edge list has exactly n_bins + 1 elements, the destinations exactly the
// contract's sizes, pre-filled with 0xA5 bytes: a load outside the views or the list, or a store outside a destination, is a report; a
// store into the padding behind n_bins shows in the output.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/brc_bins.h"

template <class T> static T* slurp(FILE* in, size_t n) {
    T* p = (T*)malloc(n ? n * sizeof(T) : 1);
    if (n && fread(p, sizeof(T), n, in) != n) { fprintf(stderr, "short case file\n"); exit(2); }
    return p;
}
static void* filled(size_t bytes) { void* p = malloc(bytes ? bytes : 1); memset(p, 0xA5, bytes ? bytes : 1); return p; }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: bins_check_asan case.bin results.bin\n"); return 2; }
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
    v.ncol = ncol; v.depth = depth; v.slotid = slotid; v.si = si; v.sf = sf; v.unavail = unavail; v.xagg = xagg; v.n_xagg = n_xagg;
    brc_device_indels d; memset(&d, 0, sizeof d);
    d.memory = BRC_MEM_HOST; d.n_lib = Lp; d.pos0 = pos0; d.n_pos = P;
    int32_t has_ref; int64_t ref_bytes;
    if (fread(&d.n_slots, 8, 1, in) != 1) return 2;
    char* slots = slurp<char>(in, (size_t)d.n_slots * 72);
    if (fread(&has_ref, 4, 1, in) != 1 || fread(&d.ref_lo, 8, 1, in) != 1 || fread(&d.ref_hi, 8, 1, in) != 1 || fread(&d.ref_len, 8, 1, in) != 1 ||
        fread(&ref_bytes, 8, 1, in) != 1 || ref_bytes < 0) return 2;
    char* ref = slurp<char>(in, (size_t)ref_bytes);
    // (the reduction spells no allele: the arrays that do are one byte each, and any load from them is a report)
    uint8_t* seq4 = (uint8_t*)malloc(1); uint64_t* seq_off = (uint64_t*)malloc(1); int32_t* l_qseq = (int32_t*)malloc(1);
    if (d.n_slots) { d.slots = slots; d.seq4 = seq4; d.seq_off = seq_off; d.l_qseq = l_qseq; }
    d.ref = has_ref ? ref : nullptr;
    brc_bins* h = nullptr;
    if (brc_bins_create(0, &h) != BRC_OK) return 2;
    for (int w = 0; w < n_calls; ++w) {
        int64_t k0, n, ds; brc_bins_params p; memset(&p, 0, sizeof p); int32_t want, has_edges;
        if (fread(&k0, 8, 1, in) != 1 || fread(&n, 8, 1, in) != 1 || fread(&p.width, 8, 1, in) != 1 || fread(&p.n_bins, 8, 1, in) != 1 || fread(&ds, 8, 1, in) != 1 ||
            fread(&p.n_thr, 4, 1, in) != 1 || fread(&p.n_hist, 4, 1, in) != 1 || fread(p.thr, 4, BRC_BINS_MAX_THR, in) != BRC_BINS_MAX_THR ||
            fread(&want, 4, 1, in) != 1 || fread(&has_edges, 4, 1, in) != 1 || ds < 0 || p.n_bins < 0 || p.n_thr < 0 || p.n_hist < 0) return 2;
        int32_t* edges = slurp<int32_t>(in, has_edges ? (size_t)p.n_bins + 1 : 0);
        p.edges = has_edges ? edges : nullptr;
        const size_t ns = L * BRC_BINS_NSUM * (size_t)ds, nc = L * (size_t)p.n_thr * (size_t)ds, nh = L * (size_t)p.n_hist;
        uint64_t* sums = (uint64_t*)filled(ns * 8); uint64_t* cov = (uint64_t*)filled(nc * 8); uint64_t* hist = (uint64_t*)filled(nh * 8);
        uint32_t* status = (uint32_t*)filled(4);
        const int32_t rc = brc_bins_reduce(h, &v, &d, &p, k0, n, (want & 1) ? sums : nullptr, (want & 2) ? cov : nullptr, (want & 4) ? hist : nullptr, ds,
                                           (want & 8) ? status : nullptr, nullptr);
        fwrite(&rc, 4, 1, out); fwrite(status, 4, 1, out); fwrite(sums, 8, ns, out); fwrite(cov, 8, nc, out); fwrite(hist, 8, nh, out);
        free(sums); free(cov); free(hist); free(status); free(edges);
    }
    brc_bins_destroy(h);
    free(ncol); free(depth); free(slotid); free(si); free(sf); free(unavail); free(xagg); free(slots); free(ref); free(seq4); free(seq_off); free(l_qseq);
    fclose(in); fclose(out);
    printf("%d calls\n", n_calls);
    return 0;
}
