// Driver of the sanitizer build (make asan): runs brc_panel_gather of the CPU build over one serialized view and a list of index lists.
//   in : i32 Lp, i32 pos0, i64 P, i64 PS, u64 n_xagg, i32 has_unavail, i32 n_lists,
//        u32 ncol[Lp*PS], depth[Lp*PS], slotid[Lp*PS], si[Lp*2*9*PS], f32 sf[Lp*2*4*PS], u32 unavail[PS] (has_unavail), n_xagg records of 64 bytes,
//        n_lists x { i64 n, dst_stride, i32 idx[n] }
//   out: per list { i32 rc, u32 status, ncol, depth, unavail, istat, fstat, metrics }, every buffer whole
// Sources are heap blocks of exactly the view's sizes, a list is a heap block of exactly n indices, the status one word of its own;
// every destination is a heap block of exactly (planes - 1) * dst_stride + n elements — the least the contract allows — pre-filled
// with 0xA5 bytes: a load outside the view or the list, or a store outside a destination, is a report; a store into the padding
// between two planes shows in the output.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/brc_panel.h"

template <class T> static T* slurp(FILE* in, size_t n) {
    T* p = (T*)malloc(n ? n * sizeof(T) : 1);
    if (n && fread(p, sizeof(T), n, in) != n) { fprintf(stderr, "short case file\n"); exit(2); }
    return p;
}
struct Dst { void* p; size_t elems; };
static Dst dst(size_t planes, int64_t n, int64_t ds) {
    Dst d; d.elems = n > 0 ? (planes - 1) * (size_t)ds + (size_t)n : 0;
    d.p = malloc(d.elems ? d.elems * 4 : 1); memset(d.p, 0xA5, d.elems ? d.elems * 4 : 1);
    return d;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: panel_check_asan case.bin results.bin\n"); return 2; }
    FILE* in = fopen(argv[1], "rb"); FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open files\n"); return 2; }
    int32_t Lp, pos0, has_unavail, n_lists; int64_t P, PS; uint64_t n_xagg;
    if (fread(&Lp, 4, 1, in) != 1 || fread(&pos0, 4, 1, in) != 1 || fread(&P, 8, 1, in) != 1 || fread(&PS, 8, 1, in) != 1 || fread(&n_xagg, 8, 1, in) != 1 ||
        fread(&has_unavail, 4, 1, in) != 1 || fread(&n_lists, 4, 1, in) != 1) return 2;
    const size_t L = (size_t)Lp, S = (size_t)PS;
    brc_device_view v; memset(&v, 0, sizeof v);
    v.memory = BRC_MEM_HOST; v.n_lib = Lp; v.pos0 = pos0; v.n_pos = P; v.stride = PS;
    uint32_t* ncol = slurp<uint32_t>(in, L * S); uint32_t* depth = slurp<uint32_t>(in, L * S); uint32_t* slotid = slurp<uint32_t>(in, L * S);
    uint32_t* si = slurp<uint32_t>(in, L * 2 * BRC_NI * S); float* sf = slurp<float>(in, L * 2 * BRC_NF * S);
    uint32_t* unavail = has_unavail ? slurp<uint32_t>(in, S) : nullptr;
    // (records: 16-byte aligned as in the engine)
    void* xagg = aligned_alloc(64, n_xagg ? n_xagg * 64 : 64);
    if (n_xagg && fread(xagg, 64, n_xagg, in) != n_xagg) return 2;
    v.ncol = ncol; v.depth = depth; v.slotid = slotid; v.si = si; v.sf = sf; v.unavail = unavail; v.xagg = xagg; v.n_xagg = n_xagg;
    brc_panel* h = nullptr;
    if (brc_panel_create(0, &h) != BRC_OK) return 2;
    for (int w = 0; w < n_lists; ++w) {
        int64_t n, ds;
        if (fread(&n, 8, 1, in) != 1 || fread(&ds, 8, 1, in) != 1 || n < 0) return 2;
        int32_t* idx = slurp<int32_t>(in, (size_t)n);
        uint32_t* status = (uint32_t*)malloc(4); memset(status, 0xA5, 4);
        Dst d[6] = {dst(L, n, ds), dst(L, n, ds), dst(1, n, ds), dst(L * BRC_NBUCKET * BRC_NI, n, ds), dst(L * BRC_NBUCKET * BRC_NF, n, ds),
                    dst(L * BRC_NBUCKET * BRC_NMETRIC, n, ds)};
        const int32_t rc = brc_panel_gather(h, &v, idx, n, ds, (uint32_t*)d[0].p, (uint32_t*)d[1].p, (uint32_t*)d[2].p, (uint32_t*)d[3].p, (float*)d[4].p,
                                            (float*)d[5].p, status, nullptr);
        fwrite(&rc, 4, 1, out); fwrite(status, 4, 1, out);
        for (int i = 0; i < 6; ++i) { fwrite(d[i].p, 4, d[i].elems, out); free(d[i].p); }
        free(idx); free(status);
    }
    brc_panel_destroy(h);
    free(ncol); free(depth); free(slotid); free(si); free(sf); free(unavail); free(xagg);
    fclose(in); fclose(out);
    printf("%d lists\n", n_lists);
    return 0;
}
