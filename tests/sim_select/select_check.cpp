// Driver of the sanitizer build (make asan): runs brc_select_sites of the CPU build over one serialized pair of views and a list of calls.
//   in : the view as tests/sim_dense/dense_check.cpp reads it —
//        i32 Lp, i32 pos0, i64 P, i64 PS, u64 n_xagg, i32 has_unavail, i32 n_calls,
//        u32 ncol[Lp*PS], depth[Lp*PS], slotid[Lp*PS], si[Lp*2*9*PS], f32 sf[Lp*2*4*PS], u32 unavail[PS] (has_unavail), n_xagg records of 64 bytes
//        — then the indel view: u64 n_slots, n_slots records of 72 bytes, i32 has_ref, i64 ref_lo, ref_hi, ref_len, i64 ref_bytes, the slice,
//        n_calls x { i64 k0, n, cap, u32 flags, min_depth, min_alt, frac_num, frac_den, ctl_min_depth, ctl_max_alt, ctl_frac_num, ctl_frac_den,
//                    i32 has_role, i32 want (1 idx | 2 why | 4 counts), u8 role[Lp] (has_role) }
//   out: per call { i32 rc, u32 counts, i32 idx[cap], u32 why[cap] } — a destination that was not wanted comes back as it was filled
// Sources are heap blocks of exactly the views' sizes; the scratch has exactly brc_select_workspace bytes, idx and why exactly cap
// elements, counts one word — the least the contract allows — pre-filled with 0xA5 bytes: a load outside the views, or a store outside
// the scratch or a destination, is a report; a store behind the list shows in the output.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/brc_select.h"

template <class T> static T* slurp(FILE* in, size_t n) {
    T* p = (T*)malloc(n ? n * sizeof(T) : 1);
    if (n && fread(p, sizeof(T), n, in) != n) { fprintf(stderr, "short case file\n"); exit(2); }
    return p;
}
static void* filled(size_t bytes) { void* p = malloc(bytes ? bytes : 1); memset(p, 0xA5, bytes ? bytes : 1); return p; }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: select_check_asan case.bin results.bin\n"); return 2; }
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
    // (the selector spells no allele: the arrays that do are one byte each, and any load from them is a report)
    uint8_t* seq4 = (uint8_t*)malloc(1); uint64_t* seq_off = (uint64_t*)malloc(1); int32_t* l_qseq = (int32_t*)malloc(1);
    if (d.n_slots) { d.slots = slots; d.seq4 = seq4; d.seq_off = seq_off; d.l_qseq = l_qseq; }
    d.ref = has_ref ? ref : nullptr;
    brc_select* h = nullptr;
    if (brc_select_create(0, &h) != BRC_OK) return 2;
    for (int w = 0; w < n_calls; ++w) {
        int64_t k0, n, cap; brc_select_params p; memset(&p, 0, sizeof p); int32_t has_role, want;
        if (fread(&k0, 8, 1, in) != 1 || fread(&n, 8, 1, in) != 1 || fread(&cap, 8, 1, in) != 1 || fread(&p.flags, 4, 9, in) != 9 ||
            fread(&has_role, 4, 1, in) != 1 || fread(&want, 4, 1, in) != 1 || cap < 0) return 2;
        uint8_t* role = slurp<uint8_t>(in, has_role ? L : 0);
        p.role = has_role ? role : nullptr;
        const int64_t wsb = brc_select_workspace(&v, &d, n);
        void* ws = filled((size_t)wsb);
        int32_t* idx = (int32_t*)filled((size_t)cap * 4); uint32_t* why = (uint32_t*)filled((size_t)cap * 4); uint32_t* counts = (uint32_t*)filled(4);
        const int32_t rc = brc_select_sites(h, &v, &d, &p, k0, n, cap, (want & 1) ? idx : nullptr, (want & 2) ? why : nullptr, (want & 4) ? counts : nullptr,
                                            wsb ? ws : nullptr, nullptr);
        fwrite(&rc, 4, 1, out); fwrite(counts, 4, 1, out); fwrite(idx, 4, (size_t)cap, out); fwrite(why, 4, (size_t)cap, out);
        free(ws); free(idx); free(why); free(counts); free(role);
    }
    brc_select_destroy(h);
    free(ncol); free(depth); free(slotid); free(si); free(sf); free(unavail); free(xagg); free(slots); free(ref); free(seq4); free(seq_off); free(l_qseq);
    fclose(in); fclose(out);
    printf("%d calls\n", n_calls);
    return 0;
}
