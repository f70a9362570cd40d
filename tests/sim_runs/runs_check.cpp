// Driver of the sanitizer build (make asan): runs brc_runs_find of the CPU build over one serialized pair of views and a list of calls.
//   in : the two views as tests/sim_select/select_check.cpp reads them —
//        i32 Lp, i32 pos0, i64 P, i64 PS, u64 n_xagg, i32 has_unavail, i32 n_calls,
//        u32 ncol[Lp*PS], depth[Lp*PS], slotid[Lp*PS], si[Lp*2*9*PS], f32 sf[Lp*2*4*PS], u32 unavail[PS] (has_unavail), n_xagg records of 64 bytes,
//        u64 n_slots, n_slots records of 72 bytes, i32 has_ref, i64 ref_lo, ref_hi, ref_len, i64 ref_bytes, the slice —
//        then n_calls x { i64 k0, n, cap, u32 combine, n_cut, keep, flags, u32 cut[15], i32 has_role, i32 want (1 start | 2 end | 4 cls | 8 counts |
//                         16 per_class), i32 with_indels, u8 role[Lp] (has_role) }
//   out: per call { i32 rc, u32 counts, i32 start[cap], i32 end[cap], u32 cls[cap], u64 per_class[n_cut + 2] } — a destination that was not
//        wanted comes back as it was filled
// Sources are heap blocks of exactly the views' sizes; the scratch has exactly brc_runs_workspace bytes, start / end / cls exactly cap
// elements, counts one word, per_class exactly n_cut + 2 elements, the role array exactly Lp bytes —
// the least the contract allows — pre-filled with 0xA5 bytes: a load outside the views, or a store outside the scratch or a
// destination, is a report; a store behind the list shows in the output.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/brc_runs.h"

template <class T> static T* slurp(FILE* in, size_t n) {
    T* p = (T*)malloc(n ? n * sizeof(T) : 1);
    if (n && fread(p, sizeof(T), n, in) != n) { fprintf(stderr, "short case file\n"); exit(2); }
    return p;
}
static void* filled(size_t bytes) { void* p = malloc(bytes ? bytes : 1); memset(p, 0xA5, bytes ? bytes : 1); return p; }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: runs_check_asan case.bin results.bin\n"); return 2; }
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
    // (the intervals read no record and spell no allele: those arrays are one byte each, and any load from them is a report)
    char* one_slot = (char*)malloc(1); uint8_t* seq4 = (uint8_t*)malloc(1); uint64_t* seq_off = (uint64_t*)malloc(1); int32_t* l_qseq = (int32_t*)malloc(1);
    if (d.n_slots) { d.slots = one_slot; d.seq4 = seq4; d.seq_off = seq_off; d.l_qseq = l_qseq; }
    d.ref = has_ref ? ref : nullptr;
    brc_runs* h = nullptr;
    if (brc_runs_create(0, &h) != BRC_OK) return 2;
    for (int w = 0; w < n_calls; ++w) {
        int64_t k0, n, cap; uint32_t head[4], cut[BRC_RUNS_MAX_CUT]; int32_t has_role, want, with_indels;
        if (fread(&k0, 8, 1, in) != 1 || fread(&n, 8, 1, in) != 1 || fread(&cap, 8, 1, in) != 1 || fread(head, 4, 4, in) != 4 ||
            fread(cut, 4, BRC_RUNS_MAX_CUT, in) != BRC_RUNS_MAX_CUT || fread(&has_role, 4, 1, in) != 1 || fread(&want, 4, 1, in) != 1 ||
            fread(&with_indels, 4, 1, in) != 1 || cap < 0 || head[1] < 1 || head[1] > BRC_RUNS_MAX_CUT) return 2;
        uint8_t* role = slurp<uint8_t>(in, has_role ? L : 0);
        // (the cuts behind n_cut are 0: a loop that read past n_cut would refuse them as not ascending, or count them)
        brc_runs_params p; memset(&p, 0, sizeof p);
        p.role = has_role ? role : nullptr; p.combine = head[0]; p.n_cut = head[1]; p.keep = head[2]; p.flags = head[3];
        for (uint32_t i = 0; i < BRC_RUNS_MAX_CUT; ++i) p.cut[i] = i < p.n_cut ? cut[i] : 0u;
        const int64_t wsb = brc_runs_workspace(n);
        void* ws = filled((size_t)wsb);
        const size_t nc = (size_t)p.n_cut + 2;
        int32_t* start = (int32_t*)filled((size_t)cap * 4); int32_t* end = (int32_t*)filled((size_t)cap * 4); uint32_t* cls = (uint32_t*)filled((size_t)cap * 4);
        uint32_t* counts = (uint32_t*)filled(4); uint64_t* per = (uint64_t*)filled(nc * 8);
        const int32_t rc = brc_runs_find(h, &v, with_indels ? &d : nullptr, &p, k0, n, cap, (want & 1) ? start : nullptr, (want & 2) ? end : nullptr,
                                         (want & 4) ? cls : nullptr, (want & 8) ? counts : nullptr, (want & 16) ? per : nullptr, wsb ? ws : nullptr, nullptr);
        fwrite(&rc, 4, 1, out); fwrite(counts, 4, 1, out); fwrite(start, 4, (size_t)cap, out); fwrite(end, 4, (size_t)cap, out); fwrite(cls, 4, (size_t)cap, out);
        fwrite(per, 8, nc, out);
        free(ws); free(start); free(end); free(cls); free(counts); free(per); free(role);
    }
    brc_runs_destroy(h);
    free(ncol); free(depth); free(slotid); free(si); free(sf); free(unavail); free(xagg); free(slots); free(ref); free(one_slot); free(seq4); free(seq_off); free(l_qseq);
    fclose(in); fclose(out);
    printf("%d calls\n", n_calls);
    return 0;
}
