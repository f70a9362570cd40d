// Driver of the sanitizer build (make asan): runs brc_ivet_records of the CPU build over one serialized pair of views and a list of calls.
//   in : the two views as tests/sim_vet/vet_check.cpp reads them —
//        i32 Lp, i32 pos0, i64 P, i64 PS, u64 n_xagg, i32 has_unavail, i32 n_calls,
//        u32 ncol[Lp*PS], depth[Lp*PS], slotid[Lp*PS], si[Lp*2*9*PS], f32 sf[Lp*2*4*PS], u32 unavail[PS] (has_unavail), n_xagg records of 64 bytes,
//        u64 n_slots, n_slots records of 72 bytes, i32 has_ref, i64 ref_lo, ref_hi, ref_len, i64 ref_bytes, the slice —
//        n_calls x { i64 m, i64 n, i64 alleles_len, i32 has_why, i32 has_role, i32 has_text, i32 want (1 fail | 2 vals | 4 ctl_count | 8 keep | 16 status),
//                    u32 tests, kinds, u32 x 12 and f32 x 13: the thresholds in brc_ivet_params' order,
//                    i32 pos[m], lib[m], len[m], u32 istat[9*m], f32 fstat[4*m], u32 allele_off[m+1] and u8 alleles[alleles_len] (has_text),
//                    i32 idx[n], u32 why[n] (has_why), u8 role[Lp] (has_role) }
//   out: per call { i32 rc, u32 status, u32 fail[m], vals[20*m], ctl_count[m], keep[n] } — a destination that was not wanted comes back as it was filled
// Sources are heap blocks of exactly the views' and the table's sizes (stride == m, alleles of exactly alleles_len bytes); idx and why
// have exactly n elements, role exactly Lp bytes, the scratch exactly brc_ivet_workspace bytes, every destination exactly [planes][m] or
// [n] elements (dst_stride == m) — the least the contract allows — pre-filled with 0xA5 bytes: a load outside the views, the table or the
// lists, or a store outside the scratch or a destination, is a report.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/brc_ivet.h"

template <class T> static T* slurp(FILE* in, size_t n) {
    T* p = (T*)malloc(n ? n * sizeof(T) : 1);
    if (n && fread(p, sizeof(T), n, in) != n) { fprintf(stderr, "short case file\n"); exit(2); }
    return p;
}
static void* filled(size_t bytes) { void* p = malloc(bytes ? bytes : 1); memset(p, 0xA5, bytes ? bytes : 1); return p; }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: ivet_check_asan case.bin results.bin\n"); return 2; }
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
    // (the filter reads no engine-side indel record: those arrays are one byte each, and any load from them is a report)
    uint8_t* seq4 = (uint8_t*)malloc(1); uint64_t* seq_off = (uint64_t*)malloc(1); int32_t* l_qseq = (int32_t*)malloc(1);
    if (d.n_slots) { d.slots = slots; d.seq4 = seq4; d.seq_off = seq_off; d.l_qseq = l_qseq; }
    d.ref = has_ref ? ref : nullptr;
    brc_ivet* h = nullptr;
    if (brc_ivet_create(0, &h) != BRC_OK) return 2;
    for (int w = 0; w < n_calls; ++w) {
        int64_t m, n, A; int32_t has_why, has_role, has_text, want; brc_ivet_params p; memset(&p, 0, sizeof p);
        if (fread(&m, 8, 1, in) != 1 || fread(&n, 8, 1, in) != 1 || fread(&A, 8, 1, in) != 1 || fread(&has_why, 4, 1, in) != 1 || fread(&has_role, 4, 1, in) != 1 ||
            fread(&has_text, 4, 1, in) != 1 || fread(&want, 4, 1, in) != 1 || fread(&p.tests, 4, 1, in) != 1 || fread(&p.kinds, 4, 1, in) != 1 ||
            fread(&p.min_depth, 4, 12, in) != 12 || fread(&p.min_var_readpos, 4, 13, in) != 13 || m < 0 || n < 0 || A < 0) return 2;
        const size_t M = (size_t)m, N = (size_t)n;
        brc_ivet_table t; memset(&t, 0, sizeof t);
        int32_t* pos = slurp<int32_t>(in, M); int32_t* lib = slurp<int32_t>(in, M); int32_t* len = slurp<int32_t>(in, M);
        uint32_t* istat = slurp<uint32_t>(in, BRC_NI * M); float* fstat = slurp<float>(in, BRC_NF * M);
        uint32_t* off = slurp<uint32_t>(in, has_text ? M + 1 : 0); uint8_t* text = slurp<uint8_t>(in, has_text ? (size_t)A : 0);
        t.m = m; t.stride = m; t.pos = pos; t.lib = lib; t.len = len; t.istat = istat; t.fstat = fstat;
        t.allele_off = has_text ? off : nullptr; t.alleles = has_text ? text : nullptr; t.alleles_len = A;
        int32_t* idx = slurp<int32_t>(in, N);
        uint32_t* why = slurp<uint32_t>(in, has_why ? N : 0);
        uint8_t* role = slurp<uint8_t>(in, has_role ? L : 0);
        p.role = has_role ? role : nullptr;
        const int64_t wsb = brc_ivet_workspace(&v, m);
        void* ws = filled((size_t)wsb);
        uint32_t* fail = (uint32_t*)filled(M * 4); float* vals = (float*)filled(BRC_IVET_NVAL * M * 4); uint32_t* ctl = (uint32_t*)filled(M * 4);
        uint32_t* keep = (uint32_t*)filled(N * 4); uint32_t* status = (uint32_t*)filled(4);
        const int32_t rc = brc_ivet_records(h, &v, &d, &p, &t, n ? idx : nullptr, has_why ? why : nullptr, n, m, (want & 1) ? fail : nullptr, (want & 2) ? vals : nullptr,
                                            (want & 4) ? ctl : nullptr, (want & 8) ? keep : nullptr, (want & 16) ? status : nullptr, ws, nullptr);
        fwrite(&rc, 4, 1, out); fwrite(status, 4, 1, out);
        fwrite(fail, 4, M, out); fwrite(vals, 4, BRC_IVET_NVAL * M, out); fwrite(ctl, 4, M, out); fwrite(keep, 4, N, out);
        free(ws); free(fail); free(vals); free(ctl); free(keep); free(status); free(idx); free(why); free(role);
        free(pos); free(lib); free(len); free(istat); free(fstat); free(off); free(text);
    }
    brc_ivet_destroy(h);
    free(ncol); free(depth); free(slotid); free(si); free(sf); free(unavail); free(xagg); free(slots); free(ref); free(seq4); free(seq_off); free(l_qseq);
    fclose(in); fclose(out);
    printf("%d calls\n", n_calls);
    return 0;
}
