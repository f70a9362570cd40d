// Driver of the sanitizer build (make asan): runs brc_inorm_table of the CPU build over one serialized view and a list of calls.
//   in : i32 n_lib, i32 pos0, i64 n_pos, i32 has_ref, i64 ref_lo, ref_hi, ref_len, i64 ref_bytes, the slice, i32 n_calls,
//        n_calls x { i64 k0, n, m, alleles_len, cap, alleles_cap, u32 max_shift, i32 has_rep, i32 want (1 counts | 2 npos, shift, flags, group |
//                    4 the merged table | 8 status),
//                    i32 pos[m], lib[m], len[m], u32 rep_read[m] and i32 rep_qpos[m] (has_rep), u32 istat[9*m], f32 fstat[4*m],
//                    u32 allele_off[m+1], u8 alleles[alleles_len] }
//   out: per call { i32 rc, u32 status, u32 counts[2], i32 npos[m], u32 shift[m], flags[m], i32 group[m], i32 pos[cap], lib[cap], len[cap],
//                   u32 rep_read[cap], i32 rep_qpos[cap], u32 members[cap], istat[9*cap], f32 fstat[4*cap], metrics[13*cap], u32 allele_off[cap+1],
//                   u8 alleles[alleles_cap] } — a destination that was not wanted comes back as it was filled
// Sources are heap blocks of exactly the table's sizes (stride == m, alleles of exactly alleles_len bytes, the reference slice of exactly
// its bytes), the scratch has exactly brc_inorm_workspace bytes, every destination exactly the contract's elements, pre-filled with 0xA5
// bytes: a load outside the reference or the table, or a store outside the scratch or a destination, is a report.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/brc_inorm.h"

template <class T> static T* slurp(FILE* in, size_t n) {
    T* p = (T*)malloc(n ? n * sizeof(T) : 1);
    if (n && fread(p, sizeof(T), n, in) != n) { fprintf(stderr, "short case file\n"); exit(2); }
    return p;
}
static void* filled(size_t bytes) { void* p = malloc(bytes ? bytes : 1); memset(p, 0xA5, bytes ? bytes : 1); return p; }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: inorm_check_asan case.bin results.bin\n"); return 2; }
    FILE* in = fopen(argv[1], "rb"); FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open files\n"); return 2; }
    brc_device_indels d; memset(&d, 0, sizeof d);
    d.memory = BRC_MEM_HOST;
    int32_t has_ref, n_calls; int64_t ref_bytes;
    if (fread(&d.n_lib, 4, 1, in) != 1 || fread(&d.pos0, 4, 1, in) != 1 || fread(&d.n_pos, 8, 1, in) != 1 || fread(&has_ref, 4, 1, in) != 1 ||
        fread(&d.ref_lo, 8, 1, in) != 1 || fread(&d.ref_hi, 8, 1, in) != 1 || fread(&d.ref_len, 8, 1, in) != 1 || fread(&ref_bytes, 8, 1, in) != 1 || ref_bytes < 0) return 2;
    char* ref = slurp<char>(in, (size_t)ref_bytes);
    d.ref = has_ref ? ref : nullptr;
    if (fread(&n_calls, 4, 1, in) != 1) return 2;
    brc_inorm* h = nullptr;
    if (brc_inorm_create(0, &h) != BRC_OK) return 2;
    for (int w = 0; w < n_calls; ++w) {
        int64_t k0, n, m, A, cap, acap; int32_t has_rep, want; brc_inorm_params p; memset(&p, 0, sizeof p);
        if (fread(&k0, 8, 1, in) != 1 || fread(&n, 8, 1, in) != 1 || fread(&m, 8, 1, in) != 1 || fread(&A, 8, 1, in) != 1 || fread(&cap, 8, 1, in) != 1 ||
            fread(&acap, 8, 1, in) != 1 || fread(&p.max_shift, 4, 1, in) != 1 || fread(&has_rep, 4, 1, in) != 1 || fread(&want, 4, 1, in) != 1 || m < 0 || A < 0 ||
            cap < 0 || acap < 0) return 2;
        const size_t M = (size_t)m, K = (size_t)cap;
        brc_inorm_source t; memset(&t, 0, sizeof t);
        int32_t* pos = slurp<int32_t>(in, M); int32_t* lib = slurp<int32_t>(in, M); int32_t* len = slurp<int32_t>(in, M);
        uint32_t* rr = slurp<uint32_t>(in, has_rep ? M : 0); int32_t* rq = slurp<int32_t>(in, has_rep ? M : 0);
        uint32_t* istat = slurp<uint32_t>(in, BRC_NI * M); float* fstat = slurp<float>(in, BRC_NF * M);
        uint32_t* off = slurp<uint32_t>(in, M + 1); uint8_t* text = slurp<uint8_t>(in, (size_t)A);
        t.m = m; t.stride = m; t.pos = pos; t.lib = lib; t.len = len; t.rep_read = has_rep ? rr : nullptr; t.rep_qpos = has_rep ? rq : nullptr;
        t.istat = istat; t.fstat = fstat; t.allele_off = off; t.alleles = text; t.alleles_len = A;
        const size_t wsb = brc_inorm_workspace(n, m);
        void* ws = filled(wsb);
        uint32_t* counts = (uint32_t*)filled(8); uint32_t* status = (uint32_t*)filled(4);
        int32_t* npos = (int32_t*)filled(M * 4); uint32_t* shift = (uint32_t*)filled(M * 4); uint32_t* flags = (uint32_t*)filled(M * 4); int32_t* group = (int32_t*)filled(M * 4);
        int32_t* opos = (int32_t*)filled(K * 4); int32_t* olib = (int32_t*)filled(K * 4); int32_t* olen = (int32_t*)filled(K * 4);
        uint32_t* orr = (uint32_t*)filled(K * 4); int32_t* orq = (int32_t*)filled(K * 4); uint32_t* omem = (uint32_t*)filled(K * 4);
        uint32_t* oi = (uint32_t*)filled(BRC_NI * K * 4); float* of = (float*)filled(BRC_NF * K * 4); float* om = (float*)filled(BRC_NMETRIC * K * 4);
        uint32_t* ooff = (uint32_t*)filled((K + 1) * 4); uint8_t* otext = (uint8_t*)filled((size_t)acap);
        const bool src = want & 2, tab = want & 4;
        const int32_t rc = brc_inorm_table(h, &d, &p, &t, k0, n, ws, wsb, (want & 1) ? counts : nullptr, src ? npos : nullptr, src ? shift : nullptr,
                                           src ? flags : nullptr, src ? group : nullptr, cap, acap, tab ? opos : nullptr, tab ? olib : nullptr, tab ? olen : nullptr,
                                           tab ? orr : nullptr, tab ? orq : nullptr, tab ? omem : nullptr, tab ? oi : nullptr, tab ? of : nullptr, tab ? om : nullptr,
                                           tab ? ooff : nullptr, tab ? otext : nullptr, (want & 8) ? status : nullptr, nullptr);
        fwrite(&rc, 4, 1, out); fwrite(status, 4, 1, out); fwrite(counts, 4, 2, out);
        fwrite(npos, 4, M, out); fwrite(shift, 4, M, out); fwrite(flags, 4, M, out); fwrite(group, 4, M, out);
        fwrite(opos, 4, K, out); fwrite(olib, 4, K, out); fwrite(olen, 4, K, out); fwrite(orr, 4, K, out); fwrite(orq, 4, K, out); fwrite(omem, 4, K, out);
        fwrite(oi, 4, BRC_NI * K, out); fwrite(of, 4, BRC_NF * K, out); fwrite(om, 4, BRC_NMETRIC * K, out); fwrite(ooff, 4, K + 1, out);
        fwrite(otext, 1, (size_t)acap, out);
        free(ws); free(counts); free(status); free(npos); free(shift); free(flags); free(group); free(opos); free(olib); free(olen); free(orr); free(orq);
        free(omem); free(oi); free(of); free(om); free(ooff); free(otext);
        free(pos); free(lib); free(len); free(rr); free(rq); free(istat); free(fstat); free(off); free(text);
    }
    brc_inorm_destroy(h);
    free(ref);
    fclose(in); fclose(out);
    printf("%d calls\n", n_calls);
    return 0;
}
