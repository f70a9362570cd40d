// Driver of the sanitizer build (make asan): runs brc_cons_call of the CPU build over a serialized view, a table and a list of calls.
//   in : i32 n_lib, pos0, i64 n_pos, stride, u64 n_xagg, i64 ref_lo, ref_bytes, ref_len,
//        u32 ncol[L*stride], depth[L*stride], slotid[L*stride], si[L*18*stride], sf[L*8*stride], u32 xagg[16*n_xagg], u8 ref[ref_bytes],
//        i64 m, alleles_len, i32 pos[m], lib[m], len[m], u32 count[m], allele_off[m + 1], u8 alleles[alleles_len],
//        i32 n_calls, n_calls x { i64 k0, n, dst_stride, seq_cap, i32 has_lib_on, u32 flags, min_depth, min_count, num, den, ins_min_count,
//                                 ins_num, ins_den, fill, gap, u8 lib_on[L] }
//   out: per call { i32 rc, u32 status, u32 counts, u8 call[n], u32 cnt[5 * dst_stride + n] (n > 0), u32 ins_rec[n], u32 off[n + 1], u8 seq[seq_cap] }
// Sources are heap blocks of exactly their sizes, the scratch has exactly brc_cons_workspace bytes, every destination exactly the
// contract's size — the last plane of cnt ends behind its n-th element —, pre-filled with 0xA5 bytes: a load outside a source, or a
// store outside the scratch or a destination, is a report.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/brc_cons.h"

template <class T> static T* slurp(FILE* in, size_t n) {
    T* p = (T*)malloc(n ? n * sizeof(T) : 1);
    if (n && fread(p, sizeof(T), n, in) != n) { fprintf(stderr, "short case file\n"); exit(2); }
    return p;
}
template <class T> static T one(FILE* in) { T x; if (fread(&x, sizeof(T), 1, in) != 1) { fprintf(stderr, "short case file\n"); exit(2); } return x; }
static void* filled(size_t bytes) { void* p = malloc(bytes ? bytes : 1); memset(p, 0xA5, bytes ? bytes : 1); return p; }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: cons_check_asan case.bin results.bin\n"); return 2; }
    FILE* in = fopen(argv[1], "rb"); FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open files\n"); return 2; }
    brc_device_view v; brc_device_indels d;
    memset(&v, 0, sizeof v); memset(&d, 0, sizeof d);
    v.memory = d.memory = BRC_MEM_HOST;
    v.n_lib = d.n_lib = one<int32_t>(in); v.pos0 = d.pos0 = one<int32_t>(in); v.n_pos = d.n_pos = one<int64_t>(in); v.stride = one<int64_t>(in);
    v.n_xagg = one<uint64_t>(in);
    d.ref_lo = one<int64_t>(in); const int64_t ref_bytes = one<int64_t>(in); d.ref_len = one<int64_t>(in);
    if (v.n_lib < 1 || v.n_pos < 0 || v.stride < v.n_pos || ref_bytes < 0) return 2;
    d.ref_hi = d.ref_lo + ref_bytes;
    const size_t row = (size_t)v.stride, L = (size_t)v.n_lib;
    uint32_t* ncol = slurp<uint32_t>(in, L * row); uint32_t* depth = slurp<uint32_t>(in, L * row); uint32_t* slotid = slurp<uint32_t>(in, L * row);
    uint32_t* si = slurp<uint32_t>(in, L * 18 * row); uint32_t* sf = slurp<uint32_t>(in, L * 8 * row); uint32_t* xagg = slurp<uint32_t>(in, 16 * (size_t)v.n_xagg);
    char* ref = slurp<char>(in, (size_t)ref_bytes);
    v.ncol = ncol; v.depth = depth; v.slotid = slotid; v.si = si; v.sf = (const float*)sf; v.xagg = v.n_xagg ? xagg : nullptr;
    d.ref = ref_bytes ? ref : nullptr;
    brc_cons_table t; memset(&t, 0, sizeof t);
    t.m = t.stride = one<int64_t>(in); t.alleles_len = one<int64_t>(in);
    if (t.m < 0 || t.alleles_len < 0) return 2;
    int32_t* pos = slurp<int32_t>(in, (size_t)t.m); int32_t* lib = slurp<int32_t>(in, (size_t)t.m); int32_t* len = slurp<int32_t>(in, (size_t)t.m);
    uint32_t* count = slurp<uint32_t>(in, (size_t)t.m); uint32_t* aoff = slurp<uint32_t>(in, (size_t)t.m + 1); uint8_t* alleles = slurp<uint8_t>(in, (size_t)t.alleles_len);
    t.pos = pos; t.lib = lib; t.len = len; t.count = count; t.allele_off = aoff; t.alleles = alleles;
    const int32_t n_calls = one<int32_t>(in);
    brc_cons* h = nullptr;
    if (brc_cons_create(0, &h) != BRC_OK) return 2;
    for (int w = 0; w < n_calls; ++w) {
        const int64_t k0 = one<int64_t>(in), n = one<int64_t>(in), ds = one<int64_t>(in), seq_cap = one<int64_t>(in);
        const int32_t has_on = one<int32_t>(in);
        brc_cons_params p; memset(&p, 0, sizeof p);
        p.flags = one<uint32_t>(in); p.min_depth = one<uint32_t>(in); p.min_count = one<uint32_t>(in); p.num = one<uint32_t>(in); p.den = one<uint32_t>(in);
        p.ins_min_count = one<uint32_t>(in); p.ins_num = one<uint32_t>(in); p.ins_den = one<uint32_t>(in); p.fill = one<uint32_t>(in); p.gap = one<uint32_t>(in);
        uint8_t* on = slurp<uint8_t>(in, L);
        p.lib_on = has_on ? on : nullptr;
        if (n < 0 || ds < n || seq_cap < 0) return 2;
        const size_t N = (size_t)n, cnt_words = N ? 5 * (size_t)ds + N : 0;
        const int64_t wsb = brc_cons_workspace(&v, n, t.m);
        void* ws = filled((size_t)wsb);
        uint32_t* counts = (uint32_t*)filled(4); uint32_t* status = (uint32_t*)filled(4);
        uint8_t* call = (uint8_t*)filled(N); uint32_t* cnt = (uint32_t*)filled(4 * cnt_words); uint32_t* ins = (uint32_t*)filled(4 * N);
        uint32_t* off = (uint32_t*)filled(4 * (N + 1)); uint8_t* seq = (uint8_t*)filled((size_t)seq_cap);
        const int32_t rc = brc_cons_call(h, &v, &d, &p, &t, k0, n, ds, seq_cap, counts, call, cnt, ins, off, seq, status, ws, nullptr);
        fwrite(&rc, 4, 1, out); fwrite(status, 4, 1, out); fwrite(counts, 4, 1, out);
        fwrite(call, 1, N, out); fwrite(cnt, 4, cnt_words, out); fwrite(ins, 4, N, out); fwrite(off, 4, N + 1, out); fwrite(seq, 1, (size_t)seq_cap, out);
        free(ws); free(counts); free(status); free(call); free(cnt); free(ins); free(off); free(seq); free(on);
    }
    brc_cons_destroy(h);
    for (void* q : std::vector<void*>{ncol, depth, slotid, si, sf, xagg, ref, pos, lib, len, count, aoff, alleles}) free(q);
    fclose(in); fclose(out);
    printf("%d calls\n", n_calls);
    return 0;
}
