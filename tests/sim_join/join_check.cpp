// Driver of the sanitizer build (make asan): runs brc_join_views of the CPU build over serialized sources and a list of calls.
//   in : i32 K, K x { i32 n_lib, pos0, i64 n_pos, stride, u64 n_xagg, i32 has_indels,
//                     u32 ncol[L*stride], depth[L*stride], slotid[L*stride], si[L*18*stride], sf[L*8*stride], u32 xagg[16*n_xagg],
//                     has_indels: u64 n_slots, i64 n_reads, u64 seq_bytes, i32 has_ref, i64 ref_lo, ref_hi, ref_len,
//                                 u32 slots[18*n_slots], u64 seq_off[n_reads], i32 l_qseq[n_reads], u8 seq4[seq_bytes], u8 ref[ref_hi - ref_lo] (has_ref) },
//        i32 n_calls, n_calls x { i32 pos0, i64 n_pos, stride, seq_cap (-1: what a first call for the counts alone says; -2: one byte less) }
//   out: per call { i32 rc, u32 status, u32 counts[2], i64 the seq_cap used, then — n_pos > 0 — ncol, depth, slotid, si, sf, xagg, slots,
//                   seq_off, l_qseq, seq4[seq_cap], ref }
// Sources are heap blocks of exactly their sizes, the scratch has exactly brc_join_workspace bytes, every destination exactly the bytes
// brc_join_sizes_of says, pre-filled with 0xA5 bytes: a load outside a source, or a store outside the scratch or a destination, is a
// report.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/brc_join.h"

template <class T> static T* slurp(FILE* in, size_t n) {
    T* p = (T*)malloc(n ? n * sizeof(T) : 1);
    if (n && fread(p, sizeof(T), n, in) != n) { fprintf(stderr, "short case file\n"); exit(2); }
    return p;
}
template <class T> static T one(FILE* in) { T x; if (fread(&x, sizeof(T), 1, in) != 1) { fprintf(stderr, "short case file\n"); exit(2); } return x; }
static void* filled(size_t bytes) { void* p = malloc(bytes ? bytes : 1); memset(p, 0xA5, bytes ? bytes : 1); return p; }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: join_check_asan case.bin results.bin\n"); return 2; }
    FILE* in = fopen(argv[1], "rb"); FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open files\n"); return 2; }
    const int32_t K = one<int32_t>(in);
    if (K < 1 || K > BRC_JOIN_MAX_SOURCES) return 2;
    std::vector<brc_device_view> V((size_t)K); std::vector<brc_device_indels> D((size_t)K); std::vector<brc_join_source> S((size_t)K);
    std::vector<void*> heap;
    for (int s = 0; s < K; ++s) {
        brc_device_view& v = V[(size_t)s]; brc_device_indels& d = D[(size_t)s];
        memset(&v, 0, sizeof v); memset(&d, 0, sizeof d);
        v.memory = d.memory = BRC_MEM_HOST;
        v.n_lib = one<int32_t>(in); v.pos0 = one<int32_t>(in); v.n_pos = one<int64_t>(in); v.stride = one<int64_t>(in); v.n_xagg = one<uint64_t>(in);
        const int32_t has_indels = one<int32_t>(in);
        if (v.n_lib < 1 || v.n_pos < 0 || v.stride < v.n_pos) return 2;
        const size_t row = (size_t)v.stride, L = (size_t)v.n_lib;
        uint32_t* ncol = slurp<uint32_t>(in, L * row); uint32_t* depth = slurp<uint32_t>(in, L * row); uint32_t* slotid = slurp<uint32_t>(in, L * row);
        uint32_t* si = slurp<uint32_t>(in, L * 18 * row); uint32_t* sf = slurp<uint32_t>(in, L * 8 * row); uint32_t* xagg = slurp<uint32_t>(in, 16 * (size_t)v.n_xagg);
        v.ncol = ncol; v.depth = depth; v.slotid = slotid; v.si = si; v.sf = (const float*)sf; v.xagg = v.n_xagg ? xagg : nullptr;
        heap.insert(heap.end(), {ncol, depth, slotid, si, sf, xagg});
        S[(size_t)s].view = &v; S[(size_t)s].indels = nullptr;
        if (has_indels) {
            d.n_lib = v.n_lib; d.pos0 = v.pos0; d.n_pos = v.n_pos;
            d.n_slots = one<uint64_t>(in); d.n_reads = one<int64_t>(in);
            const uint64_t seq_bytes = one<uint64_t>(in); const int32_t has_ref = one<int32_t>(in);
            d.ref_lo = one<int64_t>(in); d.ref_hi = one<int64_t>(in); d.ref_len = one<int64_t>(in);
            if (d.n_reads < 0 || d.ref_hi < d.ref_lo) return 2;
            uint32_t* slots = slurp<uint32_t>(in, 18 * (size_t)d.n_slots); uint64_t* seq_off = slurp<uint64_t>(in, (size_t)d.n_reads);
            int32_t* l_qseq = slurp<int32_t>(in, (size_t)d.n_reads); uint8_t* seq4 = slurp<uint8_t>(in, (size_t)seq_bytes);
            char* ref = slurp<char>(in, has_ref ? (size_t)(d.ref_hi - d.ref_lo) : 0);
            d.slots = d.n_slots ? slots : nullptr; d.seq_off = seq_off; d.l_qseq = l_qseq; d.seq4 = seq4; d.ref = has_ref ? ref : nullptr;
            heap.insert(heap.end(), {slots, seq_off, l_qseq, seq4, ref});
            S[(size_t)s].indels = &d;
        }
    }
    const int32_t n_calls = one<int32_t>(in);
    brc_join* h = nullptr;
    if (brc_join_create(0, &h) != BRC_OK) return 2;
    for (int w = 0; w < n_calls; ++w) {
        const int32_t pos0 = one<int32_t>(in); const int64_t n = one<int64_t>(in), stride = one<int64_t>(in); int64_t seq_cap = one<int64_t>(in);
        brc_join_sizes z;
        int32_t rc = brc_join_sizes_of(K, S.data(), pos0, n, stride, &z);
        uint32_t* counts = (uint32_t*)filled(8); uint32_t* status = (uint32_t*)filled(4);
        void* ws = filled((size_t)z.workspace_bytes);
        if (rc == BRC_OK && seq_cap < 0) {
            rc = brc_join_views(h, K, S.data(), pos0, n, stride, nullptr, nullptr, nullptr, counts, 0, nullptr, ws, (size_t)z.workspace_bytes, nullptr);
            seq_cap = (int64_t)counts[1] + (seq_cap == -2 ? -1 : 0);
            if (seq_cap < 0) seq_cap = 0;
            memset(counts, 0xA5, 8);
        }
        brc_join_dest d; memset(&d, 0, sizeof d);
        d.ncol = (uint32_t*)filled((size_t)z.ncol_bytes); d.depth = (uint32_t*)filled((size_t)z.depth_bytes); d.slotid = (uint32_t*)filled((size_t)z.slotid_bytes);
        d.si = (uint32_t*)filled((size_t)z.si_bytes); d.sf = (float*)filled((size_t)z.sf_bytes); d.xagg = filled((size_t)z.xagg_bytes);
        d.slots = filled((size_t)z.slots_bytes); d.seq_off = (uint64_t*)filled((size_t)z.seq_off_bytes); d.l_qseq = (int32_t*)filled((size_t)z.l_qseq_bytes);
        d.seq4 = (uint8_t*)filled((size_t)seq_cap); d.ref = (char*)filled((size_t)z.ref_bytes);
        brc_device_view ov; brc_device_indels oi;
        if (rc == BRC_OK) rc = brc_join_views(h, K, S.data(), pos0, n, stride, &d, &ov, &oi, counts, seq_cap, status, ws, (size_t)z.workspace_bytes, nullptr);
        fwrite(&rc, 4, 1, out); fwrite(status, 4, 1, out); fwrite(counts, 4, 2, out); fwrite(&seq_cap, 8, 1, out);
        if (n > 0) {
            fwrite(d.ncol, 1, (size_t)z.ncol_bytes, out); fwrite(d.depth, 1, (size_t)z.depth_bytes, out); fwrite(d.slotid, 1, (size_t)z.slotid_bytes, out);
            fwrite(d.si, 1, (size_t)z.si_bytes, out); fwrite(d.sf, 1, (size_t)z.sf_bytes, out); fwrite(d.xagg, 1, (size_t)z.xagg_bytes, out);
            fwrite(d.slots, 1, (size_t)z.slots_bytes, out); fwrite(d.seq_off, 1, (size_t)z.seq_off_bytes, out); fwrite(d.l_qseq, 1, (size_t)z.l_qseq_bytes, out);
            fwrite(d.seq4, 1, (size_t)seq_cap, out); fwrite(d.ref, 1, (size_t)z.ref_bytes, out);
        }
        free(d.ncol); free(d.depth); free(d.slotid); free(d.si); free(d.sf); free(d.xagg); free(d.slots); free(d.seq_off); free(d.l_qseq); free(d.seq4); free(d.ref);
        free(ws); free(counts); free(status);
    }
    brc_join_destroy(h);
    for (void* p : heap) free(p);
    fclose(in); fclose(out);
    printf("%d calls\n", n_calls);
    return 0;
}
