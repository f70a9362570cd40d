// Sanitizer driver of the CPU build (tests/sim_indels/Makefile: asan): reads a host view and a list of calls from a file, runs every
// call with a scratch and destinations of EXACTLY the contract's sizes on the heap, writes what came back.
//   in :  i32 n_lib, pos0; i64 n_pos; u64 n_slots; i64 n_reads; u64 seq_bytes; i64 ref_lo, ref_hi, ref_len; i32 has_ref, n_calls;
//         slots [n_slots * 72]; seq_off u64 [n_reads]; l_qseq i32 [n_reads]; seq4 [seq_bytes]; ref [ref_hi - ref_lo];
//         then per call i64 k0, n, cap, alleles_cap
//   out:  per call i32 rc, u32 counts[2], then pos lib len rep_read rep_qpos [cap], istat [9 * cap], fstat [4 * cap], metrics [13 * cap],
//         allele_off [cap + 1], alleles [alleles_cap] (destinations are pre-filled with 0xA5 bytes)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/brc_indels.h"

template <class T> static std::vector<T> rd(FILE* f, size_t n) { std::vector<T> v(n); if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } return v; }
template <class T> static T rd1(FILE* f) { return rd<T>(f, 1)[0]; }
template <class T> static T* fresh(size_t n) { T* p = (T*)malloc(n ? n * sizeof(T) : 1); memset(p, 0xA5, n * sizeof(T)); return p; }
template <class T> static void wr(FILE* f, T* p, size_t n) { if (n) fwrite(p, sizeof(T), n, f); free(p); }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
    brc_device_indels v; memset(&v, 0, sizeof v);
    v.memory = BRC_MEM_HOST;
    v.n_lib = rd1<int32_t>(f); v.pos0 = rd1<int32_t>(f); v.n_pos = rd1<int64_t>(f); v.n_slots = rd1<uint64_t>(f); v.n_reads = rd1<int64_t>(f);
    const uint64_t seq_bytes = rd1<uint64_t>(f);
    v.ref_lo = rd1<int64_t>(f); v.ref_hi = rd1<int64_t>(f); v.ref_len = rd1<int64_t>(f);
    const int32_t has_ref = rd1<int32_t>(f), n_calls = rd1<int32_t>(f);
    std::vector<uint8_t> slots = rd<uint8_t>(f, (size_t)v.n_slots * 72);
    std::vector<uint64_t> seq_off = rd<uint64_t>(f, (size_t)v.n_reads);
    std::vector<int32_t> l_qseq = rd<int32_t>(f, (size_t)v.n_reads);
    std::vector<uint8_t> seq4 = rd<uint8_t>(f, (size_t)seq_bytes);
    std::vector<char> ref = rd<char>(f, has_ref ? (size_t)(v.ref_hi - v.ref_lo) : 0);
    v.slots = v.n_slots ? slots.data() : nullptr; v.seq_off = seq_off.data(); v.l_qseq = l_qseq.data(); v.seq4 = seq4.data(); v.ref = has_ref ? ref.data() : nullptr;
    brc_indels* h = nullptr;
    if (brc_indels_create(0, &h)) return 3;
    FILE* o = fopen(argv[2], "wb"); if (!o) return 2;
    for (int c = 0; c < n_calls; ++c) {
        const int64_t k0 = rd1<int64_t>(f), n = rd1<int64_t>(f), cap = rd1<int64_t>(f), acap = rd1<int64_t>(f);
        const size_t wsb = brc_indels_workspace(&v, n), C = (size_t)cap;
        uint8_t* ws = fresh<uint8_t>(wsb);
        uint32_t* counts = fresh<uint32_t>(2);
        int32_t *pos = fresh<int32_t>(C), *lib = fresh<int32_t>(C), *len = fresh<int32_t>(C), *rq = fresh<int32_t>(C);
        uint32_t *rr = fresh<uint32_t>(C), *is = fresh<uint32_t>(9 * C), *ao = fresh<uint32_t>(C + 1);
        float *fs = fresh<float>(4 * C), *me = fresh<float>(13 * C);
        uint8_t* al = fresh<uint8_t>((size_t)acap);
        const int32_t rc = brc_indels_gather(h, &v, k0, n, wsb ? ws : nullptr, wsb, counts, cap, acap, pos, lib, len, rr, rq, is, fs, me, ao, al, nullptr);
        if (rc) fprintf(stderr, "call %d: %d (%s)\n", c, rc, brc_indels_last_error(h));
        fwrite(&rc, 4, 1, o);
        wr(o, counts, 2); wr(o, pos, C); wr(o, lib, C); wr(o, len, C); wr(o, rr, C); wr(o, rq, C); wr(o, is, 9 * C); wr(o, fs, 4 * C); wr(o, me, 13 * C);
        wr(o, ao, C + 1); wr(o, al, (size_t)acap);
        free(ws);
    }
    fclose(o); fclose(f);
    brc_indels_destroy(h);
    printf("%d calls\n", n_calls);
    return 0;
}
