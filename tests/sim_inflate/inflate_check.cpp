// Driver of the sanitizer build (make asan): runs brc_inflate_bgzf of the CPU inflater over a file of cases and writes what came back.
//   in : repeated { u32 len, len bytes }             one src chain per case
//   out: repeated { i32 rc, u32 n, n status bytes, u64 out_bytes, out_bytes bytes }
// src and dst are heap blocks of exactly the sizes the call is told, dst pre-filled with 0xA5 (a failed member must leave it so).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/brc_inflate.h"

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: inflate_check_asan cases.bin results.bin\n"); return 2; }
    FILE* in = fopen(argv[1], "rb"); FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open files\n"); return 2; }
    brc_inflater* h = nullptr;
    if (brc_inflater_create(0, &h) != BRC_OK) return 2;
    uint32_t len; size_t cases = 0;
    while (fread(&len, 4, 1, in) == 1) {
        uint8_t* src = (uint8_t*)malloc(len ? len : 1);
        if (len && fread(src, 1, len, in) != len) { fprintf(stderr, "short case file\n"); return 2; }
        const size_t cap = len / 26 + 1;
        std::vector<uint64_t> off(cap + 1); std::vector<uint8_t> st(cap);
        size_t n = cap;
        (void)brc_inflate_bgzf(h, src, len, nullptr, 0, off.data(), st.data(), &n);          // sizes first
        const uint64_t total = n <= cap ? off[n] : 0;
        uint8_t* dst = (uint8_t*)malloc(total ? total : 1);
        memset(dst, 0xA5, total ? total : 1);
        n = cap;
        const int32_t rc = brc_inflate_bgzf(h, src, len, dst, total, off.data(), st.data(), &n);
        const uint32_t n32 = (uint32_t)n;
        fwrite(&rc, 4, 1, out); fwrite(&n32, 4, 1, out); fwrite(st.data(), 1, n <= cap ? n : 0, out); fwrite(&total, 8, 1, out); fwrite(dst, 1, total, out);
        free(dst); free(src); ++cases;
    }
    brc_inflater_destroy(h);
    fclose(in); fclose(out);
    printf("%zu cases\n", cases);
    return 0;
}
