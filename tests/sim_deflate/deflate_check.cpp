// Driver of the sanitizer build (make asan): runs brc_deflate_bgzf of the CPU deflater over a file of inputs and writes what came back.
//   in : repeated { u32 len, len bytes }
//   out: repeated { i32 rc, u64 n_members, u64 out_bytes, out_bytes bytes }
// src and dst are heap blocks of exactly the sizes the call is told (dst: brc_deflate_bound).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/brc_deflate.h"

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: deflate_check_asan cases.bin results.bin\n"); return 2; }
    FILE* in = fopen(argv[1], "rb"); FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open files\n"); return 2; }
    brc_deflater* h = nullptr;
    if (brc_deflater_create(0, &h) != BRC_OK) return 2;
    uint32_t len; size_t cases = 0;
    while (fread(&len, 4, 1, in) == 1) {
        uint8_t* src = (uint8_t*)malloc(len ? len : 1);
        if (len && fread(src, 1, len, in) != len) { fprintf(stderr, "short case file\n"); return 2; }
        const size_t cap = brc_deflate_bound(len);
        uint8_t* dst = (uint8_t*)malloc(cap ? cap : 1);
        size_t got = 0, nm = 0;
        const int32_t rc = brc_deflate_bgzf(h, src, len, dst, cap, &got, &nm);
        const uint64_t n64 = nm, g64 = got;
        fwrite(&rc, 4, 1, out); fwrite(&n64, 8, 1, out); fwrite(&g64, 8, 1, out); fwrite(dst, 1, got, out);
        free(dst); free(src); ++cases;
    }
    brc_deflater_destroy(h);
    fclose(in); fclose(out);
    printf("%zu cases\n", cases);
    return 0;
}
