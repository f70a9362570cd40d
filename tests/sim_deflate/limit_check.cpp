// Driver for the length limiter of brc_deflate_core.h (make limit_check): symbol counts in, code lengths out, through the same two
// steps the kernel takes — the used symbols ranked by (count, symbol), then limited_lengths() on one lane.
//   usage: limit_check maxbits count0 count1 ...      prints one code length per symbol
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../bam_readcount_amd/csrc/brc_deflate_core.h"

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: limit_check maxbits counts...\n"); return 2; }
    const int maxbits = atoi(argv[1]), ns = argc - 2;
    if (maxbits < 1 || maxbits > 15 || ns > 320) return 2;
    std::vector<uint32_t> hist((size_t)ns), A((size_t)ns), num(16);
    std::vector<uint16_t> sorted((size_t)ns); std::vector<uint8_t> lens((size_t)ns, 0);
    for (int i = 0; i < ns; ++i) hist[(size_t)i] = (uint32_t)strtoul(argv[i + 2], nullptr, 10);
    int nused = 0;
    for (int i = 0; i < ns; ++i) {
        const uint32_t f = hist[(size_t)i];
        if (!f) continue;
        uint32_t rank = 0;
        for (int j = 0; j < ns; ++j) { const uint32_t g = hist[(size_t)j]; rank += (g && (g < f || (g == f && j < i))) ? 1u : 0u; }
        sorted[rank] = (uint16_t)i; A[rank] = f; ++nused;
    }
    brcdef::limited_lengths(A.data(), sorted.data(), num.data(), lens.data(), nused, maxbits);
    for (int i = 0; i < ns; ++i) printf("%d%c", lens[(size_t)i], i + 1 < ns ? ' ' : '\n');
    return 0;
}
