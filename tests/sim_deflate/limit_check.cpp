// Driver for the length limiter of brc_deflate_core.h (make limit_check): symbol counts in, code lengths out, through the same two
// steps the kernel takes — the used symbols ranked by (count, symbol), then limited_lengths() on one lane.
//   usage: limit_check maxbits count0 count1 ...      prints one code length per symbol
//          limit_check -                              the same for every line "maxbits count0 count1 ..." of the standard input
#include <stdio.h>
#include <stdlib.h>

#include <sstream>
#include <string>
#include <vector>

#include "../../bam_readcount_amd/csrc/brc_deflate_core.h"

static int one(int maxbits, const std::vector<uint32_t>& hist) {
    const int ns = (int)hist.size();
    if (maxbits < 1 || maxbits > 15 || ns < 1 || ns > 320) return 2;
    std::vector<uint32_t> A((size_t)ns), num(16);
    std::vector<uint16_t> sorted((size_t)ns); std::vector<uint8_t> lens((size_t)ns, 0);
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

int main(int argc, char** argv) {
    if (argc == 2 && std::string(argv[1]) == "-") {
        char* line = nullptr; size_t cap = 0;
        while (getline(&line, &cap, stdin) > 0) {
            std::istringstream in(line);
            int maxbits; unsigned long v; std::vector<uint32_t> hist;
            if (!(in >> maxbits)) continue;
            while (in >> v) hist.push_back((uint32_t)v);
            if (const int rc = one(maxbits, hist)) { free(line); return rc; }
        }
        free(line);
        return 0;
    }
    if (argc < 3) { fprintf(stderr, "usage: limit_check maxbits counts... | limit_check -\n"); return 2; }
    std::vector<uint32_t> hist;
    for (int i = 2; i < argc; ++i) hist.push_back((uint32_t)strtoul(argv[i], nullptr, 10));
    return one(atoi(argv[1]), hist);
}
