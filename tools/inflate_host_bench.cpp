// The host side of tools/inflate_bench.py: the members of a BGZF file inflated by brcio::Bgzf as the command line's fetch threads
// do it (bamio.cpp: libdeflate when the system has it, zlib otherwise; one block at a time, CRC checked), on T threads, each with a
// handle of its own over a contiguous share of the members.  Prints: threads, members, bytes out, repetitions, seconds.
#include <stdio.h>
#include <stdlib.h>

#include <chrono>
#include <thread>
#include <vector>

#include "../bam_readcount_amd/csrc/io/bamio.h"

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: inflate_host_bench file.bgzf threads min_seconds\n"); return 2; }
    const int T = atoi(argv[2]); const double min_s = atof(argv[3]);
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint64_t> offs; std::vector<uint32_t> isize; uint8_t h[18], t4[4]; uint64_t o = 0;
    while (fseeko(f, (off_t)o, SEEK_SET) == 0 && fread(h, 1, 18, f) == 18) {      // (BC is the first subfield of what the tool writes)
        const uint64_t next = o + (uint64_t)(h[16] | h[17] << 8) + 1;
        if (fseeko(f, (off_t)(next - 4), SEEK_SET) != 0 || fread(t4, 1, 4, f) != 4) break;
        offs.push_back(o); isize.push_back((uint32_t)t4[0] | (uint32_t)t4[1] << 8 | (uint32_t)t4[2] << 16 | (uint32_t)t4[3] << 24); o = next;
    }
    fclose(f);
    offs.push_back(o);
    const size_t n = offs.size() - 1;
    std::vector<brcio::Bgzf> hs((size_t)T);
    for (auto& b : hs) if (!b.open(argv[1])) return 2;
    std::vector<uint64_t> got((size_t)T);
    auto pass = [&]() {
        std::vector<std::thread> th;
        for (int t = 0; t < T; ++t) th.emplace_back([&, t]() {
            const size_t a = n * (size_t)t / (size_t)T, b = n * (size_t)(t + 1) / (size_t)T;
            std::vector<uint8_t> buf(1 << 16); uint64_t total = 0;
            if (a < b && hs[(size_t)t].seek(offs[a] << 16)) {
                for (size_t i = a; i < b; ++i) { if (isize[i] && !hs[(size_t)t].read(buf.data(), isize[i])) break; total += isize[i]; }      // exactly this share's blocks
            }
            got[(size_t)t] = total;
        });
        for (auto& x : th) x.join();
    };
    pass();                                                   // warm-up (page cache, libdeflate handles)
    const auto t0 = std::chrono::steady_clock::now(); int reps = 0; double s = 0;
    do { pass(); ++reps; s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); } while (s < min_s);
    uint64_t out = 0; for (uint64_t g : got) out += g;
    printf("%d %zu %llu %d %.6f\n", T, n, (unsigned long long)out, reps, s);
    return 0;
}
