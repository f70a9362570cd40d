// The host yardstick of tools/deflate_bench.py: zlib on a pool of threads over the same 0xff00-byte pieces the deflater library cuts,
// each piece a BGZF member of its own.
//   deflate_host pipe THREADS [LEVEL]                 stdin -> BGZF members + the end-of-file member -> stdout (batches of 32 MB)
//   deflate_host bench FILE THREADS SECONDS [LEVEL]   the file's pieces over and over for at least SECONDS; prints: reps seconds output_bytes
// LEVEL 1..9: zlib; 101..112: libdeflate at level LEVEL - 100, when a libdeflate.so can be loaded (exit code 3 when not).
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <zlib.h>

#include <atomic>
#include <chrono>
#include <string>
#include <thread>
#include <vector>

static const size_t M = 0xff00, SLOT = 0xff00 + 64;
static const unsigned char kEof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

static void* (*ld_alloc)(int) = nullptr; static size_t (*ld_compress)(void*, const void*, size_t, void*, size_t) = nullptr; static void (*ld_free)(void*) = nullptr;
static void need_libdeflate() {
    void* l = dlopen("libdeflate.so.0", RTLD_NOW); if (!l) l = dlopen("libdeflate.so", RTLD_NOW);
    if (l) { ld_alloc = (void* (*)(int))dlsym(l, "libdeflate_alloc_compressor"); ld_compress = (size_t (*)(void*, const void*, size_t, void*, size_t))dlsym(l, "libdeflate_deflate_compress"); ld_free = (void (*)(void*))dlsym(l, "libdeflate_free_compressor"); }
    if (!ld_alloc || !ld_compress || !ld_free) { fprintf(stderr, "deflate_host: no libdeflate on this box\n"); exit(3); }
}

static size_t member(const unsigned char* src, size_t n, unsigned char* out, int level, void* ld) {
    static const unsigned char hd[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    size_t body;
    if (ld) { body = ld_compress(ld, src, n, out + 18, SLOT - 26); if (!body) { fprintf(stderr, "deflate_host: a piece did not fit its slot\n"); exit(2); } }
    else {
        z_stream z; memset(&z, 0, sizeof z);
        deflateInit2(&z, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY);
        z.next_in = (Bytef*)src; z.avail_in = (uInt)n; z.next_out = out + 18; z.avail_out = (uInt)(SLOT - 26);
        if (deflate(&z, Z_FINISH) != Z_STREAM_END) { fprintf(stderr, "deflate_host: a piece did not fit its slot\n"); exit(2); }
        body = z.total_out; deflateEnd(&z);
    }
    const size_t total = 18 + body + 8; const uint32_t crc = (uint32_t)crc32(0, src, (uInt)n), isz = (uint32_t)n;
    memcpy(out, hd, 16); out[16] = (unsigned char)(total - 1); out[17] = (unsigned char)((total - 1) >> 8);
    memcpy(out + 18 + body, &crc, 4); memcpy(out + 22 + body, &isz, 4);
    return total;
}

// the pieces of buf[0, n) -> slots, sizes; returns the bytes of all members
static size_t batch(const unsigned char* buf, size_t n, std::vector<unsigned char>& slots, std::vector<size_t>& sizes, int threads, int level) {
    const size_t np = (n + M - 1) / M;
    if (slots.size() < np * SLOT) slots.resize(np * SLOT);
    sizes.assign(np, 0);
    std::atomic<size_t> next(0);
    if (level > 100 && !ld_alloc) need_libdeflate();
    auto work = [&]() {
        void* ld = level > 100 ? ld_alloc(level - 100) : nullptr;
        for (;;) { const size_t i = next.fetch_add(1); if (i >= np) break; sizes[i] = member(buf + i * M, n - i * M < M ? n - i * M : M, slots.data() + i * SLOT, level, ld); }
        if (ld) ld_free(ld);
    };
    std::vector<std::thread> th;
    for (int k = 1; k < threads; ++k) th.emplace_back(work);
    work();
    for (std::thread& t : th) t.join();
    size_t total = 0; for (size_t s : sizes) total += s;
    return total;
}

static void write_all(const unsigned char* p, size_t n) { while (n) { const ssize_t w = write(1, p, n); if (w <= 0) exit(0); p += w; n -= (size_t)w; } }

int main(int argc, char** argv) {
    if (argc >= 3 && !strcmp(argv[1], "pipe")) {
        const int threads = atoi(argv[2]), level = argc > 3 ? atoi(argv[3]) : 1;
        const size_t B = (32u << 20) / M * M;
        std::vector<unsigned char> in(B), slots, packed; std::vector<size_t> sizes;
        for (;;) {
            size_t n = 0; ssize_t g;
            while (n < B && (g = read(0, in.data() + n, B - n)) > 0) n += (size_t)g;
            if (!n) break;
            const size_t total = batch(in.data(), n, slots, sizes, threads, level);
            packed.resize(total); size_t o = 0;
            for (size_t i = 0; i < sizes.size(); ++i) { memcpy(packed.data() + o, slots.data() + i * SLOT, sizes[i]); o += sizes[i]; }
            write_all(packed.data(), total);
            if (n < B) break;
        }
        write_all(kEof, sizeof kEof);
        return 0;
    }
    if (argc >= 5 && !strcmp(argv[1], "bench")) {
        FILE* f = fopen(argv[2], "rb"); if (!f) return 2;
        fseek(f, 0, SEEK_END); const size_t n = (size_t)ftell(f); fseek(f, 0, SEEK_SET);
        std::vector<unsigned char> in(n); if (fread(in.data(), 1, n, f) != n) return 2; fclose(f);
        const int threads = atoi(argv[3]), level = argc > 5 ? atoi(argv[5]) : 1; const double want = atof(argv[4]);
        std::vector<unsigned char> slots; std::vector<size_t> sizes;
        size_t total = batch(in.data(), n, slots, sizes, threads, level);              // warm-up
        const auto t0 = std::chrono::steady_clock::now(); int reps = 0; double s = 0;
        do { total = batch(in.data(), n, slots, sizes, threads, level); ++reps; s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); } while (s < want);
        printf("%d %.6f %zu\n", reps, s, total);
        return 0;
    }
    fprintf(stderr, "usage: deflate_host pipe THREADS [LEVEL] | bench FILE THREADS SECONDS [LEVEL]\n");
    return 2;
}
