// host_check — the engine's host side (brc_host.cpp) over the CPU lane simulator as a stand-alone program for the host sanitizers
// (make asan: -fsanitize=address,undefined; tests/test_sim_parity.py runs it).  One walk through the life of an engine: create, a region
// with a pooled push, a window fetched behind the whole-region result, both ways to the text (brc_format_region and its parts), a
// refused push and the next region (pushed on one thread, in two batches), the device-text route, its line patcher regrowing its buffer
// in the middle of a line (the sanitizer's realloc always moves: a pointer kept across it is a report), the max-count rule, destroy.  Every
// step checks what it returns; the texts of the same reads must be the same bytes whichever way they came.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/brc.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "host_check: line %d: %s\n", __LINE__, #c); return 1; } } while (0)
#define OK(call) do { const int rc_ = (call); if (rc_ != BRC_OK) { fprintf(stderr, "host_check: line %d: %s -> %d\n", __LINE__, #call, rc_); return 1; } } while (0)

namespace {
struct Reads {
    std::vector<int32_t> pos, l_qseq, nm, sm; std::vector<uint16_t> flag; std::vector<uint8_t> mapq, tags, seq4, qual; std::vector<int16_t> lib;
    std::vector<uint32_t> n_cigar, cigar; std::vector<uint64_t> cigar_off, seq_off, qual_off;
    // reads [i0, i1) as a batch (offsets re-based to the sub-arenas, which are slices of the whole ones: the reads lie in file order)
    brc_read_batch batch(size_t i0, size_t i1, std::vector<uint64_t>* off) const {
        const size_t n = i1 - i0; off->resize(3 * n);
        for (size_t i = 0; i < n; ++i) { (*off)[i] = cigar_off[i0 + i] - cigar_off[i0]; (*off)[n + i] = seq_off[i0 + i] - seq_off[i0]; (*off)[2 * n + i] = qual_off[i0 + i] - qual_off[i0]; }
        const uint64_t c1 = i1 < pos.size() ? cigar_off[i1] : cigar.size(), s1 = i1 < pos.size() ? seq_off[i1] : seq4.size(), q1 = i1 < pos.size() ? qual_off[i1] : qual.size();
        brc_read_batch b; memset(&b, 0, sizeof b);
        b.n_reads = (int64_t)n; b.pos = pos.data() + i0; b.flag = flag.data() + i0; b.mapq = mapq.data() + i0; b.lib = lib.data() + i0; b.l_qseq = l_qseq.data() + i0;
        b.n_cigar = n_cigar.data() + i0; b.cigar_off = off->data(); b.seq_off = off->data() + n; b.qual_off = off->data() + 2 * n;
        b.nm = nm.data() + i0; b.sm = sm.data() + i0; b.tags = tags.data() + i0;
        b.cigar = cigar.data() + cigar_off[i0]; b.seq4 = seq4.data() + seq_off[i0]; b.qual = qual.data() + qual_off[i0];
        b.n_cigar_total = c1 - cigar_off[i0]; b.seq_bytes = s1 - seq_off[i0]; b.qual_bytes = q1 - qual_off[i0];
        return b;
    }
};
uint32_t rng_state = 12345u;
uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

// n reads of 100 or 101 bases over [0, len): plain matches, a deletion or an insertion in every fifth, two libraries, a mismatch here and there
Reads make_reads(const std::string& ref, size_t n) {
    Reads r; const int32_t len = (int32_t)ref.size();
    for (size_t i = 0; i < n; ++i) {
        const int32_t lq = 100 + (int32_t)(i % 7 == 0), p = (int32_t)((uint64_t)(i / 3) * 3 * (uint64_t)(len - 200) / n);      // (three reads start at every position: the max-count rule looks at such runs)
        const int kind = (int)(rnd() % 10);
        r.pos.push_back(p); r.l_qseq.push_back(lq); r.flag.push_back((rnd() & 1) ? 16 : 0); r.mapq.push_back((uint8_t)(20 + rnd() % 40)); r.lib.push_back((int16_t)(i % 2));
        r.nm.push_back((int32_t)(rnd() % 3)); r.sm.push_back(30); r.tags.push_back((uint8_t)(BRC_TAG_NM | BRC_TAG_SM));
        r.cigar_off.push_back(r.cigar.size()); r.seq_off.push_back(r.seq4.size()); r.qual_off.push_back(r.qual.size());
        if (kind == 0) { r.cigar.push_back(40u << 4); r.cigar.push_back((2u << 4) | 2u); r.cigar.push_back((uint32_t)(lq - 40) << 4); r.n_cigar.push_back(3); }          // 40M 2D ..M
        else if (kind == 1) { r.cigar.push_back(50u << 4); r.cigar.push_back((3u << 4) | 1u); r.cigar.push_back((uint32_t)(lq - 53) << 4); r.n_cigar.push_back(3); }     // 50M 3I ..M
        else { r.cigar.push_back((uint32_t)lq << 4); r.n_cigar.push_back(1); }
        for (int32_t j = 0; j < lq; j += 2) {
            uint8_t byte = 0;
            for (int h = 0; h < 2 && j + h < lq; ++h) {
                char c = ref[(size_t)(p + j + h)];
                if (rnd() % 50 == 0) c = "ACGT"[rnd() & 3];
                const uint8_t code = c == 'A' ? 1 : c == 'C' ? 2 : c == 'G' ? 4 : 8;
                byte |= (uint8_t)(code << (h == 0 ? 4 : 0));
            }
            r.seq4.push_back(byte);
        }
        for (int32_t j = 0; j < lq; ++j) r.qual.push_back((uint8_t)(2 + rnd() % 40));
    }
    return r;
}
// one read written down by hand: its bases are the reference's under the M operators
void add_read(Reads& r, const std::string& ref, int32_t pos, const std::vector<std::pair<int, int> >& ops, int16_t lib) {
    int32_t lq = 0; for (const auto& o : ops) if (o.first == 0 || o.first == 1 || o.first == 4) lq += o.second;
    r.pos.push_back(pos); r.l_qseq.push_back(lq); r.flag.push_back(0); r.mapq.push_back(50); r.lib.push_back(lib); r.nm.push_back(1); r.sm.push_back(30);
    r.tags.push_back((uint8_t)(BRC_TAG_NM | BRC_TAG_SM));
    r.cigar_off.push_back(r.cigar.size()); r.seq_off.push_back(r.seq4.size()); r.qual_off.push_back(r.qual.size()); r.n_cigar.push_back((uint32_t)ops.size());
    std::vector<uint8_t> codes; int32_t x = pos;
    for (const auto& o : ops) {
        r.cigar.push_back(((uint32_t)o.second << 4) | (uint32_t)o.first);
        if (o.first == 0) for (int j = 0; j < o.second; ++j, ++x) { const char c = ref[(size_t)x]; codes.push_back(c == 'A' ? 1 : c == 'C' ? 2 : c == 'G' ? 4 : 8); }
        else if (o.first == 2) x += o.second;
        else for (int j = 0; j < o.second; ++j) codes.push_back(1);
    }
    for (size_t j = 0; j < codes.size(); j += 2) r.seq4.push_back((uint8_t)((codes[j] << 4) | (j + 1 < codes.size() ? codes[j + 1] : 0)));
    for (int32_t j = 0; j < lq; ++j) r.qual.push_back(30);
}
// The line patcher of the device-text route (brc_host.cpp: format_device_text) with more to write than its buffer holds: a region that ends at
// the due position of 400 deletion alleles of 1 .. 400 bases leaves them pending; the next region's reads are plain, so the device's line at
// that position is some 150 bytes and the rewritten one about 100 KB — in a buffer that starts with 64 KiB and is regrown while the line is
// being written.  The text of the second region; the same steps through the host's own formatter (device_text == 0) are the expected value.
int patched_line(const std::string& ref, bool device_text, std::string* out) {
    brc_config cfg; memset(&cfg, 0, sizeof cfg);
    cfg.abi_version = BRC_ABI_VERSION;
    brc_engine* e = nullptr; brc_result res; std::vector<uint64_t> off; const char* t = nullptr; size_t n = 0;
    OK(brc_create(&cfg, &e));
    if (device_text) { OK(brc_set_option(e, BRC_OPT_TEXT_ONLY, 1)); OK(brc_set_option(e, BRC_OPT_DEVICE_TEXT, 1)); OK(brc_set_chrom(e, "chrS")); }
    const int32_t D = 500;
    Reads pending, plain;
    for (int d = 1; d <= 400; ++d) add_read(pending, ref, D - 20, {{0, 20}, {2, d}, {0, 10}}, 0);
    for (int32_t p = 440; p < 520; p += 20) add_read(plain, ref, p, {{0, 80}}, 0);
    for (int step = 0; step < 2; ++step) {
        const Reads& use = step ? plain : pending;
        OK(brc_begin_region(e, 0, step ? D - 5 : D - 10, step ? D + 5 : D, ref.data(), (int64_t)ref.size()));
        const brc_read_batch b = use.batch(0, use.pos.size(), &off);
        OK(brc_push_reads(e, &b));
        OK(brc_end_region(e, &res));
        OK(brc_format_region(e, &res, "chrS", &t, &n));              // (no brc_clear_indel_queue: the queue lives across the regions)
    }
    out->assign(t, n);
    brc_destroy(e);
    return 0;
}
// one region over the reads (pushed in batches of `step`) up to its result
int region(brc_engine* e, const std::string& ref, const Reads& r, size_t step, brc_result* res) {
    OK(brc_begin_region(e, 0, 0, (int32_t)ref.size(), ref.data(), (int64_t)ref.size()));
    std::vector<uint64_t> off;
    for (size_t i = 0; i < r.pos.size(); i += step) { const brc_read_batch b = r.batch(i, std::min(r.pos.size(), i + step), &off); OK(brc_push_reads(e, &b)); }
    OK(brc_end_region(e, res));
    return 0;
}
int text_of(brc_engine* e, const brc_result* res, std::string* out) {
    const char* t = nullptr; size_t n = 0;
    OK(brc_clear_indel_queue(e));
    OK(brc_format_region(e, res, "chrS", &t, &n));
    CHECK(t && t[n] == 0);
    out->assign(t, n);
    return 0;
}
}  // namespace

int main() {
    std::string ref(30000, 'A');
    for (char& c : ref) c = "ACGT"[rnd() & 3];
    const size_t N = 12000;                                   // (above the 8192 reads from which a batch is staged by the pool)
    const Reads reads = make_reads(ref, N);
    const char* names[2] = {"libA", "libB"};
    brc_config cfg; memset(&cfg, 0, sizeof cfg);
    cfg.abi_version = BRC_ABI_VERSION; cfg.per_lib = 1; cfg.n_libs = 2; cfg.lib_names = names; cfg.min_bq = 5;
    brc_engine* e = nullptr; brc_result res, win;
    OK(brc_create(&cfg, &e));

    // a region with a pooled push; its text; a window behind it leaves the whole-region result what it was
    std::string text_a, text_b;
    if (region(e, ref, reads, N, &res)) return 1;
    CHECK(res.n_events > 1000000 && res.n_indel > 100 && res.n_lib == 2);
    if (text_of(e, &res, &text_a)) return 1;
    CHECK(text_a.size() > 1000000);
    OK(brc_fetch_window(e, 1000, 2000, &win));
    CHECK(win.n_pos >= 1000 && win.n_pos <= 1001 && win.istat != res.istat && win.refbase != res.refbase && win.n_events > 0);
    for (int64_t k = 0; k < win.n_pos; ++k) CHECK(win.refbase[k] == res.refbase[win.pos0 - res.pos0 + k] && win.ncol[k] == res.ncol[win.pos0 - res.pos0 + k]);
    if (text_of(e, &res, &text_b)) return 1;
    CHECK(text_b == text_a);
    {   // the other way to the same text: its parts
        const char* const* parts = nullptr; const size_t* lens = nullptr; size_t np = 0; std::string cat;
        OK(brc_clear_indel_queue(e));
        OK(brc_format_region_parts(e, &res, "chrS", &parts, &lens, &np));
        for (size_t i = 0; i < np; ++i) cat.append(parts[i], lens[i]);
        CHECK(cat == text_a);
    }

    // a refused push abandons the region; the next region (one thread, two batches) is the first one again
    {
        Reads bad = reads; bad.l_qseq[9000] += 1; bad.l_qseq[11000] += 1;
        std::vector<uint64_t> off; const brc_read_batch b = bad.batch(0, N, &off);
        OK(brc_begin_region(e, 0, 0, (int32_t)ref.size(), ref.data(), (int64_t)ref.size()));
        CHECK(brc_push_reads(e, &b) == BRC_E_ARG && strstr(brc_last_error(e), "CIGAR and sequence length disagree"));
        const brc_read_batch g = reads.batch(0, 100, &off);
        CHECK(brc_push_reads(e, &g) == BRC_E_ARG && strstr(brc_last_error(e), "outside an open region"));
    }
    OK(brc_set_option(e, BRC_OPT_FORMAT_THREADS, 1));
    if (region(e, ref, reads, N / 2, &res) || text_of(e, &res, &text_b)) return 1;
    CHECK(text_b == text_a);
    brc_destroy(e); e = nullptr;

    // the device-text route: the lines come from the device code, the host joins them
    OK(brc_create(&cfg, &e));
    OK(brc_set_option(e, BRC_OPT_TEXT_ONLY, 1)); OK(brc_set_option(e, BRC_OPT_DEVICE_TEXT, 1)); OK(brc_set_chrom(e, "chrS"));
    if (region(e, ref, reads, N, &res)) return 1;
    CHECK(res.ncol == NULL && res.istat == NULL);
    if (text_of(e, &res, &text_b)) return 1;
    CHECK(text_b == text_a);
    brc_destroy(e); e = nullptr;

    // the line patcher with a line of 100 KB to rewrite: its buffer is regrown in the middle of the line
    {
        std::string dev, host;
        if (patched_line(ref, true, &dev) || patched_line(ref, false, &host)) return 1;
        size_t entries = 0;
        for (size_t i = 0; i + 1 < dev.size(); ++i) if (dev[i] == '\t' && dev[i + 1] == '-') ++entries;
        CHECK(dev == host && dev.size() > 65536 + 16384 && entries == 400);
    }

    // the max-count rule (one-thread pass whatever the batch's size): one large batch drops what batches of 1000 drop
    cfg.max_cnt = 15;
    OK(brc_create(&cfg, &e));
    if (region(e, ref, reads, N, &res)) return 1;
    const uint64_t ev_all = res.n_events;
    if (text_of(e, &res, &text_b)) return 1;
    std::string text_c;
    if (region(e, ref, reads, 1000, &res) || text_of(e, &res, &text_c)) return 1;
    CHECK(res.n_events == ev_all && text_c == text_b && text_b != text_a);
    brc_destroy(e);
    printf("host_check ok: %zu reads, %zu bytes of text\n", N, text_a.size());
    return 0;
}
