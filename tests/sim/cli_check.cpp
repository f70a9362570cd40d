// cli_check — the pure parts of the command line (cli_args.cpp: the knob table and the parsers; cli_ranks.cpp: rank_slice) as a
// stand-alone program for the host sanitizers (tests/sim/Makefile: asan; tests/test_cli.py runs it).  It checks its own results.
#include <limits.h>
#include <math.h>

#include "../../bam_readcount_amd/csrc/io/cli_internal.h"

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "cli_check: line %d: %s\n", __LINE__, #c); ++g_fail; } } while (0)

// ---------------------------------------------------------------- knobs: an environment of one variable
static const char* g_name = nullptr; static const char* g_value = nullptr;
static const char* one_variable(const char* name) { return g_name && strcmp(name, g_name) == 0 ? g_value : nullptr; }
static Knobs with(const char* name, const char* value) { g_name = name; g_value = value; return read_knobs(one_variable); }

// the values every knob is tried with; the last one is the knob's own large value
enum { UNSET, EMPTY, ZERO, ONE, MINUS, WORD, LARGE, N_VALUES };
static const char* const kValues[N_VALUES] = {nullptr, "", "0", "1", "-1", "abc", nullptr};
// what the five rules of cli_internal.h (Knobs) answer for them.  D: the knob's default, L: its large value as the knob keeps it,
// U: "1" as the knob keeps it (BRC_BGZF_BATCH lifts it to its floor)
enum Rule { OFF_IF_ZERO, ON_IF_NONZERO, IF_POSITIVE, AS_GIVEN, PRESENCE };
static const double D = 1e300, L = 2e300, U = 3e300;
static const double kExpect[5][N_VALUES] = {
    /* OFF_IF_ZERO   */ {1, 0, 0, 1, 1, 0, 1},
    /* ON_IF_NONZERO */ {0, 0, 0, 1, 1, 0, 1},
    /* IF_POSITIVE   */ {D, D, D, U, D, D, L},
    /* AS_GIVEN      */ {D, 0, 0, 1, -1, 0, L},
    /* PRESENCE      */ {0, 1, 1, 1, 1, 1, 1},
};
struct KnobCase { const char* name; Rule rule; double (*get)(const Knobs&); double dflt; const char* large; double large_kept; double one_kept; };
#define GET(expr) [](const Knobs& k) -> double { return (double)(expr); }
static const double kTwo40 = 1099511627776.0;
static const KnobCase kKnobs[] = {
    {"BRC_ZERO_COPY", OFF_IF_ZERO, GET(k.zero_copy), 1, "2000000000", 1, 1},
    {"BRC_DEVICE_TEXT", OFF_IF_ZERO, GET(k.device_text), 1, "2000000000", 1, 1},
    {"BRC_RANK_NARROW", OFF_IF_ZERO, GET(k.rank_narrow), 1, "2000000000", 1, 1},
    {"BRC_RANK_AFFINITY", OFF_IF_ZERO, GET(k.rank_affinity), 1, "2000000000", 1, 1},
    {"BRC_PIN_AHEAD", OFF_IF_ZERO, GET(k.pin_ahead), 1, "2000000000", 1, 1},
    {"BRC_SITE_AHEAD", OFF_IF_ZERO, GET(k.site_ahead), 1, "2000000000", 1, 1},
    {"BRC_DEVICE_INFLATE", ON_IF_NONZERO, GET(k.device_inflate), 0, "2000000000", 1, 1},
    {"BRC_BGZF_OUTPUT", ON_IF_NONZERO, GET(k.bgzf_output), 0, "2000000000", 1, 1},
    {"BRC_FETCH_THREADS", IF_POSITIVE, GET(k.fetch_threads), 0, "2000000000", 2e9, 1},      // (read with atoi: a large value that an int holds)
    {"BRC_FETCH_AHEAD", IF_POSITIVE, GET(k.fetch_ahead), 2, "2000000000", 2e9, 1},
    {"BRC_PLAN_VMAX", IF_POSITIVE, GET(k.plan_vmax), 0, "1099511627776", kTwo40, 1},
    {"BRC_RANK_CUT", IF_POSITIVE, GET(k.rank_cut), 65536, "1099511627776", kTwo40, 1},
    {"BRC_CHUNK_BYTES", IF_POSITIVE, GET(k.chunk_bytes), 26.0e6, "1099511627776", kTwo40, 1},
    {"BRC_BGZF_BATCH", IF_POSITIVE, GET(k.bgzf_batch), 33554432, "1099511627776", 1073741824, 65536},      // within 64 KB .. 1 GB
    {"BRC_FETCH_STRIPE_MIN", AS_GIVEN, GET(k.fetch_stripe_min), 65536, "1099511627776", kTwo40, 1},
    {"BRC_RANKS", AS_GIVEN, GET(k.ranks), 0, "1099511627776", kTwo40, 1},
    {"BRC_STREAMS", AS_GIVEN, GET(k.streams), 1, "1099511627776", kTwo40, 1},
    {"BRC_DEVICE", AS_GIVEN, GET(k.device), 0, "2000000000", 2e9, 1},
    {"BRC_RANK_STATUS_FD", AS_GIVEN, GET(k.rank_status_fd), -1, "2000000000", 2e9, 1},
    {"BRC_CLI_TIMING", PRESENCE, GET(k.cli_timing), 0, "2000000000", 1, 1},
    {"BRC_CLEAN_EXIT", PRESENCE, GET(k.clean_exit), 0, "2000000000", 1, 1},
    {"BRC_ENGINE_TIMING", PRESENCE, GET(k.clean_exit), 0, "2000000000", 1, 1},
};

static void check_knobs() {
    for (const KnobCase& kc : kKnobs)
        for (int v = 0; v < N_VALUES; ++v) {
            const Knobs k = with(v == UNSET ? nullptr : kc.name, v == LARGE ? kc.large : kValues[v]);
            double want = kExpect[kc.rule][v];
            want = want == D ? kc.dflt : want == L ? kc.large_kept : want == U ? kc.one_kept : want;
            const double got = kc.get(k);
            if (got != want) { fprintf(stderr, "cli_check: %s=%s: %.17g, expected %.17g\n", kc.name, v == UNSET ? "(unset)" : v == LARGE ? kc.large : kValues[v], got, want); ++g_fail; }
        }
    // the examples of the knob table's own description
    CHECK(with("BRC_FETCH_AHEAD", nullptr).fetch_ahead == 2 && with("BRC_FETCH_AHEAD", "0").fetch_ahead == 2 && with("BRC_FETCH_AHEAD", "-1").fetch_ahead == 2 && with("BRC_FETCH_AHEAD", "abc").fetch_ahead == 2);
    CHECK(!with("BRC_ZERO_COPY", "abc").zero_copy);
    CHECK(!with("BRC_DEVICE_INFLATE", "abc").device_inflate);
    CHECK(with("BRC_BGZF_BATCH", "1").bgzf_batch == 65536);
    CHECK(with("BRC_BGZF_BATCH", "1099511627776").bgzf_batch == (size_t)1 << 30);
    CHECK(with("BRC_FETCH_STRIPE_MIN", "0").fetch_stripe_min == 0);
    CHECK(with("BRC_CLI_TIMING", "").cli_timing);
    // BRC_DEVICE: whether it was given matters too (a single engine takes it, --brc-gpus 2 does not)
    CHECK(!with(nullptr, nullptr).has_device && with("BRC_DEVICE", "").has_device && with("BRC_DEVICE", "3").device == 3);
    // the libraries: used as given if set, even if empty; TMPDIR: used if non-empty
    CHECK(!with(nullptr, nullptr).has_inflate_lib && !with(nullptr, nullptr).has_deflate_lib);
    CHECK(with("BRC_INFLATE_LIB", "").has_inflate_lib && with("BRC_INFLATE_LIB", "").inflate_lib.empty() && with("BRC_INFLATE_LIB", "/x/y.so").inflate_lib == "/x/y.so");
    CHECK(with("BRC_DEFLATE_LIB", "").has_deflate_lib && with("BRC_DEFLATE_LIB", "").deflate_lib.empty() && with("BRC_DEFLATE_LIB", "z.so").deflate_lib == "z.so");
    CHECK(!with("BRC_INFLATE_LIB", "a").has_deflate_lib && !with("BRC_DEFLATE_LIB", "a").has_inflate_lib);
    CHECK(with(nullptr, nullptr).tmpdir.empty() && with("TMPDIR", "").tmpdir.empty() && with("TMPDIR", "/var/tmp").tmpdir == "/var/tmp");
    // the two lists
    CHECK(with(nullptr, nullptr).devices.empty() && with("BRC_DEVICES", "").devices.empty());
    CHECK((with("BRC_DEVICES", "0,2,3").devices == std::vector<int>{0, 2, 3}) && (with("BRC_DEVICES", "1").devices == std::vector<int>{1}) && (with("BRC_DEVICES", "4,,x,").devices == std::vector<int>{4, 0, 0}));
    CHECK(with(nullptr, nullptr).visible.empty() && (with("HIP_VISIBLE_DEVICES", "").visible == std::vector<std::string>{""}));
    CHECK((with("HIP_VISIBLE_DEVICES", "0,GPU-1,").visible == std::vector<std::string>{"0", "GPU-1", ""}) && (with("HIP_VISIBLE_DEVICES", "7").visible == std::vector<std::string>{"7"}));
    // the crash directory: a copy of fixed size
    CHECK(!with(nullptr, nullptr).has_crash_dir && with("BRC_CRASH_DIR", "").has_crash_dir && strcmp(with("BRC_CRASH_DIR", "/tmp/c").crash_dir, "/tmp/c") == 0);
    const std::string longdir(2000, 'd'); const Knobs kl = with("BRC_CRASH_DIR", longdir.c_str());
    CHECK(strlen(kl.crash_dir) == sizeof kl.crash_dir - 1 && longdir.compare(0, sizeof kl.crash_dir - 1, kl.crash_dir) == 0);
}

// ---------------------------------------------------------------- parsers
static void check_rank_of() {
    struct { const char* v; bool ok; int r, n; } cases[] = {
        {"0:1", true, 0, 1}, {"3:4", true, 3, 4}, {"4:4", false, 0, 0}, {"-1:2", false, 0, 0}, {"1:", false, 0, 0},
        {":2", true, 0, 2},      // (no digits before the colon read as 0: what the parser has always done)
        {"1:4097", false, 0, 0}, {"1:2x", false, 0, 0}, {"12", false, 0, 0}, {"", false, 0, 0}, {"4095:4096", true, 4095, 4096}, {"1x:2", false, 0, 0},
    };
    for (const auto& c : cases) {
        int r = -7, n = -7; const bool ok = parse_rank_of(c.v, &r, &n);
        if (ok != c.ok || (ok && (r != c.r || n != c.n))) { fprintf(stderr, "cli_check: parse_rank_of(%s): %d %d:%d\n", c.v, (int)ok, r, n); ++g_fail; }
    }
}

static void check_site_line() {
    struct { const char* line; bool ok; const char* name; int beg, end; } cases[] = {
        {"chr1 10 20\n", true, "chr1", 10, 20}, {"chr1\t+5\t-3", true, "chr1", 5, -3}, {"  chr1 1 2\r\n", true, "chr1", 1, 2},
        {"chr1 1 2junk more", true, "chr1", 1, 2}, {"chr1 -2147483648 2147483647", true, "chr1", INT_MIN, INT_MAX},
        {"chr1 10", false, "", 0, 0}, {"chr1 x 5", false, "", 0, 0}, {"chr1 12abc 7", false, "", 0, 0}, {"chr1 2147483648 5", false, "", 0, 0},
        {"chr1 5 -2147483649", false, "", 0, 0}, {"chr1 99999999999999999999 1", false, "", 0, 0}, {"chr1 - 1", false, "", 0, 0},
        {"", false, "", 0, 0}, {"\n", false, "", 0, 0}, {"   \t\n", false, "", 0, 0}, {"chr1", false, "", 0, 0},
    };
    for (const auto& c : cases) {
        std::string name; int beg = -7, end = -7; const bool ok = parse_site_line(c.line, strlen(c.line), &name, &beg, &end);
        if (ok != c.ok || (ok && (name != c.name || beg != c.beg || end != c.end))) { fprintf(stderr, "cli_check: parse_site_line(%s): %d %s %d %d\n", c.line, (int)ok, name.c_str(), beg, end); ++g_fail; }
    }
}

static void check_region() {
    BamHeader h; h.names = {"chr1", "chr:x", "chr2"}; h.lengths = {1000, 500, 700};
    for (size_t i = 0; i < h.names.size(); ++i) h.name2tid[h.names[i]] = (int)i;
    struct { const char* s; bool ok; int tid; int64_t beg, end; const char* log; } cases[] = {
        {"chr1", true, 0, 0, INT_MAX, ""}, {"chr2", true, 2, 0, INT_MAX, ""}, {"nochr:1-2", false, 0, 0, 0, ""}, {"nochr", false, 0, 0, 0, ""},
        {"chr1:100-200", true, 0, 99, 200, ""}, {"chr1:100", true, 0, 99, INT_MAX, ""},
        {"chr1:1,000-2,000", true, 0, 999, 2000, ""},                                       // commas
        {"chr1:1k-2k", true, 0, 999, 2000, ""}, {"chr1:1M", true, 0, 999999, INT_MAX, ""}, {"chr1:1G-2G", true, 0, 999999999, 2000000000, ""},      // k/M/G
        {"chr1:1.5k-2k", true, 0, 1499, 2000, ""}, {"chr1:1e2-2E2", true, 0, 99, 200, ""},
        {"chr1:1.5-20", true, 0, 0, 20, "[W::hts_parse_decimal] Discarding fractional part of 1.5\n"},
        {"chr1:10-20x", true, 0, 9, 20, "[W::hts_parse_decimal] Ignoring unknown characters after 20[x]\n"},
        {"chr1:0-10", true, 0, 0, 10, ""}, {"chr1:-5-10", true, 0, 0, 10, ""},            // beg <= 0 means 1
        {"chr1:10-10", true, 0, 9, 10, ""}, {"chr1:11-10", false, 0, 0, 0, ""}, {"chr1:10-5", false, 0, 0, 0, ""},      // an empty interval is no region
        {"chr1:3G", false, 0, 0, 0, "[E::hts_parse_reg] Position 2999999999 too large\n"},                              // past INT_MAX
        {"chr1:5-3000000000", false, 0, 0, 0, "[E::hts_parse_reg] Position 3000000000 too large\n"},
        {"chr1:2147483647", true, 0, 2147483646, INT_MAX, ""}, {"chr1:1-2147483647", true, 0, 0, INT_MAX, ""},
        {"chr:x:5-6", true, 1, 4, 6, ""}, {"chr:x", true, 1, 0, INT_MAX, ""}, {"chr:x:", true, 1, 0, INT_MAX, ""},         // the name ends at the LAST colon; else the whole string is a name
    };
    for (const auto& c : cases) {
        int tid = -7; int64_t beg = -7, end = -7; std::string log; const bool ok = parse_region(h, c.s, &tid, &beg, &end, &log);
        if (ok != c.ok || log != c.log || (ok && (tid != c.tid || beg != c.beg || end != c.end))) { fprintf(stderr, "cli_check: parse_region(%s): %d tid %d [%lld, %lld) log '%s'\n", c.s, (int)ok, tid, (long long)beg, (long long)end, log.c_str()); ++g_fail; }
    }
}

// ---------------------------------------------------------------- rank_slice
static void check_cover(const std::vector<double>& w, int n) {
    size_t at = 0;
    for (int r = 0; r < n; ++r) {
        size_t lo = 99, hi = 99; rank_slice(w, r, n, &lo, &hi);
        if (lo != at || hi < lo || hi > w.size()) { fprintf(stderr, "cli_check: rank_slice: %zu weights, rank %d of %d: [%zu, %zu) behind %zu\n", w.size(), r, n, lo, hi, at); ++g_fail; return; }
        at = hi;
    }
    if (at != w.size()) { fprintf(stderr, "cli_check: rank_slice: %zu weights over %d ranks end at %zu\n", w.size(), n, at); ++g_fail; }
}

static void check_rank_slice() {
    const int ns[] = {1, 2, 3, 7};
    for (int n : ns) {
        const int lens[] = {0, 1, n - 1, n, n + 1};
        for (int m : lens) {
            if (m < 0) continue;
            std::vector<double> w((size_t)m);
            for (int i = 0; i < m; ++i) w[(size_t)i] = 1.0 + (double)((i * 7) % 5);
            check_cover(w, n);
            check_cover(std::vector<double>((size_t)m, 0.0), n);              // all-zero weights
            check_cover(std::vector<double>((size_t)m, 1.0), n);
        }
    }
    // three vectors worked out by hand with the rule of bam_readcount_amd/shard.py: partition — the atom that crosses a boundary goes to
    // the side that leaves the smaller excess
    struct { std::vector<double> w; int n; std::vector<size_t> cuts; } cases[] = {
        {{1, 1, 1, 1}, 2, {0, 2, 4}},                  // target 2: the second atom ends on it
        {{5, 1, 1, 1}, 2, {0, 1, 4}},                  // target 4 falls inside the first atom: 1 over is less than 4 under
        {{1, 2, 3, 4, 5, 6}, 3, {0, 3, 5, 6}},         // targets 7 and 14: 10 is 3 over, 6 is 1 under -> cut at 3; 15 is 1 over, 10 is 4 under -> cut at 5
    };
    for (const auto& c : cases)
        for (int r = 0; r < c.n; ++r) {
            size_t lo = 99, hi = 99; rank_slice(c.w, r, c.n, &lo, &hi);
            if (lo != c.cuts[(size_t)r] || hi != c.cuts[(size_t)r + 1]) { fprintf(stderr, "cli_check: rank_slice: %zu weights, rank %d of %d: [%zu, %zu), expected [%zu, %zu)\n", c.w.size(), r, c.n, lo, hi, c.cuts[(size_t)r], c.cuts[(size_t)r + 1]); ++g_fail; }
        }
}

int main() {
    check_knobs();
    check_rank_of();
    check_site_line();
    check_region();
    check_rank_slice();
    if (g_fail) { fprintf(stderr, "cli_check: %d checks failed\n", g_fail); return 1; }
    printf("cli_check ok: %zu knobs\n", sizeof kKnobs / sizeof kKnobs[0]);
    return 0;
}
