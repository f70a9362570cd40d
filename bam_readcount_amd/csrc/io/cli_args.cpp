// cli_args.cpp — what the command line is told: its options (boost::program_options' unix style, as the reference's main() reads
// them), the knob table (the environment, read once), and the parsers of regions, -l lines and --brc-rank-of.  Pure functions: they
// open nothing and print nothing (tests/sim/cli_check.cpp drives them).
#include <errno.h>
#include <limits.h>

#include <algorithm>

#include "cli_internal.h"

const char* const kUsage =
    "Usage: bam-readcount [OPTIONS] bam_file|cram_file [region]\n"
    "Generate metrics for bam_file at single nucleotide positions.\n"
    "Example: bam-readcount -f ref.fa some.bam|some.cram\n\n"
    "Available options:\n"
    "  -h [ --help ]                         produce this message\n"
    "  -v [ --version ]                      output the version number\n"
    "  -q [ --min-mapping-quality ] arg (=0) minimum mapping quality of reads used \n"
    "                                        for counting.\n"
    "  -b [ --min-base-quality ] arg (=0)    minimum base quality at a position to \n"
    "                                        use the read for counting.\n"
    "  -d [ --max-count ] arg (=10000000)    max depth to avoid excessive memory \n"
    "                                        usage.\n"
    "  -l [ --site-list ] arg                file containing a list of regions to \n"
    "                                        report readcounts within.\n"
    "  -f [ --reference-fasta ] arg          reference sequence in the fasta format.\n"
    "  -D [ --print-individual-mapq ] arg    report the mapping qualities as a comma \n"
    "                                        separated list.\n"
    "  -p [ --per-library ]                  report results by library.\n"
    "  -w [ --max-warnings ] arg             maximum number of warnings of each type \n"
    "                                        to emit. -1 gives an unlimited number.\n"
    "  -i [ --insertion-centric ]            generate indel centric readcounts. Reads \n"
    "                                        containing insertions will not be \n"
    "                                        included in per-base counts\n\n";

struct OptSpec { char s; const char* l; bool takes_value; };
static const OptSpec kSpecs[] = {
    {'h', "help", false}, {'v', "version", false}, {'q', "min-mapping-quality", true}, {'b', "min-base-quality", true},
    {'d', "max-count", true}, {'l', "site-list", true}, {'f', "reference-fasta", true}, {'D', "print-individual-mapq", true},
    {'p', "per-library", false}, {'w', "max-warnings", true}, {'i', "insertion-centric", false}, {0, "brc-chunk", true}, {1, "brc-plan", true}, {2, "brc-gpus", true}, {3, "brc-streams", true},
    {4, "brc-ranks", true}, {5, "brc-rank-of", true}, {6, "brc-tmpdir", true}, {7, "brc-device-inflate", false},
    {8, "brc-bgzf-output", false},
};

static bool apply(Options& o, const OptSpec& sp, const std::string& v, std::string* err) {
    auto to_ll = [&](long long* out) {
        char* e = nullptr; errno = 0; const long long x = strtoll(v.c_str(), &e, 10);
        if (errno || e == v.c_str() || *e) { *err = "the argument ('" + v + "') for option '--" + sp.l + "' is invalid"; return false; }
        *out = x; return true;
    };
    // (boost::program_options: none of the reference's options is composing — a second occurrence is an error, :463)
    const unsigned bit = 1u << (unsigned)(&sp - kSpecs);
    if (o.seen & bit) { *err = std::string("option '--") + sp.l + "' cannot be specified more than once"; return false; }
    o.seen |= bit;
    long long x = 0;
    switch (sp.s) {
        case 'h': o.help = true; return true;
        case 'v': o.version = true; return true;
        case 'p': o.per_lib = true; return true;
        case 'i': o.insertion_centric = true; return true;
        case 'q': if (!to_ll(&x)) return false; o.min_mapq = (int)x; return true;
        case 'b': if (!to_ll(&x)) return false; o.min_bq = (int)x; return true;
        case 'd': if (!to_ll(&x)) return false; o.max_cnt = (int)x; return true;
        case 'w': if (!to_ll(&x)) return false; o.max_warnings = x; return true;
        case 'l': o.site_list = v; return true;
        case 'f': o.fasta = v; return true;
        case 'D': o.distribution = (v == "1" || v == "true" || v == "yes" || v == "on"); return true;
        case 1: if (!to_ll(&x)) return false; o.plan_sites = x; return true;
        case 2: if (!to_ll(&x)) return false; o.gpus = x; return true;
        case 3: if (!to_ll(&x)) return false; o.streams = x; return true;
        case 4: if (!to_ll(&x)) return false; o.ranks = x; return true;
        case 5: o.rank_of = v; return true;
        case 6: o.tmpdir = v; return true;
        case 7: o.device_inflate = true; return true;
        case 8: o.bgzf_output = true; return true;
        default: if (!to_ll(&x)) return false; o.chunk_bp = x; o.chunk_given = true; return true;
    }
}

bool parse_args(int argc, char** argv, Options& o, std::string* err) {
    std::vector<std::string> pos;
    bool only_pos = false;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (only_pos || a.size() < 2 || a[0] != '-') { pos.push_back(a); continue; }
        if (a == "--") { only_pos = true; continue; }
        if (a[1] == '-') {                                   // long option, optional =value, unambiguous prefix
            const size_t eq = a.find('=');
            const std::string name = a.substr(2, eq == std::string::npos ? std::string::npos : eq - 2);
            const OptSpec* hit = nullptr; int nhit = 0;
            for (const OptSpec& sp : kSpecs) {
                if (name == sp.l) { hit = &sp; nhit = 1; break; }
                if (strncmp(sp.l, name.c_str(), name.size()) == 0) { hit = &sp; ++nhit; }
            }
            if (nhit == 0) { *err = "unrecognised option '" + a + "'"; return false; }
            if (nhit > 1) { *err = "option '" + a + "' is ambiguous"; return false; }
            std::string v;
            if (hit->takes_value) {
                if (eq != std::string::npos) v = a.substr(eq + 1);
                else if (i + 1 < argc) v = argv[++i];
                else { *err = std::string("the required argument for option '--") + hit->l + "' is missing"; return false; }
            } else if (eq != std::string::npos) { *err = "option '--" + name + "' does not take any arguments"; return false; }
            if (!apply(o, *hit, v, err)) return false;
            continue;
        }
        for (size_t k = 1; k < a.size(); ++k) {              // short options, sticky
            const OptSpec* hit = nullptr;
            for (const OptSpec& sp : kSpecs) if (sp.s >= 'A' && sp.s == a[k]) hit = &sp;      // (codes below 'A' name the long-only --brc-* options)
            if (!hit) { *err = std::string("unrecognised option '-") + a[k] + "'"; return false; }
            if (hit->takes_value) {
                std::string v = a.substr(k + 1);
                if (v.empty()) { if (i + 1 < argc) v = argv[++i]; else { *err = std::string("the required argument for option '--") + hit->l + "' is missing"; return false; } }
                if (!apply(o, *hit, v, err)) return false;
                break;
            }
            if (!apply(o, *hit, "", err)) return false;
        }
    }
    if (!pos.empty()) { o.bam = pos[0]; o.regions.assign(pos.begin() + 1, pos.end()); }
    return true;
}

// ---------------------------------------------------------------- the knob table
Knobs g_knobs;

static std::vector<int> parse_device_list(const char* s) {      // "0,2,3"
    std::vector<int> out;
    for (const char* q = s; *q;) { out.push_back(atoi(q)); while (*q && *q != ',') ++q; if (*q) ++q; }
    return out;
}

static std::vector<std::string> parse_visible_list(const char* s) {      // "0,GPU-1234," -> its entries, empty ones too
    std::vector<std::string> out; std::string cur;
    for (const char* q = s;; ++q) { if (*q == ',' || !*q) { out.push_back(cur); cur.clear(); if (!*q) break; } else cur.push_back(*q); }
    return out;
}

Knobs read_knobs(const char* (*lookup)(const char*)) {
    auto get = [lookup](const char* name) -> const char* { return lookup ? lookup(name) : getenv(name); };
    auto unless_zero = [&](const char* name) { const char* v = get(name); return !(v && atoi(v) == 0); };
    auto if_nonzero = [&](const char* name) { const char* v = get(name); return v && atoi(v) != 0; };
    auto positive = [&](const char* name, long long otherwise) { const char* v = get(name); return v && atoll(v) > 0 ? atoll(v) : otherwise; };
    auto positive_int = [&](const char* name, int otherwise) { const char* v = get(name); return v && atoi(v) > 0 ? atoi(v) : otherwise; };
    Knobs k;
    k.zero_copy = unless_zero("BRC_ZERO_COPY"); k.device_text = unless_zero("BRC_DEVICE_TEXT"); k.rank_narrow = unless_zero("BRC_RANK_NARROW");
    k.rank_affinity = unless_zero("BRC_RANK_AFFINITY"); k.pin_ahead = unless_zero("BRC_PIN_AHEAD"); k.site_ahead = unless_zero("BRC_SITE_AHEAD");
    k.device_inflate = if_nonzero("BRC_DEVICE_INFLATE"); k.bgzf_output = if_nonzero("BRC_BGZF_OUTPUT");
    k.fetch_threads = positive_int("BRC_FETCH_THREADS", 0); k.fetch_ahead = positive_int("BRC_FETCH_AHEAD", 2);
    k.plan_vmax = positive("BRC_PLAN_VMAX", 0); k.rank_cut = positive("BRC_RANK_CUT", 65536);
    if (const char* v = get("BRC_CHUNK_BYTES")) if (atof(v) > 0) k.chunk_bytes = atof(v);
    // (BRC_BGZF_BATCH within 64 KB .. 1 GB: the library holds about three times the batch on the device, and three page-locked buffers of it here)
    if (const long long b = positive("BRC_BGZF_BATCH", 0)) k.bgzf_batch = (size_t)std::min<long long>(std::max<long long>(b, 65536), 1ll << 30);
    if (const char* v = get("BRC_FETCH_STRIPE_MIN")) k.fetch_stripe_min = atoll(v);
    if (const char* v = get("BRC_RANKS")) k.ranks = atoll(v);
    if (const char* v = get("BRC_STREAMS")) k.streams = atoll(v);
    if (const char* v = get("BRC_DEVICE")) { k.has_device = true; k.device = atoi(v); }
    if (const char* v = get("BRC_RANK_STATUS_FD")) k.rank_status_fd = atoi(v);
    k.cli_timing = get("BRC_CLI_TIMING") != nullptr;
    k.clean_exit = get("BRC_CLEAN_EXIT") != nullptr || get("BRC_ENGINE_TIMING") != nullptr;
    if (const char* v = get("BRC_INFLATE_LIB")) { k.has_inflate_lib = true; k.inflate_lib = v; }
    if (const char* v = get("BRC_DEFLATE_LIB")) { k.has_deflate_lib = true; k.deflate_lib = v; }
    if (const char* v = get("TMPDIR")) k.tmpdir = v;
    if (const char* v = get("BRC_DEVICES")) k.devices = parse_device_list(v);
    if (const char* v = get("HIP_VISIBLE_DEVICES")) k.visible = parse_visible_list(v);
    if (const char* v = get("BRC_CRASH_DIR")) { k.has_crash_dir = true; snprintf(k.crash_dir, sizeof k.crash_dir, "%s", v); }
    return k;
}

// ---------------------------------------------------------------- regions, -l lines, --brc-rank-of
// A command-line region as samtools-1.10's legacy bam_parse_region reads it (bamreadcount.cpp:644; bam.c: hts_parse_reg, and
// when that fails the whole string as a contig name): the name ends at the LAST colon; numbers go through
// hts_parse_decimal (leading white space, sign, thousands commas, fraction, exponent, k/M/G suffix; stderr notes for a
// discarded fraction and for trailing characters); "chr:beg" runs to the end, beg <= 0 means 1, an interval that is empty
// or past INT_MAX is no region.  Returns tid, 0-based beg, end.
static long long parse_decimal_like_htslib(const char* str, const char** strend, std::string* log) {
    auto push = [](long long v, char ch) { const int d = ch - '0'; return v > (LLONG_MAX - d) / 10 ? LLONG_MAX : 10 * v + d; };
    long long n = 0; int decimals = 0, e = 0, lost = 0; char sign = '+', esign = '+';
    while (*str == ' ' || (*str >= '\t' && *str <= '\r')) ++str;
    const char* q = str;
    if (*q == '+' || *q == '-') sign = *q++;
    while (*q) { if (*q >= '0' && *q <= '9') n = push(n, *q++); else if (*q == ',') ++q; else break; }
    if (*q == '.') { ++q; while (*q >= '0' && *q <= '9') { ++decimals; n = push(n, *q++); } }
    switch (*q) {
        case 'e': case 'E':
            ++q; if (*q == '+' || *q == '-') esign = *q++;
            while (*q >= '0' && *q <= '9') e = (int)push(e, *q++);
            if (esign == '-') e = -e;
            break;
        case 'k': case 'K': e += 3; ++q; break;
        case 'm': case 'M': e += 6; ++q; break;
        case 'g': case 'G': e += 9; ++q; break;
    }
    e -= decimals;
    while (e > 0) { n *= 10; --e; }
    while (e < 0) { lost += (int)(n % 10); n /= 10; ++e; }
    if (lost > 0) *log += "[W::hts_parse_decimal] Discarding fractional part of " + std::string(str, q) + "\n";
    if (strend) *strend = q;
    else if (*q) *log += "[W::hts_parse_decimal] Ignoring unknown characters after " + std::string(str, q) + "[" + q + "]\n";
    return sign == '+' ? n : -n;
}

bool parse_region(const BamHeader& h, const std::string& s, int* tid, int64_t* beg, int64_t* end, std::string* log) {
    // (log: what htslib writes to stderr while it parses — the caller prints it when the reference would reach this region)
    const size_t colon = s.rfind(':');
    bool ok = true;                                                 // parsable as a region
    long long b = 0, e = 0;
    if (colon == std::string::npos) { b = 0; e = LLONG_MAX; }
    else {
        const char* hyphen = nullptr;
        b = parse_decimal_like_htslib(s.c_str() + colon + 1, &hyphen, log) - 1;
        if (b < 0) b = 0;
        if (*hyphen == '\0') e = LLONG_MAX;
        else if (*hyphen == '-') e = parse_decimal_like_htslib(hyphen + 1, nullptr, log);
        else ok = false;
        if (ok && b >= e) ok = false;
    }
    // hts_parse_reg narrows hts_parse_reg64's positions to int whatever that returned
    if (b > INT_MAX) { *log += "[E::hts_parse_reg] Position " + std::to_string(b) + " too large\n"; ok = false; }
    else if (e > INT_MAX) { if (e == LLONG_MAX) e = INT_MAX; else { *log += "[E::hts_parse_reg] Position " + std::to_string(e) + " too large\n"; ok = false; } }
    size_t name_lim = colon == std::string::npos ? s.size() : colon;
    if (!ok) { name_lim = s.size(); b = 0; e = INT_MAX; }            // ... but possibly a contig named "foo:a"
    auto it = h.name2tid.find(s.substr(0, name_lim));
    if (it == h.name2tid.end()) return false;
    *tid = it->second; *beg = b; *end = e;
    return true;
}

// One line of the site list as `std::stringstream ss(line); ss >> ref_name >> beg >> end` reads it (bamreadcount.cpp:574-577):
// fields separated by any white space, the numbers as the stream's num_get takes them — optional sign, decimal digits, stop
// at the first other character; no digit, or a value outside int, fails the extraction and the line is skipped.
bool parse_site_line(const char* p, size_t n, std::string* name, int* beg, int* end) {
    const char* e = p + n;
    if (n && e[-1] == '\n') --e;                                   // (getline drops the delimiter; a '\r' stays and is white space)
    auto space = [](char ch) { return ch == ' ' || (ch >= '\t' && ch <= '\r'); };
    auto skip = [&]() { while (p < e && space(*p)) ++p; };
    skip();
    const char* b = p;
    while (p < e && !space(*p)) ++p;
    if (p == b) return false;
    name->assign(b, p);
    auto integer = [&](int* out) {
        skip();
        bool neg = false;
        if (p < e && (*p == '+' || *p == '-')) { neg = *p == '-'; ++p; }
        const char* d = p; long long v = 0; bool over = false;
        while (p < e && *p >= '0' && *p <= '9') { if (v < (1ll << 40)) v = v * 10 + (*p - '0'); else over = true; ++p; }
        if (p == d) return false;
        if (neg) v = -v;
        if (over || v > 2147483647ll || v < -2147483648ll) return false;
        *out = (int)v; return true;
    };
    return integer(beg) && integer(end);
}

bool parse_rank_of(const std::string& v, int* r, int* n) {
    const size_t c = v.find(':');
    if (c == std::string::npos) return false;
    char* e = nullptr; const long a = strtol(v.c_str(), &e, 10); if (e != v.c_str() + c) return false;
    const long b = strtol(v.c_str() + c + 1, &e, 10); if (*e || e == v.c_str() + c + 1) return false;
    if (b < 1 || b > 4096 || a < 0 || a >= b) return false;
    *r = (int)a; *n = (int)b; return true;
}
