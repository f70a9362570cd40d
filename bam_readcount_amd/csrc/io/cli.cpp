// cli.cpp — `bam-readcount`-compatible command line over the C-ABI engine (include/brc.h).
//
// Mirrors main() of the reference (src/exe/bam-readcount/bamreadcount.cpp:421-670): same options and spellings
// (boost::program_options unix style: -q20, -q 20, --min-mapping-quality=20, --min-mapping-quality 20, sticky short
// switches -pi, unambiguous long prefixes), same positional arguments (BAM then regions), same stdout records, the same
// informational stderr lines, same -l site-list and region semantics including the "fetch one base early" rule (:602).
// What differs is below the callbacks: reads are batched and handed to the MI355X engine instead of bam_plbuf.
//
// Not reproduced (documented in DESIGN.md): whole-file mode without region or site list (the reference marks it FIXME
// and produces degraded output) is refused.
//
// Engine-side options (not in the reference): --brc-chunk (tiling of long regions), --brc-plan (site-list planner),
// --brc-gpus N / BRC_DEVICES=0,1,.. and --brc-streams K (K engines per GPU, each with a worker thread; work items — region
// pieces, site-list batches — are dealt out in file order and their text is written in file order).  Every engine
// pipelines consecutive pieces: piece k is formatted and written while piece k+1 is staged and on the GPU and piece k+2
// is being decoded.
//
// --brc-ranks N (one rank per GPU): the command line becomes N PROCESSES, started before any of them has touched
// the HIP runtime; rank r binds to GPU devices[r] and to its share of the CPUs, takes a contiguous, event-weighted slice of the
// work list IN FILE ORDER (the rule of shard.partition; weights from the index's file offsets, BamIndex::span_bytes) and prints
// it; the coordinating process writes the ranks' text and stderr in rank order — see cli_ranks.cpp.
//
// --brc-device-inflate (BRC_DEVICE_INFLATE=1; off by default): the BGZF blocks of a BAM are inflated on the GPU, a piece's worth per
// call, by the inflater library of include/brc_inflate.h — found with dlopen (BRC_INFLATE_LIB, else libbrc_inflate_hip.so next to
// this executable; a missing library or device is an error, exit code 1) — instead of one block at a time on the fetch threads.
// Output, messages and exit codes are those of the switch off.  Every rank opens its own inflater on its own GPU; CRAM input has no
// BGZF blocks and says once that the switch is ignored.
//
// --brc-bgzf-output (BRC_BGZF_OUTPUT=1; off by default): everything this program would write to stdout leaves as BGZF members instead,
// compressed on the GPU by the deflater library of include/brc_deflate.h — found with dlopen (BRC_DEFLATE_LIB, else
// libbrc_deflate_hip.so next to this executable; a missing library or device is an error, exit code 1, nothing on stdout).  One sink
// (BgzfSink, cli_output.cpp) sits behind every place that writes text; it gathers the text in page-locked buffers and compresses a batch per call
// on a thread of its own.  The end-of-file member follows the last member exactly once (with --brc-ranks: the coordinator appends it
// behind the last rank's members).  stderr and the exit code are those of the switch off; zcat of stdout is the switch-off stdout.
// --help and --version print their plain text whatever the switch says: they end the run before any input is opened or any library
// loaded, and what they print is for a person, not a file of records.  A write error on stdout other than a closed pipe ends the run
// with a message and exit code 1.
//
// The other units of this program: cli_internal.h lists them; the end of this file includes them.
#include <execinfo.h>
#include <fcntl.h>
#include <limits.h>
#include <signal.h>

#include <algorithm>
#include <atomic>
#include <future>

#include "cli_internal.h"

// ---------------------------------------------------------------- work items and engines
// The command line is turned into work items in file order: a site-list batch (narrow -l lines, planner), or a piece of a
// region / wide -l line.  One engine: the items run one after the other on it.  Several engines (--brc-gpus N, one per
// GPU, each with a worker thread and its own file handles): item i goes to engine i mod N — except the first piece of a
// command-line region, which follows the last piece of the previous region onto its engine, because it must see the
// deletions that piece left pending (the reference does not clear its queue between command-line regions, :641-657) —
// and the main thread writes the items' text in file order.
enum class WorkKind { Region, SiteBatch, Error, Message };      // a region piece; a site-list batch; an error that ends the run; a message (stderr) in file order
struct Work {
    WorkKind kind = WorkKind::Region;
    int tid = 0; int64_t beg0 = 0, end = 0; bool site_mode = false, keep_queue = false, inner_piece = false;
    std::vector<Site> sites;
    int engine = 0;
    std::string out, err, wev; int rc = 0; bool done = false;
    const char* const* parts = nullptr; const size_t* lens = nullptr; size_t n_parts = 0;      // a region piece's text, still in its engine's buffers
};

static int run_item(Ctx& c, Work& w) {
    if (w.kind == WorkKind::SiteBatch) return run_site_batch(c, w.sites);
    return run_region(c, w.tid, w.beg0, w.end, w.site_mode, w.keep_queue, w.inner_piece);
}

// A crash must not be silent: frames of the faulting thread (module + offset: `addr2line -e <module> <offset>` resolves
// them) go to stderr before the default action takes the process down.
static void crash_handler(int sig) {
    void* frames[64];
    const int n = backtrace(frames, 64);
    static const char msg[] = "bam-readcount: fatal signal, backtrace of the faulting thread:\n";
    if (write(2, msg, sizeof msg - 1) < 0) {}
    backtrace_symbols_fd(frames, n, 2);
    if (g_knobs.has_crash_dir) {       // (test harnesses: the same frames into a file of their own; BRC_CRASH_DIR as main() found it)
        char path[sizeof g_knobs.crash_dir + 48]; snprintf(path, sizeof path, "%s/brc_crash_%d.txt", g_knobs.crash_dir, (int)getpid());
        const int fd = open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (fd >= 0) { backtrace_symbols_fd(frames, n, fd); close(fd); }
    }
    signal(sig, SIG_DFL); raise(sig);
}

static void install_crash_handler() {
    struct sigaction sa; memset(&sa, 0, sizeof sa); sa.sa_handler = crash_handler; sigemptyset(&sa.sa_mask); sa.sa_flags = SA_RESETHAND;
    sigaction(SIGSEGV, &sa, nullptr); sigaction(SIGBUS, &sa, nullptr); sigaction(SIGABRT, &sa, nullptr); sigaction(SIGFPE, &sa, nullptr);
}

// ---------------------------------------------------------------- one run, phase by phase (main() is the table of contents)
static const int kGoOn = -1;            // what a phase returns when the run goes on (else: main's return value)
struct Run {
    Ctx c;                              // the first context: this thread's inputs, engine of devices[0]
    int my_rank = -1, n_ranks = 1;      // --brc-rank-of (-1: not one of a group)
    bool lead = true;                   // the process whose informational lines reach the caller (a single process, or rank 0)
    double t_start = 0, t_inputs = 0, t_engine0 = 0;
    std::vector<int> devices; size_t N = 1;      // the GPU of every engine; engines
    bool atoms = false;                 // a rank of a group first lists ATOMS — one -l line, or one 64-kb piece of a region / wide line, each with a weight —, takes its
    int64_t rank_cut = 65536;           // slice of them and joins what lies side by side in it back into batches and regions (take_rank_slice)
    std::vector<Work> items;            // the work, in file order
    // the inflater, the sink and the engine start on threads of their own while this one reads the index and the site list
    int inf_rc = 0, def_rc = 0; bool eng_reported = false;
    std::promise<int> eng_promise; std::shared_future<int> eng_ready;
    std::thread inf_thread; JoinOnExit join_inf{inf_thread};
    std::thread def_thread; JoinOnExit join_def{def_thread};
    std::thread eng_thread; JoinOnExit join_eng{eng_thread};
    std::thread pin_ahead; JoinOnExit join_pin{pin_ahead};
    // a rank tells the coordinator how it ended (exit code, ReadWarnings' counters, seconds)
    int leave(int rc) {
        if (my_rank >= 0 && g_knobs.rank_status_fd >= 0) {
            char b[256]; const int n = snprintf(b, sizeof b, "%d %lld %lld %lld %lld %.6f %d\n", rc, (long long)c.wcount[0], (long long)c.wcount[1], (long long)c.wcount[2], (long long)c.wcount[3], now_s() - t_start, g_sink && g_sink->calls ? 1 : 0);   // (last: --brc-bgzf-output, this rank wrote members)
            fflush(stdout); fflush(stderr);
            write_all(g_knobs.rank_status_fd, b, (size_t)n);
        }
        return rc;
    }
    // --brc-bgzf-output: whoever leaves before any text was written still leaves a whole BGZF file — its end-of-file member — unless the
    // deflater itself could not be had: then stdout stays empty
    int bail(int rc) { if (def_thread.joinable()) def_thread.join(); if (g_sink) g_sink->finish(my_rank < 0); return leave(rc); }
    bool wait_engine() {
        const int r = eng_ready.get();
        if (r && !eng_reported) { eng_reported = true; fprintf(stderr, "bam-readcount: cannot create the MI355X engine: %s\n", brc_strerror(r)); }
        return r == 0;
    }
};

// ranks: this process is one of a group (--brc-rank-of): its number, its share of the CPUs
static bool rank_setup(Run& R) {
    const Options& o = R.c.opt;
    if (!o.rank_of.empty()) {
        if (!parse_rank_of(o.rank_of, &R.my_rank, &R.n_ranks)) { fprintf(stderr, "bam-readcount: the argument ('%s') for option '--brc-rank-of' is invalid\n", o.rank_of.c_str()); return false; }
        g_ranks = (unsigned)R.n_ranks;
        if (R.n_ranks > 1 && g_knobs.rank_affinity) bind_rank_cpus(R.my_rank, R.n_ranks);
    }
    R.lead = R.my_rank <= 0;
    R.t_start = now_s();
    return true;
}

// --version, --help, and the hand-off to the coordinator of a group of ranks (which never initialises the GPU)
static int early_exit(Run& R, int argc, char** argv) {
    const Options& o = R.c.opt;
    if (o.version) { if (R.lead) printf("bam-readcount version: 1.0.1-mi355x (engine %s, abi %d)\n", brc_engine_kind(), BRC_ABI_VERSION); return R.leave(1); }   // :467-470
    if (o.help || o.bam.empty()) { if (R.lead) { fputs(kUsage, stdout); fputs("\n", stdout); } return R.leave(1); }                                                   // :472-475
    const long long want = o.ranks > 0 ? o.ranks : g_knobs.ranks;
    // (several command-line regions: one process — see cli_ranks.cpp; -D ends the run before any work)
    if (R.my_rank < 0 && want > 1 && !o.distribution && (!o.site_list.empty() || o.regions.size() == 1)) return coordinate(argc, argv, o, (int)std::min<long long>(want, 4096));
    return kGoOn;
}

// the input files, and the informational lines the reference prints while it opens them
static int open_run_inputs(Run& R) {
    Ctx& c = R.c; const Options& o = c.opt; const bool lead = R.lead;
    c.tag_warnings = R.my_rank > 0;
    if (lead) fprintf(stderr, "Minimum mapping quality is set to %d\n", o.min_mapq);                                                                 // :477
    if (!open_inputs(c, !lead)) return R.leave(1);
    R.t_inputs = now_s();
    if (lead) for (const std::string& l : c.header().expected) fprintf(stderr, "Expect library: %s in BAM\n", l.c_str());                                         // :526-529
    if (o.distribution) { if (lead) fprintf(stderr, "Not currently supporting distributions\n"); return R.leave(1); }                                          // :367 (the reference throws)
    // -d below any real depth changes which reads bam_plp_push keeps, and that depends on everything buffered before:
    // no internal pieces then (the planner is off for the same reason)
    if (o.max_cnt < 1000000) c.opt.chunk_bp = (long long)INT_MAX;
    return kGoOn;
}

// devices: BRC_DEVICES=0,2,3 or --brc-gpus N (devices 0..N-1); BRC_DEVICE=k for a single engine
static void resolve_devices(Run& R) {
    const Options& o = R.c.opt; std::vector<int>& devices = R.devices;
    if (R.my_rank < 0) devices = g_knobs.devices;
    if (R.my_rank >= 0) devices.push_back(g_knobs.device);       // one rank, one GPU
    if (devices.empty()) for (long long g = 0; g < std::max<long long>(o.gpus, 1); ++g) devices.push_back((o.gpus <= 1 && g_knobs.has_device) ? g_knobs.device : (int)g);
    if (R.my_rank < 0) {   // K engines per GPU, GPU-major round robin (engine i -> GPU i mod #GPUs)
        long long K = o.streams > 0 ? o.streams : g_knobs.streams;
        if (K < 1) K = 1;
        if (o.max_cnt < 1000000) K = 1;                  // (no internal pieces then)
        const std::vector<int> one = devices;
        for (long long k = 1; k < K; ++k) devices.insert(devices.end(), one.begin(), one.end());
    }
    // Deletions left pending by one command-line region reach into the next (the reference does not clear its queue there,
    // :641-657) and can block its deletions from the first position to the last: such runs keep every piece on one engine,
    // in order.  (One region — a chromosome — and site lists spread over the engines.)
    if (o.site_list.empty() && o.regions.size() > 1) devices.resize(1);
    R.N = devices.size();
}

// The inflater, the sink and the engine (HIP runtime start, streams) are created on threads of their own while this one reads the
// index and the site list and — inside the first work item — the reference and the first reads; whoever needs one waits for it.
static void start_background(Run& R) {
    Ctx& c = R.c;
    if (g_knobs.device_inflate) c.opt.device_inflate = true;
    if (c.opt.device_inflate) {
        if (c.is_cram) { c.opt.device_inflate = false; if (R.lead) fprintf(stderr, "bam-readcount: --brc-device-inflate is ignored for CRAM input\n"); }
    }
    if (c.opt.device_inflate) R.inf_thread = std::thread([&R]() { R.inf_rc = open_inflater(R.c, R.devices[0]); });
    if (g_knobs.bgzf_output) c.opt.bgzf_output = true;
    if (c.opt.bgzf_output) R.def_thread = std::thread([&R]() { R.def_rc = open_bgzf_sink(R.devices[0]); });
    R.eng_ready = R.eng_promise.get_future().share();
    R.eng_thread = std::thread([&R]() { const int r = make_engine(R.c, R.devices[0]); R.t_engine0 = now_s(); R.eng_promise.set_value(r); });
    c.need_engine = [&R]() { return R.wait_engine(); };
}

static void add_region(Run& R, int tid, int64_t beg0, int64_t end, bool site_mode) {
    // one engine: the region as a whole (run_region cuts it and fetches the next piece in the background); several:
    // its pieces become items of their own so that they spread over the GPUs
    end = clamp_to_contig(R.c.header(), tid, beg0, end);
    const int64_t step = R.atoms ? R.rank_cut : (R.N > 1 ? (int64_t)R.c.opt.chunk_bp : (int64_t)INT_MAX);
    bool first = true;
    int64_t a = beg0;
    do {
        // (atoms end on multiples of the cut: the index's windows, what the weights are known by)
        const int64_t b = std::min<int64_t>(R.atoms && step < (int64_t)INT_MAX ? (a / step + 1) * step : a + step, end);
        Work w; w.kind = WorkKind::Region; w.tid = tid; w.beg0 = a; w.end = b; w.site_mode = site_mode && b >= end;
        w.keep_queue = first && !site_mode;       // a -l line starts from an empty queue (:605 cleared it after the previous line)
        w.inner_piece = !first;
        R.items.push_back(std::move(w));
        first = false; a = b;
    } while (a < end);
}

static bool load_index(Run& R) {
    if (!R.c.is_cram && !R.c.idx.load(R.c.opt.bam)) { if (R.lead) fprintf(stderr, "BAM indexing file is not available.\n"); return false; }     // :548-551, :637-640
    return true;
}

static int items_from_site_list(Run& R) {
    Ctx& c = R.c; const Options& o = c.opt; std::vector<Work>& items = R.items;
    FILE* fp = fopen(o.site_list.c_str(), "r");
    if (!fp) { if (R.lead) fprintf(stderr, "Failed to open region list file: %s\n", o.site_list.c_str()); return R.bail(1); }            // :535-538
    if (!load_index(R)) return R.bail(1);
    // the planner needs -d to be out of play (its drop rule depends on what else is buffered) and narrow lines
    const bool plan = o.plan_sites > 0 && o.max_cnt >= 1000000 && !c.is_cram;
    Work pend; pend.kind = WorkKind::SiteBatch; int64_t pend_bp = 0;
    auto flush = [&]() { if (!pend.sites.empty()) { items.push_back(std::move(pend)); pend = Work(); pend.kind = WorkKind::SiteBatch; pend_bp = 0; } };
    char* line = nullptr; size_t line_cap = 0; ssize_t line_len;
    while ((line_len = getline(&line, &line_cap, fp)) >= 0) {                   // getline + ss >> ref_name >> beg >> end (:574-577)
        std::string name; int beg, end;
        if (!parse_site_line(line, (size_t)line_len, &name, &beg, &end)) continue;
        auto it = c.header().name2tid.find(name);
        if (it == c.header().name2tid.end()) {                                   // :580-582 — printed when the reference's loop reaches the line,
            flush();                                                             // i.e. behind the warnings of the lines before it: a work item of its own
            Work w; w.kind = WorkKind::Message; w.err = name + " not found in bam file. Region " + name + " " + std::to_string(beg) + " " + std::to_string(end) + " skipped.\n";
            items.push_back(std::move(w)); continue;
        }
        // pileup_func works on [beg - 2, end) in 0-based terms (:268 takes the position before the first printed one for
        // its deletions): a line whose end lies before that touches nothing
        if ((int64_t)end < (int64_t)beg - 1) continue;
        if (beg < 1) beg = 1;
        // (windows near the end of a contig run on their own: fetch_func's "Request for position" lines carry real coordinates)
        if (plan && (int64_t)end - beg < 1000 && (int64_t)end + 100000 < (int64_t)c.header().lengths[(size_t)it->second]) {
            Site st; st.tid = it->second; st.beg0 = (int64_t)beg - 1; st.end = end < beg - 1 ? beg - 1 : end;
            st.end = clamp_to_contig(c.header(), st.tid, st.beg0, st.end);
            pend.sites.push_back(st); pend_bp += (st.end - st.beg0) + 600;
            if (R.atoms || (long long)pend.sites.size() >= o.plan_sites || pend_bp > 4 * (int64_t)c.opt.chunk_bp) flush();
            continue;
        }
        flush();
        add_region(R, it->second, (int64_t)beg - 1, end, true);
    }
    flush();
    free(line);
    fclose(fp);
    return kGoOn;
}

static int items_from_regions(Run& R) {
    Ctx& c = R.c; const Options& o = c.opt;
    if (o.regions.empty()) {
        if (R.lead) fprintf(stderr, "bam-readcount: give a region or a site list (-l); the reference's whole-file mode skips its per-read "
                                    "pre-processing (bamreadcount.cpp:624 FIXME) and is not reproduced\n");
        return R.bail(1);
    }
    if (!load_index(R)) return R.bail(1);
    for (const std::string& r : o.regions) {
        int tid; int64_t beg, end; std::string log;
        if (!parse_region(c.header(), r, &tid, &beg, &end, &log)) {              // :645-648: the regions before it have been printed
            Work w; w.kind = WorkKind::Error; w.err = log + "Invalid region " + r + "\n"; w.rc = 1; R.items.push_back(std::move(w)); break;
        }
        if (!log.empty()) { Work w; w.kind = WorkKind::Message; w.err = log; R.items.push_back(std::move(w)); }
        add_region(R, tid, beg, end, false);
    }
    return kGoOn;
}

// this rank's slice of the atoms, in file order, by estimated work: the compressed bytes the index places under an atom —
// for a -l line, what its indexed fetch decodes: from the start of its 16-kb window to the line (bamio.h: span_bytes)
static void take_rank_slice(Run& R) {
    Ctx& c = R.c; const Options& o = c.opt; std::vector<Work>& items = R.items;
    std::vector<double> w(items.size(), 0.0); bool known = !c.is_cram;
    for (size_t i = 0; i < items.size() && known; ++i) {
        const Work& a = items[i];
        if (a.kind == WorkKind::Region) { w[i] = c.idx.span_bytes(a.tid, std::max<int64_t>(a.beg0 - 1, 0), std::max<int64_t>(a.end, a.beg0)); if (w[i] < 0) known = false; w[i] += 64.0; }
        else if (a.kind == WorkKind::SiteBatch) { const Site& s = a.sites[0]; w[i] = c.idx.span_bytes(s.tid, (std::max<int64_t>(s.beg0 - 1, 0) >> 14) << 14, std::max<int64_t>(s.end, s.beg0)); if (w[i] < 0) known = false; w[i] += 2048.0; }
    }
    if (!known) for (size_t i = 0; i < items.size(); ++i) { const Work& a = items[i]; w[i] = a.kind == WorkKind::Region ? (double)(a.end - a.beg0) + 1.0 : (a.kind == WorkKind::SiteBatch ? 1000.0 : 0.0); }   // (no offsets to weigh by: positions)
    size_t lo = 0, hi = 0;
    rank_slice(w, R.my_rank, R.n_ranks, &lo, &hi);
    // an error item ends the run where the reference's loop would have stopped: the rank that owns it reports it, the ranks behind
    // it have nothing to do (the coordinator drops whatever they print)
    std::vector<Work> mine;
    for (size_t i = lo; i < hi; ++i) {
        Work& a = items[i];
        if (!mine.empty()) {
            Work& p = mine.back();
            if (a.kind == WorkKind::SiteBatch && p.kind == WorkKind::SiteBatch && (long long)p.sites.size() < std::max<long long>(o.plan_sites, 1)) {
                int64_t bp = 0; for (const Site& s : p.sites) bp += (s.end - s.beg0) + 600;
                if (bp <= 4 * (int64_t)c.opt.chunk_bp) { p.sites.push_back(a.sites[0]); continue; }
            }
            if (a.kind == WorkKind::Region && p.kind == WorkKind::Region && a.inner_piece && a.tid == p.tid && a.beg0 == p.end && !p.site_mode) { p.end = a.end; p.site_mode = a.site_mode; continue; }
        }
        mine.push_back(std::move(a));
    }
    if (g_knobs.cli_timing) {
        double wm = 0, wt = 0; for (size_t i = 0; i < w.size(); ++i) { wt += w[i]; if (i >= lo && i < hi) wm += w[i]; }
        fprintf(stderr, "rank %d of %d: atoms [%zu, %zu) of %zu, %.4f of the estimated work (%s), %zu work items\n", R.my_rank, R.n_ranks, lo, hi, items.size(), wt > 0 ? wm / wt : 0.0, known ? "index offsets" : "positions", mine.size());
    }
    items.swap(mine);
    R.N = 1;
    // a rank's part of a region is a fraction of it: pieces small enough that the rank's decode | GPU | format pipeline still has a
    // few of them to overlap (a part of one piece would run its three stages one after the other)
    if (o.max_cnt >= 1000000) {
        int64_t widest = 0; for (const Work& w2 : items) if (w2.kind == WorkKind::Region) widest = std::max<int64_t>(widest, w2.end - w2.beg0);
        if (widest > 0 && widest < 4 * (int64_t)c.opt.chunk_bp) c.opt.chunk_bp = std::min<long long>(c.opt.chunk_bp, std::max<long long>(131072, ((widest / 4 + 65535) / 65536) * 65536));
    }
}

// the work is known: the sink and the inflater must be there, the engines get their share of the CPUs, long pieces their text buffers
static int settle_engines(Run& R) {
    Ctx& c = R.c; const Options& o = c.opt;
    if (R.def_thread.joinable()) { R.def_thread.join(); if (R.def_rc != 0) return R.leave(1); }      // no text is written before the sink exists (or the run ends: no return to plain text)
    if (R.inf_thread.joinable()) { R.inf_thread.join(); if (R.inf_rc != 0) return R.bail(1); }      // no reader starts before the inflater exists (or the run ends: no return to the host path)
    if (R.items.size() < R.N) R.N = std::max<size_t>(R.items.size(), 1);      // engines without work are never created
    if (R.N > 1) {    // the engines share this process's CPUs: each gets its part of the decode and formatter pools
        g_engines = (unsigned)R.N;
        c.opt.chunk_given = true;        // (the items ARE the pieces here: one brc_format_region per item, whose text stays in its engine's buffer)
        // (told to every engine with BRC_OPT_FORMAT_THREADS in make_engine — never through setenv(): the engine-creation
        // threads are inside the HIP runtime by now, which reads the environment while it starts, and a read of it racing a
        // setenv() that reallocates `environ` was a rare SIGSEGV before the first line of output)
        g_format_threads = std::max(2u, effective_cpus() / (unsigned)R.N);
        // engine 0 was created before the number of engines was known: it is told its share here, explicitly (the other
        // engines get theirs in make_engine) — not as a side effect of whoever waits for it next
        if (R.eng_ready.get() == 0) brc_set_option(c.eng, BRC_OPT_FORMAT_THREADS, (int64_t)g_format_threads.load());
    } else if (g_ranks > 1) {
        // a rank among others on this node: the engine's own pools (staging, formatter) get this rank's share of the CPUs too
        if (R.eng_ready.get() == 0) brc_set_option(c.eng, BRC_OPT_FORMAT_THREADS, (int64_t)std::max(2u, effective_cpus()));
    }
    // pin the text buffers of a long region's pieces while the first reads are being decoded
    int64_t widest = 0; for (const Work& w : R.items) if (w.kind == WorkKind::Region) widest = std::max<int64_t>(widest, std::min<int64_t>(w.end - w.beg0, auto_chunk(c, w.tid, w.beg0, w.end)));
    if (g_knobs.device_text && widest >= 100000 && g_knobs.pin_ahead) {
        const int64_t bytes = widest * (int64_t)(o.per_lib ? std::max<size_t>(c.libs.size(), 1) : 1) * 400;
        std::shared_future<int> eng_ready = R.eng_ready;
        R.pin_ahead = std::thread([&c, eng_ready, bytes]() { if (eng_ready.get() == 0) brc_set_option(c.eng, BRC_OPT_EXPECT_TEXT, bytes); });
    }
    return kGoOn;
}

// one engine: the items one after the other.  Site-list batches: the reads of batch k + 1 are fetched and decoded (a pool of BAM
// handles) while batch k is laid out, computed and printed
static int run_single(Run& R) {
    Ctx& c = R.c; std::vector<Work>& items = R.items;
    int ret = 0;
    std::unique_ptr<SiteFetch> ahead_f; std::thread ahead_t; size_t ahead_i = (size_t)-1;
    JoinOnExit join_ahead{ahead_t};
    for (size_t i = 0; i < items.size(); ++i) {
        Work& w = items[i];
        if (w.kind == WorkKind::Error) { fflush(stdout); fputs(w.err.c_str(), stderr); ret = 1; break; }
        if (w.kind == WorkKind::Message) { fflush(stdout); fputs(w.err.c_str(), stderr); continue; }
        if (w.kind == WorkKind::SiteBatch && g_knobs.site_ahead) {
            std::unique_ptr<SiteFetch> cur;
            const double w0 = now_s();
            if (ahead_i == i) { ahead_t.join(); cur = std::move(ahead_f); }
            else { cur.reset(new SiteFetch()); fetch_site_batch(c, w.sites, *cur); }
            c.t_site_fetch += now_s() - w0;
            if (i + 1 < items.size() && items[i + 1].kind == WorkKind::SiteBatch) {
                ahead_f.reset(new SiteFetch()); ahead_i = i + 1;
                SiteFetch* fp = ahead_f.get(); const std::vector<Site>* sp = &items[i + 1].sites; const Ctx* cp = &c;
                ahead_t = std::thread([cp, sp, fp]() { fetch_site_batch(*cp, *sp, *fp); });
            }
            if ((ret = run_site_batch(c, w.sites, cur.get()))) break;
            continue;
        }
        if ((ret = run_item(c, w))) break;
    }
    return ret;
}

// several engines, each with a worker thread, its own handles and its own GPU; this thread writes the items' text in file order
static int run_multi(Run& R) {
    Ctx& c = R.c; std::vector<Work>& items = R.items; const std::vector<int>& devices = R.devices; const size_t N = R.N;
    int ret = 0;
    // engine of every item: round robin, the first piece of a command-line region after the region before it
    int last_engine = -1; size_t rr = 0;
    for (Work& w : items) {
        if (w.kind == WorkKind::Region && w.keep_queue && last_engine >= 0) w.engine = last_engine;
        else w.engine = (int)(rr++ % N);
        if (w.kind == WorkKind::Region) last_engine = w.engine;
    }
    std::vector<std::unique_ptr<Ctx> > ctxs(N);
    std::mutex mu; std::condition_variable cv;
    size_t printed = 0; bool abort_all = false;
    int64_t gcount[BRC_N_WARN] = {0, 0, 0, 0};
    auto worker = [&](size_t g) {
        Ctx* wc = &c;
        if (g > 0) {                                                             // own handles, own engine
            ctxs[g].reset(new Ctx()); wc = ctxs[g].get(); wc->opt = c.opt;
            bool ok = open_inputs(*wc, true) && (wc->is_cram || wc->idx.load(c.opt.bam)) && make_engine(*wc, devices[g]) == 0 && (!c.opt.device_inflate || open_inflater(*wc, devices[g]) == 0);
            if (!ok) {
                std::lock_guard<std::mutex> lk(mu);
                for (Work& w : items) if ((size_t)w.engine == g && !w.done) { w.rc = 1; w.err = "bam-readcount: cannot set up the engine of GPU " + std::to_string(devices[g]) + "\n"; w.done = true; }
                cv.notify_all(); return;
            }
        }
        size_t held = (size_t)-1;                                               // item whose text sits in this engine's buffer
        wc->pre_format = [&]() {
            if (held == (size_t)-1) return;
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&]() { return abort_all || printed > held; });
            held = (size_t)-1;
        };
        for (size_t i = 0; i < items.size(); ++i) {
            Work& w = items[i];
            if ((size_t)w.engine != g) continue;
            {   // bound the text held in memory: stay within 2 N items of the one being written
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&]() { return abort_all || i < printed + 2 * N; });
                if (abort_all) return;
            }
            int r = w.rc;
            if (w.kind != WorkKind::Error && w.kind != WorkKind::Message) {
                wc->out_buf = &w.out; wc->err_buf = &w.err; wc->wev_buf = &w.wev;
                // (a piece is formatted by exactly one brc_format_region call: its text can stay where it is)
                const bool zc = w.kind == WorkKind::Region && w.end - w.beg0 <= (int64_t)c.opt.chunk_bp;
                wc->zc_parts = zc ? &w.parts : nullptr; wc->zc_lens = zc ? &w.lens : nullptr; wc->zc_n = zc ? &w.n_parts : nullptr;
                if (!zc) wc->pre_format();
                // the reads of this engine's next piece are fetched meanwhile (own handles: fetch_chunk only touches the
                // context's reader pool, which a single-piece item does not use after its own fetch)
                std::thread ahead;
                size_t j = i + 1;
                while (j < items.size() && (size_t)items[j].engine != g) ++j;
                if (zc && j < items.size() && items[j].kind == WorkKind::Region && !wc->is_cram) {
                    if (!wc->pf_buf) wc->pf_buf.reset(new Fetched());
                    const Work& nx = items[j];
                    const int64_t nb = std::min<int64_t>(nx.beg0 + (int64_t)c.opt.chunk_bp, nx.end);
                    if (!(wc->pf.valid && wc->pf.tid == nx.tid && wc->pf.a == nx.beg0 && wc->pf.b == nb)) {
                        Ctx* pc = wc; const int ntid = nx.tid; const int64_t na = nx.beg0;
                        // (started only after this item took its own prefetched reads: run_region swaps them out first thing)
                        wc->after_take = [pc, ntid, na, nb, &ahead]() { ahead = std::thread([pc, ntid, na, nb]() { fetch_chunk(*pc, ntid, na, nb, *pc->pf_buf); pc->pf.tid = ntid; pc->pf.a = na; pc->pf.b = nb; }); };
                    }
                }
                r = run_item(*wc, w);
                wc->after_take = nullptr;
                if (ahead.joinable()) { ahead.join(); wc->pf.valid = true; }
                if (zc && w.n_parts) held = i;
            }
            std::lock_guard<std::mutex> lk(mu);
            w.rc = r; w.done = true; cv.notify_all();
        }
    };
    std::vector<std::thread> th;
    for (size_t g = 0; g < N; ++g) th.emplace_back(worker, g);
    for (size_t i = 0; i < items.size(); ++i) {
        Work& w = items[i];
        { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&]() { return w.done; }); }
        if (!w.out.empty()) write_text(w.out.data(), w.out.size());
        if (w.n_parts) write_parts(w.parts, w.lens, w.n_parts);
        if (!w.wev.empty()) print_warn_events(w.wev.data(), w.wev.size(), c.opt.max_warnings, gcount, stderr);   // the global -w counters, in file order
        if (!w.err.empty()) fputs(w.err.c_str(), stderr);
        std::string().swap(w.out);
        { std::lock_guard<std::mutex> lk(mu); printed = i + 1; if (w.rc) { abort_all = true; ret = 1; } cv.notify_all(); }
        if (ret) break;
    }
    { std::lock_guard<std::mutex> lk(mu); abort_all = abort_all || ret != 0; printed = items.size(); cv.notify_all(); }
    for (std::thread& t : th) t.join();
    // (the process is about to end: see finish() for why the engines are only destroyed on request)
    for (size_t g = 1; g < N; ++g) if (ctxs[g]) { for (int w = 0; w < BRC_N_WARN; ++w) c.warn[w] += ctxs[g]->warn[w]; if (g_knobs.clean_exit) ctxs[g]->destroy_orderly(); }
    if (!g_knobs.clean_exit) for (auto& p : ctxs) (void)p.release();
    return ret;
}

// the last batch of the sink, and (BRC_CLI_TIMING) where the time went
static int report(Run& R, int ret) {
    Ctx& c = R.c; const bool timing = g_knobs.cli_timing;
    const std::string who = R.my_rank >= 0 ? "rank " + std::to_string(R.my_rank) + ": " : std::string();
    if (g_sink) {       // the last batch; the end-of-file member unless this is a rank (the coordinator writes it behind the last rank)
        g_sink->finish(R.my_rank < 0);
        if (g_sink->failed) { fprintf(stderr, "bam-readcount: --brc-bgzf-output: the deflater failed: %s\n", g_sink->err.c_str()); ret = 1; }
        if (timing) fprintf(stderr, "%sdevice deflate: %llu calls, %.1f MB in, %.1f MB out, %.3f s\n", who.c_str(), (unsigned long long)g_sink->calls, g_sink->bytes_in / 1e6, g_sink->bytes_out / 1e6, g_sink->seconds);
    }
    if (!timing) return ret;
    fprintf(stderr, "%sstartup: open inputs %.3f s, create engine %.3f s\n", who.c_str(), R.t_inputs - R.t_start, R.t_engine0 - R.t_inputs);
    fprintf(stderr, "%stiming: fetch+decode %.3f s, engine (push, upload, kernels, download) %.3f s, format %.3f s, write %.3f s\n", who.c_str(), c.t_fetch, c.t_engine, c.t_format, c.t_write);
    if (c.inf)
        fprintf(stderr, "%sdevice inflate: %llu calls, %.1f MB in, %.1f MB out, %.3f s inside the fetch threads\n", who.c_str(), (unsigned long long)c.inf->calls.load(), c.inf->bytes_in.load() / 1e6, c.inf->bytes_out.load() / 1e6, c.inf->nanos.load() * 1e-9);
    if (c.n_site_lines)
        fprintf(stderr, "%ssites: %llu lines in %llu clusters, %llu engine regions of %llu reads all told: waiting for indexed fetch + decode %.3f s (the fetches themselves, next batch behind the current one: %.3f s), layout on the virtual axis %.3f s, engine (push, upload, kernels, download) %.3f s, cutting the lines out + writing %.3f s\n",
                who.c_str(), (unsigned long long)c.n_site_lines, (unsigned long long)c.n_site_clusters, (unsigned long long)c.n_site_batches, (unsigned long long)c.n_site_reads, c.t_site_fetch, c.t_site_fetch_threads, c.t_site_layout, c.t_site_engine, c.t_site_format);
    return ret;
}

// Everything has been written.  Unpinning and freeing gigabytes of staging and the HIP runtime's own teardown only delay
// the exit of a process that is done: leave them to the operating system (BRC_CLEAN_EXIT=1 keeps the orderly path).
static int finish(Run& R, int ret) {
    fflush(stdout); fflush(stderr);
    R.leave(ret);
    // (a rank: whoever reads the run's stdout / stderr through a pipe sees its end when the last holder lets go — now, not when the kernel has
    // unpinned this process's gigabytes)
    if (R.my_rank >= 0 && !g_knobs.clean_exit) { close(1); close(2); }
    if (!g_knobs.clean_exit) _exit(ret);
    if (!R.wait_engine()) R.c.eng = nullptr;
    R.c.destroy_orderly();
    return ret;
}

int main(int argc, char** argv) {
    g_knobs = read_knobs();             // the environment, once, before the first thread
    install_crash_handler();
    Run R; std::string err;
    if (!parse_args(argc, argv, R.c.opt, &err)) { fprintf(stderr, "bam-readcount: %s\n", err.c_str()); return 1; }
    if (!rank_setup(R)) return 1;
    int rc = early_exit(R, argc, argv);
    if (rc == kGoOn) rc = open_run_inputs(R);
    if (rc != kGoOn) return rc;
    resolve_devices(R);
    start_background(R);
    // the work items, in file order
    R.atoms = R.my_rank >= 0 && R.n_ranks > 1;
    // (64 kb: four windows of the index; BRC_RANK_CUT: tests cut their kilobase contigs finer)
    R.rank_cut = R.c.opt.max_cnt < 1000000 ? (int64_t)INT_MAX : (int64_t)g_knobs.rank_cut;
    rc = R.c.opt.site_list.empty() ? items_from_regions(R) : items_from_site_list(R);
    if (rc != kGoOn) return rc;
    if (R.atoms) take_rank_slice(R);
    if ((rc = settle_engines(R)) != kGoOn) return rc;
    int ret = R.N == 1 ? run_single(R) : run_multi(R);
    ret = report(R, ret);
    return finish(R, ret);
}

// The program is compiled as ONE translation unit: a build rule names cli.cpp (with bamio.cpp and cram.cpp), as the rules of this
// program always have, and the other units come in here — so no rule, old or new, can link half a command line.  Every unit still
// compiles on its own against cli_internal.h (tests/sim/cli_check.cpp links three of them).
#include "cli_args.cpp"
#include "cli_output.cpp"
#include "cli_codec.cpp"
#include "cli_fetch.cpp"
#include "cli_pipeline.cpp"
#include "cli_ranks.cpp"
