// cli_internal.h — what the units of the `bam-readcount` command line share (cli.cpp says what the program is, and includes the others:
// a build rule compiles cli.cpp alone; every unit also compiles on its own against this header):
//   cli_args.cpp    options, the knob table (the environment, read once), the parsers of regions, -l lines and --brc-rank-of
//   cli_output.cpp  ReadWarnings' text, the BGZF sink, everything that writes stdout
//   cli_codec.cpp   the inflater and deflater libraries through dlopen
//   cli_fetch.cpp   reads of a region piece (striped) and of a batch of -l lines, in the engine's batch layout
//   cli_pipeline.cpp a context at work: inputs, engine, a region through the pipeline, a batch of -l lines through the planner
//   cli_ranks.cpp   --brc-ranks: the coordinating process, a rank's slice of the work and its share of the CPUs
//   cli.cpp         the work list, the schedulers, main; the one file a build rule names
#ifndef BRC_CLI_INTERNAL_H
#define BRC_CLI_INTERNAL_H
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/brc.h"
#include "bamio.h"

using namespace brcio;

// ---------------------------------------------------------------- cli_args.cpp
struct Options {
    bool help = false, version = false, per_lib = false, insertion_centric = false, distribution = false;
    unsigned seen = 0;                 // options given so far
    int min_mapq = 0, min_bq = 0, max_cnt = 10000000;
    long long max_warnings = -1;
    std::string site_list, fasta, bam;
    std::vector<std::string> regions;
    long long chunk_bp = 1000000;   // engine-side tiling of long regions (not a reference option): --brc-chunk
    bool chunk_given = false;       // ... given on the command line (else: sized by the data under a region, run_region: auto_chunk)
    long long plan_sites = 4096;    // site-list planner: -l lines batched per engine pass (0 = one pass per line): --brc-plan
    long long gpus = 1;             // GPUs: --brc-gpus
    long long streams = 0;          // engines per GPU (0: one; every engine already overlaps decode | GPU | format of consecutive pieces): --brc-streams
    long long ranks = 0;            // processes, one per GPU: --brc-ranks (BRC_RANKS)
    std::string rank_of;            // "r:N": this process IS rank r of N (what the coordinating process starts its children with): --brc-rank-of
    bool bgzf_output = false;       // stdout as BGZF members compressed by the deflater library (include/brc_deflate.h): --brc-bgzf-output (BRC_BGZF_OUTPUT=1)
    bool device_inflate = false;    // BGZF blocks inflated by the inflater library (include/brc_inflate.h): --brc-device-inflate (BRC_DEVICE_INFLATE=1)
    std::string tmpdir;             // where the ranks behind the first keep their text until its turn comes: --brc-tmpdir (TMPDIR, /tmp)
};
extern const char* const kUsage;
bool parse_args(int argc, char** argv, Options& o, std::string* err);

// Everything this program takes from the environment (DESIGN.md "The command line's knobs" is the table: name, rule, default).  Read
// ONCE, in main() before the first thread exists — the HIP runtime reads and the rank starter writes the environment, and a read
// racing a setenv() was a rare SIGSEGV here once — and only read afterwards.  Five rules:
struct Knobs {
    // off only if set and atoi == 0
    bool zero_copy = true, device_text = true, rank_narrow = true, rank_affinity = true, pin_ahead = true, site_ahead = true;
    // on if atoi != 0
    bool device_inflate = false, bgzf_output = false;
    // overrides if > 0 (fetch_threads, plan_vmax 0: the program's own choice)
    int fetch_threads = 0, fetch_ahead = 2;
    long long plan_vmax = 0, rank_cut = 65536;
    double chunk_bytes = 26.0e6;
    size_t bgzf_batch = (size_t)32 << 20;      // (kept within 64 KB .. 1 GB)
    // any value if set
    long long fetch_stripe_min = 65536, ranks = 0, streams = 1;
    bool has_device = false; int device = 0, rank_status_fd = -1;
    // presence only
    bool cli_timing = false, clean_exit = false;           // clean_exit: BRC_CLEAN_EXIT or BRC_ENGINE_TIMING
    // used as given if set, even if empty
    bool has_inflate_lib = false, has_deflate_lib = false; std::string inflate_lib, deflate_lib;
    std::string tmpdir;                        // TMPDIR: used if non-empty
    std::vector<int> devices;                  // BRC_DEVICES
    std::vector<std::string> visible;          // HIP_VISIBLE_DEVICES (set but empty: one empty entry)
    bool has_crash_dir = false; char crash_dir[512] = {0};      // BRC_CRASH_DIR, for the signal handler (which may not call getenv)
};
extern Knobs g_knobs;
Knobs read_knobs(const char* (*lookup)(const char*) = nullptr);      // nullptr: the process environment
bool parse_region(const BamHeader& h, const std::string& s, int* tid, int64_t* beg, int64_t* end, std::string* log);
bool parse_site_line(const char* p, size_t n, std::string* name, int* beg, int* end);
bool parse_rank_of(const std::string& v, int* r, int* n);

// ---------------------------------------------------------------- cli_output.cpp
inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
struct JoinOnExit {             // whoever leaves the scope early still joins its helpers
    std::thread* t; size_t n;
    explicit JoinOnExit(std::thread& one) : t(&one), n(1) {}
    explicit JoinOnExit(std::vector<std::thread>& many) : t(many.data()), n(many.size()) {}
    ~JoinOnExit() { for (size_t i = 0; i < n; ++i) if (t[i].joinable()) t[i].join(); }
};
void print_warn_events(const char* ev, size_t n, long long max, int64_t* counts, FILE* fp);
bool write_all(int fd, const char* p, size_t n);
extern const unsigned char kBgzfEof[28];
// --brc-bgzf-output: the one place stdout's bytes go when the switch is on.  Text is gathered in two page-locked buffers of one batch
// each; a full buffer is handed to the sink's own thread, which compresses it in one call of the deflater library (a batch is cut into
// members of 0xff00 input bytes from its start, so only a batch's last member is short) and writes the members, in order, while the
// caller fills the other buffer.  One caller at a time (the formatter thread of a region, else the main thread).
struct BgzfSink {
    void* handle = nullptr;
    int (*deflate)(void*, const void*, size_t, void*, size_t, size_t*, size_t*) = nullptr;
    const char* (*last_error)(const void*) = nullptr;
    size_t batch = (size_t)32 << 20;
    char* buf[2] = {nullptr, nullptr}; size_t fill[2] = {0, 0}; char* dst = nullptr; size_t dst_cap = 0;
    int cur = 0, pending = -1;              // the buffer being filled; the buffer the thread is compressing (-1: none)
    bool stop = false, failed = false, finished = false; std::string err;
    std::mutex mu; std::condition_variable cv; std::thread worker;
    uint64_t calls = 0, bytes_in = 0, bytes_out = 0; double seconds = 0;
    bool write_fd(const char* p, size_t n);
    void run();
    void hand_over();
    void write(const char* t, size_t n);
    void finish(bool eof);                  // the rest of the text, then (eof) the end-of-file member: once, whatever calls it again
};
extern BgzfSink* g_sink;                     // set before the first byte of text, never cleared
void write_text(const char* t, size_t n);   // to the sink, else to stdout
void write_parts(const char* const* parts, const size_t* lens, size_t n);

// ---------------------------------------------------------------- cli_fetch.cpp
// The two big arenas of a batch (SEQ, QUAL: 225 of the ~290 bytes of a 150-base read) can live in page-locked memory
// (brc_host_alloc): the engine then uploads them from where the decoder wrote them (brc_push_reads_pinned) instead of copying them
// into its own staging first — the copy was the longest stage of the engine thread.  A stateful allocator: `pinned` chooses.
template <class T> struct ArenaAlloc {
    typedef T value_type; typedef std::true_type propagate_on_container_copy_assignment; typedef std::true_type propagate_on_container_move_assignment; typedef std::true_type propagate_on_container_swap;
    bool pinned = false;
    ArenaAlloc() {}
    explicit ArenaAlloc(bool p) : pinned(p) {}
    template <class U> ArenaAlloc(const ArenaAlloc<U>& o) : pinned(o.pinned) {}
    // (a 16-byte header in front of every block says where it came from: when no more page-locked memory can be had a block comes from the
    // heap instead of failing the decode thread — hipMemcpyAsync takes pageable memory too, only slower)
    T* allocate(size_t n) {
        char* p = pinned ? (char*)brc_host_alloc(n * sizeof(T) + 16) : nullptr; uint64_t tag = 1;
        if (!p) { p = (char*)malloc(n * sizeof(T) + 16); tag = 0; }
        if (!p) throw std::bad_alloc();
        memcpy(p, &tag, sizeof tag);
        return (T*)(p + 16);
    }
    void deallocate(T* q, size_t) { char* p = (char*)q - 16; uint64_t tag; memcpy(&tag, p, sizeof tag); if (tag) brc_host_free(p); else free(p); }
    template <class U> bool operator==(const ArenaAlloc<U>& o) const { return pinned == o.pinned; }
    template <class U> bool operator!=(const ArenaAlloc<U>& o) const { return pinned != o.pinned; }
};
typedef std::vector<uint8_t, ArenaAlloc<uint8_t> > ArenaVec;

// SoA batch in the brc_read_batch layout
struct Batcher {
    std::vector<int32_t> pos, l_qseq, nm, sm; std::vector<uint16_t> flag; std::vector<uint8_t> mapq, tags;
    std::vector<int16_t> lib; std::vector<uint32_t> n_cigar, cigar; std::vector<uint64_t> cig_off, seq_off, qual_off;
    ArenaVec seq4, qual;
    bool pinned = false; size_t seen_seq = 0, seen_qual = 0;       // arenas in page-locked memory; the largest fills seen so far (what a pinned arena is sized by)
    std::vector<char> names; std::vector<size_t> name_off; mutable std::vector<const char*> name_ptr;   // read names (warning text)
    bool keep_names = true;           // -w 0: no warning text will ever be printed
    void use_pinned();
    void clear();
    void add(const BamRecord& r, int lib_index);
    brc_read_batch view() const;
};

// Reads of one chunk [a-1, b) (the reference's own fetch rule, :602), decoded by a pool of BAM handles: see fetch_chunk
struct Fetched { std::vector<Batcher> parts; bool ok = true; std::string err; unsigned uses = 0; bool allow_pinned = false;
                 std::vector<std::unique_ptr<BamReader> > pool;      // the BAM handles of this buffer's stripes (fetches of different buffers run side by side)
                 std::vector<std::unique_ptr<CramReader> > cram_pool; };   // ... or its CRAM readers

struct Site { int tid; int64_t beg0, end; };
// the indexed fetches of one batch of lines: every line's own reads (exactly what samfetch would hand over for [beg0 - 1, end))
// and the extent they span.  Reads only what never changes while the run lasts (options, index, header, libraries), so the
// fetch of the NEXT batch runs on threads of its own while this batch is laid out, computed and printed.
struct SiteFetch { std::vector<Batcher> parts; std::vector<int64_t> lo, hi; bool ok = true; size_t n_clusters = 0; double seconds = 0; };

// One set of inputs and one engine (cli.cpp; the fetches read its inputs)
struct Ctx {
    double t_fetch = 0, t_engine = 0, t_format = 0, t_write = 0;   // BRC_CLI_TIMING=1 prints them on stderr
    double t_site_fetch = 0, t_site_fetch_threads = 0, t_site_layout = 0, t_site_engine = 0, t_site_format = 0; uint64_t n_site_lines = 0, n_site_clusters = 0, n_site_reads = 0, n_site_batches = 0;   // the site-list planner's own account
    Options opt; BamReader bam; BamIndex idx; Fasta fa; bool have_fa = false;
    CramReader cram; bool is_cram = false;          // CRAM 3.0 input (cram.cpp); region queries go through the .crai or one walk over the container headers
    const BamHeader& header() const { return is_cram ? cram.header() : bam.header(); }
    brc_engine* eng = nullptr;
    ExtInflater* inf = nullptr;             // --brc-device-inflate: this context's inflater (its GPU's); destroyed on the orderly exit path (BRC_CLEAN_EXIT)
    std::vector<std::string> libs;
    int ref_tid = -1; std::string ref;      // currently loaded contig (load_reference, :83-90)
    Batcher batch;
    uint64_t warn[BRC_N_WARN] = {0, 0, 0, 0};
    // where a work item's text goes: straight to stdout / stderr (one engine), or into the item's buffers (several engines:
    // the main thread writes them in file order)
    std::string* out_buf = nullptr; std::string* err_buf = nullptr;
    std::string* wev_buf = nullptr;       // tagged warning events of the item (several engines) — else they are printed at once
    int64_t wcount[BRC_N_WARN] = {0, 0, 0, 0};   // ReadWarnings' counters (the main context's are the global ones)
    // a rank behind the first: its warning events travel to the coordinating process as they are, one per stderr line behind a
    // 0x01 byte — ReadWarnings' counters are global (-w caps every type across the whole run), so the process that sees the
    // ranks' streams in file order applies them
    bool tag_warnings = false;
    void warn_events(const char* ev, size_t n);
    void emit(const char* t, size_t n) { if (!n) return; if (out_buf) out_buf->append(t, n); else write_text(t, n); }
    // several engines, region pieces: the text stays in the engine's buffer (no copy of hundreds of megabytes per piece);
    // the main thread writes it from there, and this engine's next format call waits for that (pre_format)
    std::function<bool()> need_engine;      // the first context's engine is created in the background: wait for it (false: it failed)
    std::function<void()> pre_format;
    std::function<void()> after_take;       // run once the piece has taken its reads (the worker starts the next fetch then)
    const char* const** zc_parts = nullptr; const size_t** zc_lens = nullptr; size_t* zc_n = nullptr;
    void emit_region(const char* const* parts, const size_t* lens, size_t n);
    // several engines: the reads of this engine's next piece, fetched while the current piece is on the GPU / being formatted
    struct Prefetch { bool valid = false; int tid = 0; int64_t a = 0, b = 0; } pf;
    std::unique_ptr<Fetched> pf_buf;
    // run_region's fetch buffers.  They outlive the call: the engine may still hold pointers into the page-locked arenas of the last piece
    // it adopted (brc_push_reads_pinned: valid until the next brc_begin_region or brc_destroy, include/brc.h), and the next region finds
    // its handles open and its arenas pinned
    std::vector<Fetched> bufs;
    void complain(const std::string& m) { if (err_buf) err_buf->append(m); else fputs(m.c_str(), stderr); }
    // the engine and the inflater given back in order (its readers first): only where the run asks for it (BRC_CLEAN_EXIT), see finish()
    void destroy_orderly();
};
void fetch_chunk(Ctx& c, int tid, int64_t a, int64_t b, Fetched& out);
void fetch_site_batch(const Ctx& c, const std::vector<Site>& sites, SiteFetch& F);

// ---------------------------------------------------------------- cli_pipeline.cpp
extern std::atomic<unsigned> g_format_threads;   // formatter threads per engine when several engines share the process (0: the engine's default)
bool open_inputs(Ctx& c, bool quiet);
int make_engine(Ctx& c, int device);
int64_t clamp_to_contig(const BamHeader& h, int tid, int64_t beg0, int64_t end);
int64_t auto_chunk(const Ctx& c, int tid, int64_t beg0, int64_t end);
int run_region(Ctx& c, int tid, int64_t beg0, int64_t end, bool site_mode, bool keep_queue = true, bool inner_piece = false);
int run_site_batch(Ctx& c, const std::vector<Site>& sites, SiteFetch* pre = nullptr);

// ---------------------------------------------------------------- cli_codec.cpp
int open_inflater(Ctx& c, int device);      // --brc-device-inflate: c.inf, or a message and 1
int open_bgzf_sink(int device);             // --brc-bgzf-output: g_sink, or a message and 1

// ---------------------------------------------------------------- cli_ranks.cpp
extern unsigned g_engines;                  // engines of this process (they share the CPUs)
extern unsigned g_ranks;                    // --brc-ranks: processes side by side on this node; each sizes its pools by its share of the CPUs (set before the first effective_cpus())
unsigned effective_cpus();
void bind_rank_cpus(int rank, int n_ranks);
int coordinate(int argc, char** argv, const Options& o, int N);
void rank_slice(const std::vector<double>& w, int r, int n, size_t* lo, size_t* hi);
#endif
