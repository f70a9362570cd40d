// cli_ranks.cpp — ranks: one process per GPU
// `bam-readcount --brc-ranks N ...` (or BRC_RANKS=N): this process becomes the COORDINATOR.  It never touches the HIP runtime: it
// starts N copies of itself (`--brc-rank-of r:N`), each a fresh process that binds to one GPU (BRC_DEVICES=a,b,.. names them, default
// 0..N-1; the child sees only its own through HIP_VISIBLE_DEVICES) and to its share of the CPUs, builds the same work list from the
// same files, cuts it — in FILE ORDER — into N contiguous slices of near-equal estimated work (the index's file offsets per 16-kb
// window: BamIndex::span_bytes) and runs its own slice exactly like a single process would.  No data-path exchange: a line depends on
// nothing but the reads over its position (and the position before it, which every piece fetches itself, bamreadcount.cpp:602);
// overlapping and repeated -l lines are printed as often as the list names them (:574-608), the deletion queue is cleared per line
// (:605).  Rank 0 writes to this process's stdout and stderr directly; the ranks behind it write into unlinked temporary files
// (--brc-tmpdir, TMPDIR, /tmp) which the coordinator copies to stdout in rank order, following rank r's file while it is still being
// written once the ranks before it are done (stdout /dev/null: they write there themselves).  stderr of those ranks arrives line by
// line, warning events tagged so that ReadWarnings' -w counters run over the whole run in file order.  A rank that fails ends the run
// where the reference would have stopped: the text of the ranks before it is out, the ranks behind it are stopped and their text dropped.
// Several command-line regions in one run stay one process: a deletion left pending by one region can hold back the deletions of every
// region behind it (the reference does not clear its queue there, :641-657), which only a process that has seen them all can know.
#include <errno.h>
#include <poll.h>
#include <sched.h>
#include <signal.h>
#include <sys/sendfile.h>
#include <sys/stat.h>
#include <sys/sysmacros.h>
#include <sys/wait.h>

#include <algorithm>

#include "cli_internal.h"

// CPUs this process may really use at once: hardware threads capped by a cgroup CPU quota (a container with 16 CPUs of
// quota on a 256-thread host is throttled for most of every period if its pools are sized by the hardware)
unsigned g_engines = 1;
unsigned g_ranks = 1;
unsigned effective_cpus() {
    // (worker threads call this: a function-local static is initialised once, thread-safely)
    static const unsigned cached = []() -> unsigned {
        unsigned n = std::thread::hardware_concurrency(); if (n == 0) n = 1;
        double quota = 0;
        if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
            char q[64]; long long per = 0;
            if (fscanf(f, "%63s %lld", q, &per) == 2 && strcmp(q, "max") != 0 && per > 0) quota = atof(q) / (double)per;
            fclose(f);
        } else {
            long long q = -1, per = 0;
            if (FILE* g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) { if (fscanf(g, "%lld", &q) != 1) q = -1; fclose(g); }
            if (FILE* g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (fscanf(g, "%lld", &per) != 1) per = 0; fclose(g); }
            if (q > 0 && per > 0) quota = (double)q / (double)per;
        }
        if (quota > 0 && quota < (double)n) n = (unsigned)(quota + 0.999);
        if (g_ranks > 1) n = (n + g_ranks - 1) / g_ranks;              // one rank's share
        return n < 1 ? 1u : n;
    }();
    return cached;
}

// this rank's share of the CPUs, as a contiguous slice of the ones the group may use (BRC_RANK_AFFINITY=0: left to the scheduler)
void bind_rank_cpus(int rank, int n_ranks) {
    cpu_set_t all; CPU_ZERO(&all);
    if (sched_getaffinity(0, sizeof all, &all) != 0) return;
    std::vector<int> cpus; for (int k = 0; k < CPU_SETSIZE; ++k) if (CPU_ISSET(k, &all)) cpus.push_back(k);
    if ((int)cpus.size() < n_ranks) return;
    cpu_set_t mine; CPU_ZERO(&mine);
    const size_t a = cpus.size() * (size_t)rank / (size_t)n_ranks, b = cpus.size() * (size_t)(rank + 1) / (size_t)n_ranks;
    for (size_t k = a; k < b; ++k) CPU_SET(cpus[k], &mine);
    (void)sched_setaffinity(0, sizeof mine, &mine);
}

// ---------------------------------------------------------------- the coordinator
// A rank is DONE when it has written its last word to the status pipe (it flushes its text and its stderr first) — or when the pipe
// closes without one (it died).  The process itself may take a good while longer to disappear: a rank that printed gigabytes holds as
// many gigabytes of page-locked buffers, which the kernel unpins at exit (0.5-0.7 s for BASELINE config 5's share) — nothing this run has
// to wait for: the coordinator goes on to the next rank's text, and leaves when the last rank is done.
struct Child { pid_t pid = -1; int out = -1, err = -1, status = -1; bool reaped = false; int wstatus = 0;
               std::string status_line; bool status_eof = false; double secs = 0, done_at = 0; };
struct Group {
    Group(const Options& opt, int n) : o(opt), N(n) {}
    const Options& o; int N; bool to_null = false; std::string tdir;
    std::vector<Child> ch;
    std::vector<char> buf;
    bool text_out = false;                          // some rank has (or may have) written text: rank 0 ended well, or a later rank's bytes were copied
    int64_t gcount[BRC_N_WARN] = {0, 0, 0, 0};
};

static bool reap(Child& c, bool block) {
    if (c.reaped) return true;
    const pid_t w = waitpid(c.pid, &c.wstatus, block ? 0 : WNOHANG);
    if (w == c.pid) c.reaped = true;
    return c.reaped;
}

// every rank as a fresh image of this program: its text and stderr where the coordinator will look for them, its GPU, its status pipe
static int start_ranks(Group& g, int argc, char** argv) {
    const int N = g.N;
    // GPUs of the ranks
    std::vector<int> devs = g_knobs.devices;
    if (devs.empty()) for (int d = 0; d < N; ++d) devs.push_back(d);
    const std::vector<std::string>& visible = g_knobs.visible;               // the caller's own HIP_VISIBLE_DEVICES: rank r's GPU is the devs[r]-th entry of it
    const bool narrow = g_knobs.rank_narrow;
    auto tmpfd = [&]() -> int {
        std::string path = g.tdir + "/brc_rank_XXXXXX";
        std::vector<char> b(path.begin(), path.end()); b.push_back(0);
        const int fd = mkstemp(b.data());
        if (fd >= 0) unlink(b.data());
        return fd;
    };
    std::vector<Child>& ch = g.ch;
    fflush(stdout); fflush(stderr);
    for (int r = 0; r < N; ++r) {
        Child& c = ch[(size_t)r];
        int sp[2];
        if (pipe(sp) != 0) { fprintf(stderr, "bam-readcount: cannot create a pipe for rank %d: %s\n", r, strerror(errno)); return 1; }
        if (r > 0) {
            if (!g.to_null) { c.out = tmpfd(); if (c.out < 0) { fprintf(stderr, "bam-readcount: cannot create a temporary file in %s for the text of rank %d: %s (--brc-tmpdir)\n", g.tdir.c_str(), r, strerror(errno)); return 1; } }
            c.err = tmpfd(); if (c.err < 0) { fprintf(stderr, "bam-readcount: cannot create a temporary file in %s: %s (--brc-tmpdir)\n", g.tdir.c_str(), strerror(errno)); return 1; }
        }
        const pid_t pid = fork();
        if (pid < 0) { fprintf(stderr, "bam-readcount: cannot start rank %d: %s\n", r, strerror(errno)); return 1; }
        if (pid == 0) {
            // the child: its text and stderr where the coordinator will look for them, its GPU, then a fresh image of this program
            close(sp[0]);
            if (r > 0) {
                if (c.out >= 0) dup2(c.out, 1);
                dup2(c.err, 2);
            }
            for (int k = 0; k < r; ++k) { if (ch[(size_t)k].status >= 0) close(ch[(size_t)k].status); }
            const int dev = devs[(size_t)r % devs.size()];
            char b[64];
            if (narrow) {
                if (!visible.empty()) { if ((size_t)dev < visible.size()) setenv("HIP_VISIBLE_DEVICES", visible[(size_t)dev].c_str(), 1); }
                else { snprintf(b, sizeof b, "%d", dev); setenv("HIP_VISIBLE_DEVICES", b, 1); }
                setenv("BRC_DEVICE", "0", 1);
            } else { snprintf(b, sizeof b, "%d", dev); setenv("BRC_DEVICE", b, 1); }
            unsetenv("BRC_DEVICES"); unsetenv("BRC_RANKS");
            snprintf(b, sizeof b, "%d", sp[1]); setenv("BRC_RANK_STATUS_FD", b, 1);
            std::vector<char*> av;
            av.push_back(argv[0]);
            std::string ro = "--brc-rank-of=" + std::to_string(r) + ":" + std::to_string(N);
            av.push_back(&ro[0]);
            for (int i = 1; i < argc; ++i) av.push_back(argv[i]);
            av.push_back(nullptr);
            execv("/proc/self/exe", av.data());
            execvp(argv[0], av.data());
            fprintf(stderr, "bam-readcount: cannot start rank %d: %s\n", r, strerror(errno));
            _exit(127);
        }
        close(sp[1]);
        c.pid = pid; c.status = sp[0];
    }
    return 0;
}

static bool poll_status(Child& c, int timeout_ms) {         // true: the rank has said its last word (or will never)
    if (c.status_eof) return true;
    for (;;) {
        struct pollfd pf; pf.fd = c.status; pf.events = POLLIN; pf.revents = 0;
        const int pr = poll(&pf, 1, timeout_ms);
        if (pr < 0 && errno == EINTR) continue;
        if (pr <= 0) return false;
        char b[256]; const ssize_t g = read(c.status, b, sizeof b);
        if (g < 0 && (errno == EINTR || errno == EAGAIN)) continue;
        if (g <= 0) { c.status_eof = true; return true; }
        c.status_line.append(b, (size_t)g);
        if (c.status_line.find('\n') != std::string::npos) { c.status_eof = true; return true; }
        timeout_ms = 0;
    }
}

// follow the rank's text: copy what is there, look whether the rank is done, copy the rest
static void follow_text(Group& g, Child& c) {
    std::vector<char>& buf = g.buf;
    off_t off = 0; bool use_sendfile = true;
    for (;;) {
        const bool finished = poll_status(c, 0);
        struct stat fs; if (fstat(c.out, &fs) != 0) break;
        bool moved = false;
        while (off < fs.st_size) {
            ssize_t w = -1;
            if (use_sendfile) { w = sendfile(1, c.out, &off, (size_t)std::min<off_t>(fs.st_size - off, (off_t)1 << 30)); if (w < 0 && (errno == EINVAL || errno == ENOSYS)) use_sendfile = false; else if (w < 0 && (errno == EINTR || errno == EAGAIN)) continue; else if (w < 0) { off = fs.st_size; break; } }
            if (!use_sendfile) {
                const ssize_t got = pread(c.out, buf.data(), (size_t)std::min<off_t>(fs.st_size - off, (off_t)buf.size()), off);
                if (got <= 0) { if (got < 0 && errno == EINTR) continue; off = fs.st_size; break; }
                if (!write_all(1, buf.data(), (size_t)got)) { off = fs.st_size; break; }     // (a closed pipe: like the reference, carry on silently)
                off += got;
            }
            moved = true; g.text_out = true;
        }
        if (finished) { struct stat f2; if (fstat(c.out, &f2) == 0 && f2.st_size > off) continue; break; }
        if (!moved) poll_status(c, 1);
    }
}

// what the rank said when it ended: exit code, ReadWarnings' counters (rank 0 printed its own warnings), seconds
static int read_status(Group& g, int r) {
    Child& c = g.ch[(size_t)r];
    long long w[BRC_N_WARN] = {0, 0, 0, 0}; int src = 1, wrote = 0; double s = 0;
    if (sscanf(c.status_line.c_str(), "%d %lld %lld %lld %lld %lf %d", &src, &w[0], &w[1], &w[2], &w[3], &s, &wrote) >= 6) { if (wrote) g.text_out = true; c.secs = s; if (r == 0) for (int k = 0; k < BRC_N_WARN; ++k) g.gcount[k] = w[k]; return src; }
    reap(c, true);           // (a rank that ended without a word did not end well: wait for it, say how it went)
    return WIFEXITED(c.wstatus) && WEXITSTATUS(c.wstatus) ? WEXITSTATUS(c.wstatus) : 1;
}

// its stderr, in order: plain lines as they are, tagged warning events through the run's counters
static void replay_stderr(Group& g, Child& c) {
    std::vector<char>& buf = g.buf;
    fflush(stdout);
    std::string all; ssize_t got; off_t eo = 0;
    while ((got = pread(c.err, buf.data(), buf.size(), eo)) > 0 || (got < 0 && errno == EINTR)) if (got > 0) { all.append(buf.data(), (size_t)got); eo += got; }
    for (size_t i = 0; i < all.size();) {
        size_t j = i; while (j < all.size() && all[j] != '\n') ++j;
        if (all[i] == 1) { std::string ev(all, i + 1, j - (i + 1)); ev.push_back('\n'); print_warn_events(ev.data(), ev.size(), g.o.max_warnings, g.gcount, stderr); }
        else { fwrite(all.data() + i, 1, j - i, stderr); if (j < all.size()) fputc('\n', stderr); }
        i = j + 1;
    }
}

int coordinate(int argc, char** argv, const Options& o, int N) {
    const double t0 = now_s();
    Group g(o, N);
    struct stat st; g.to_null = fstat(1, &st) == 0 && S_ISCHR(st.st_mode) && major(st.st_rdev) == 1 && minor(st.st_rdev) == 3;
    g.tdir = !o.tmpdir.empty() ? o.tmpdir : (!g_knobs.tmpdir.empty() ? g_knobs.tmpdir : "/tmp");
    g.ch.resize((size_t)N); g.buf.resize((size_t)1 << 20);
    if (start_ranks(g, argc, argv)) return 1;
    int ret = 0;
    for (int r = 0; r < N && !ret; ++r) {
        Child& c = g.ch[(size_t)r];
        if (r > 0 && c.out >= 0) follow_text(g, c);
        while (!poll_status(c, 1000)) {}
        c.done_at = now_s() - t0;
        const int rc = read_status(g, r);
        if (r > 0) replay_stderr(g, c);
        if (rc) ret = rc == 127 ? 1 : rc;
        else if (r == 0) g.text_out = true;
        if (c.reaped && WIFSIGNALED(c.wstatus)) { ret = 1; fprintf(stderr, "bam-readcount: rank %d ended on signal %d\n", r, WTERMSIG(c.wstatus)); }
    }
    // a failed run: the ranks behind the failure are stopped, their text is dropped.  (Ranks that are done are not waited for: see above.)
    if (ret) { for (Child& c : g.ch) if (!c.reaped && !c.status_eof) kill(c.pid, SIGTERM); }
    for (Child& c : g.ch) reap(c, false);
    if (g_knobs.cli_timing) {
        fprintf(stderr, "ranks: %d processes", N);
        for (int r = 0; r < N; ++r) fprintf(stderr, "%s rank %d: %.3f s (its text was out after %.3f s)", r ? ";" : ":", r, g.ch[(size_t)r].secs, g.ch[(size_t)r].done_at);
        fprintf(stderr, "; all told %.3f s\n", now_s() - t0);
    }
    fflush(stdout); fflush(stderr);
    // --brc-bgzf-output: the ranks wrote members and no end-of-file member; it follows the last rank's bytes, once
    // (a run whose first rank failed before any text — no deflater to be had — leaves stdout empty)
    if (!g.to_null && (ret == 0 || g.text_out) && (o.bgzf_output || g_knobs.bgzf_output)) write_all(1, (const char*)kBgzfEof, sizeof kBgzfEof);
    return ret;
}

// the slice of `atoms` that rank r of n owns: contiguous, order-preserving, balanced by weight — shard.partition's rule (the atom that
// crosses the r-th boundary goes to whichever side leaves the smaller excess)
void rank_slice(const std::vector<double>& w, int r, int n, size_t* lo, size_t* hi) {
    const size_t m = w.size();
    std::vector<double> cum(m); double t = 0; for (size_t i = 0; i < m; ++i) { t += w[i] > 1e-9 ? w[i] : 1e-9; cum[i] = t; }
    size_t start = 0, stop = 0;
    for (int k = 0; k <= r; ++k) {
        start = stop;
        if (k + 1 < n) {
            const double target = t * (double)(k + 1) / (double)n;
            stop = (size_t)(std::upper_bound(cum.begin(), cum.end(), target) - cum.begin());
            if (stop < m && stop >= start && (cum[stop] - target) < (target - (stop > 0 ? cum[stop - 1] : 0.0))) ++stop;
        } else stop = m;
        if (stop < start) stop = start;
        if (stop > m) stop = m;
    }
    *lo = start; *hi = stop;
}
