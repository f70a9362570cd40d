// cli_output.cpp — what the command line writes: ReadWarnings' lines, and stdout either as plain text or through the BGZF sink.
#include <errno.h>
#include <sys/uio.h>

#include <algorithm>

#include "cli_internal.h"

// ReadWarnings::warn (src/lib/bamrc/ReadWarnings.hpp:39-50) over a tagged event stream of the engine (brc_region_warnings)
void print_warn_events(const char* ev, size_t n, long long max, int64_t* counts, FILE* fp) {
    static const char* const kMsg[BRC_N_WARN] = {
        "Couldn't find single-end mapping quality. Check to see if the SM tag is in BAM.",
        "Couldn't find number of mismatches. Check to see if the NM tag is in BAM.",
        "Couldn't find the generated tag.",
        "Library unavailable. Check to make sure the LB tag is present in the @RG entries of the header."};
    for (size_t i = 0; i < n;) {
        size_t j = i; while (j < n && ev[j] != '\n') ++j;
        const char* tp = strchr("SNZL", ev[i]);
        if (ev[i] == 'B') { if (j > i + 2) fwrite(ev + i + 2, 1, j - (i + 2), fp); fputc('\n', fp); }
        else if (tp && *tp && j >= i + 2) {
            const int t = (int)(tp - "SNZL");
            ++counts[t];
            if (!(max >= 0 && counts[t] > max)) {
                fputs("WARNING: In read ", fp); fwrite(ev + i + 2, 1, j - (i + 2), fp); fputs(": ", fp); fputs(kMsg[t], fp); fputc('\n', fp);
                if (max >= 0 && counts[t] == max) fprintf(fp, "The previous warning has been emitted %lld times and will be disabled.\n", (long long)counts[t]);
            }
        }
        i = j + 1;
    }
}

bool write_all(int fd, const char* p, size_t n) {
    while (n) { const ssize_t w = write(fd, p, n); if (w < 0) { if (errno == EINTR || errno == EAGAIN) continue; return false; } p += w; n -= (size_t)w; }
    return true;
}

// ---------------------------------------------------------------- the BGZF sink (cli_internal.h says what it is)
const unsigned char kBgzfEof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
BgzfSink* g_sink = nullptr;

// a closed pipe: like the reference, carry on silently; any other error (a full disk) is the run's: message and exit code 1
bool BgzfSink::write_fd(const char* p, size_t n) {
    while (n) {
        const ssize_t w = ::write(1, p, n);
        if (w < 0) {
            if (errno == EINTR) continue;
            if (errno == EAGAIN) { usleep(1000); continue; }
            if (errno != EPIPE && !failed) { failed = true; err = std::string("cannot write to stdout: ") + strerror(errno); }
            return false;
        }
        p += w; n -= (size_t)w;
    }
    return true;
}

void BgzfSink::run() {
    std::unique_lock<std::mutex> lk(mu);
    for (;;) {
        cv.wait(lk, [&]() { return pending >= 0 || stop; });
        if (pending < 0) return;
        const int b = pending;
        lk.unlock();
        const auto t0 = std::chrono::steady_clock::now();
        size_t got = 0, nm = 0;
        const int rc = failed ? 0 : deflate(handle, buf[b], fill[b], dst, dst_cap, &got, &nm);
        if (rc != 0) { failed = true; err = last_error ? last_error(handle) : ""; }
        else if (!failed) { write_fd(dst, got); ++calls; bytes_in += fill[b]; bytes_out += got; }
        seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        lk.lock();
        fill[b] = 0; pending = -1; cv.notify_all();
    }
}

void BgzfSink::hand_over() {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&]() { return pending < 0; });
    pending = cur; cur ^= 1; cv.notify_all();
}

void BgzfSink::write(const char* t, size_t n) {
    while (n) {
        const size_t k = std::min(n, batch - fill[cur]);
        memcpy(buf[cur] + fill[cur], t, k); fill[cur] += k; t += k; n -= k;
        if (fill[cur] == batch) hand_over();
    }
}

void BgzfSink::finish(bool eof) {
    if (finished) return;
    finished = true;
    if (fill[cur]) hand_over();
    { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&]() { return pending < 0; }); stop = true; cv.notify_all(); }
    if (worker.joinable()) worker.join();
    if (eof && !failed) write_fd((const char*)kBgzfEof, sizeof kBgzfEof);
}

void write_text(const char* t, size_t n) { if (g_sink) g_sink->write(t, n); else fwrite(t, 1, n, stdout); }

// Many pieces of text -> stdout with few system calls: a region's text arrives as thousands of pieces (the device's text
// between the lines the host rewrote); one write() each would cost more than producing them.
void write_parts(const char* const* parts, const size_t* lens, size_t n) {
    if (g_sink) { for (size_t i = 0; i < n; ++i) if (lens[i]) g_sink->write(parts[i], lens[i]); return; }
    fflush(stdout);
    const int fd = fileno(stdout);
    std::vector<struct iovec> iov; iov.reserve(1024);
    size_t i = 0;
    while (i < n) {
        iov.clear();
        for (; i < n && iov.size() < 1024; ++i) if (lens[i]) { struct iovec v; v.iov_base = (void*)parts[i]; v.iov_len = lens[i]; iov.push_back(v); }
        size_t k = 0;
        while (k < iov.size()) {
            const ssize_t w = writev(fd, iov.data() + k, (int)(iov.size() - k));
            if (w < 0) { if (errno == EINTR || errno == EAGAIN) continue; return; }     // (a closed pipe: like the reference, carry on silently)
            size_t left = (size_t)w;
            while (k < iov.size() && left >= iov[k].iov_len) { left -= iov[k].iov_len; ++k; }
            if (k < iov.size() && left) { iov[k].iov_base = (char*)iov[k].iov_base + left; iov[k].iov_len -= left; }
        }
    }
}
