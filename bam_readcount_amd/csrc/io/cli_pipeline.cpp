// cli_pipeline.cpp — a context at work: its inputs and its engine, a region through the three-stage pipeline (run_region), a batch
// of -l lines through the planner (run_site_batch).
#include <limits.h>

#include <algorithm>

#include "cli_internal.h"

std::atomic<unsigned> g_format_threads{0};   // formatter threads per engine when several engines share the process (0: the engine's default)

void Ctx::warn_events(const char* ev, size_t n) {
    if (!n) return;
    if (wev_buf) { wev_buf->append(ev, n); return; }
    if (tag_warnings) {
        for (size_t i = 0; i < n;) { size_t j = i; while (j < n && ev[j] != '\n') ++j; fputc(1, stderr); fwrite(ev + i, 1, j - i, stderr); fputc('\n', stderr); i = j + 1; }
        return;
    }
    print_warn_events(ev, n, opt.max_warnings, wcount, stderr);
}

void Ctx::emit_region(const char* const* parts, const size_t* lens, size_t n) {
    if (zc_parts) { *zc_parts = parts; *zc_lens = lens; *zc_n = n; return; }
    if (out_buf) { for (size_t i = 0; i < n; ++i) emit(parts[i], lens[i]); return; }
    write_parts(parts, lens, n);
}

void Ctx::destroy_orderly() {
    if (eng) { brc_destroy(eng); eng = nullptr; }
    if (inf) { bufs.clear(); pf_buf.reset(); if (inf->destroy) inf->destroy(inf->handle); delete inf; inf = nullptr; }      // (its readers first)
}

// this contig's reference bases, or say so (the reference dereferences a null pointer here)
static void load_contig(Ctx& c, int tid) {
    if (tid == c.ref_tid) return;
    const std::string& name = c.header().names[(size_t)tid];
    if (!c.fa.fetch(name, &c.ref)) { c.ref.clear(); fprintf(stderr, "bam-readcount: %s: no reference bases for %s\n", c.fa.error().c_str(), name.c_str()); }
    c.ref_tid = tid;
}

// nothing aligns past the contig (and a thousand bases of grace): the end of a window [beg0, end) on tid, never before its start
int64_t clamp_to_contig(const BamHeader& h, int tid, int64_t beg0, int64_t end) {
    const int64_t last = (int64_t)h.lengths[(size_t)tid] + 1000;
    if (end > last) end = last;
    return end < beg0 ? beg0 : end;
}

static int engine_failed(Ctx& c, int rc) {
    c.complain(std::string("bam-readcount: engine error: ") + brc_strerror(rc) + " (" + brc_last_error(c.eng) + ")\n");
    return 1;
}

// one reporting window [beg0,end) on tid: the body of the site-list / region loops (:588-605, :649-656)
// keep_queue: the first piece keeps the deletions the previous command-line region left pending (like the reference, :641-657)
// inner_piece: (several engines) this window is a piece of a longer region whose previous piece ran elsewhere
// The piece a long region is cut into, when the command line does not say (--brc-chunk): by the DATA under it, not by positions — about
// 26 MB of compressed records (200 000 reads of 150 bases), weighed by the index's file offsets (BamIndex::span_bytes): 1 Mbp of a 30x
// genome, 125 kb of a 200x tumour.  A piece sizes everything that is page-locked (decode arenas, staging, two text buffers — 1.4 GB per
// Mbp with four libraries) and the latency of the three-stage pipeline's first piece: BASELINE config 5 end to end went from 1.7 s at the
// fixed 1 Mbp to 0.93 s at 125 kb on the same box (profiles/r06_e2e_tumor_chunk_sweep.log), a third of it process exit (the kernel unpins
// what was pinned).  Multiples of 64 kb; never above the 1 Mbp that suits shallow data.
int64_t auto_chunk(const Ctx& c, int tid, int64_t beg0, int64_t end) {
    const int64_t max_chunk = (int64_t)c.opt.chunk_bp;
    if (c.opt.chunk_given || c.is_cram || end - beg0 < 2 * 65536 || c.opt.max_cnt < 1000000) return max_chunk;
    const double target = g_knobs.chunk_bytes;
    const double bytes = c.idx.span_bytes(tid, beg0, end);
    if (bytes <= 0) return max_chunk;
    const double per_bp = bytes / (double)(end - beg0);
    int64_t ch = (int64_t)(target / per_bp);
    ch = ((ch + 65535) / 65536) * 65536;
    if (ch < 65536) ch = 65536;
    return ch < max_chunk ? ch : max_chunk;
}

int run_region(Ctx& c, int tid, int64_t beg0, int64_t end, bool site_mode, bool keep_queue, bool inner_piece) {
    const BamHeader& h = c.header();
    if (c.have_fa) load_contig(c, tid);
    const char* ref = c.have_fa && !c.ref.empty() ? c.ref.data() : nullptr;
    end = clamp_to_contig(h, tid, beg0, end);
    // long regions are cut into abutting pieces; each piece fetches one base early exactly like the reference (:602).
    // The next `ahead` pieces are fetched and decoded in the background (each by its own pool of striped BAM handles)
    // while the current one is on the GPU / being formatted: decoding is the slowest of the three stages.
    const int64_t chunk = auto_chunk(c, tid, beg0, end);
    const int64_t npieces = std::max<int64_t>(1, (end - beg0 + chunk - 1) / chunk);
    const int ahead = g_knobs.fetch_ahead;
    std::vector<Fetched>& bufs = c.bufs; if (bufs.size() < (size_t)ahead + 1) bufs.resize((size_t)ahead + 1);
    std::vector<std::thread> fth((size_t)ahead + 1);
    for (Fetched& f : bufs) { if (npieces > (int64_t)ahead + 1) f.allow_pinned = true; }        // (only a run of pieces reuses its buffers)
    auto start_fetch = [&](int64_t j) {
        if (j >= npieces) return;
        const size_t slot = (size_t)(j % (ahead + 1));
        const int64_t fa = beg0 + j * chunk, fb = std::min<int64_t>(fa + chunk, end);
        fth[slot] = std::thread([&c, tid, fa, fb, &bufs, slot]() { fetch_chunk(c, tid, fa, fb, bufs[slot]); });
    };
    JoinOnExit join_all{fth};
    int64_t a = beg0;
    double t0 = now_s();
    if (c.pf.valid && c.pf.tid == tid && c.pf.a == a && c.pf.b == std::min<int64_t>(a + chunk, end)) std::swap(bufs[0], *c.pf_buf);   // fetched ahead by the worker
    else start_fetch(0);
    c.pf.valid = false;
    if (c.after_take) { if (fth[0].joinable()) fth[0].join(); c.after_take(); c.after_take = nullptr; }
    for (int64_t j = 1; j < ahead; ++j) start_fetch(j);
    c.t_fetch += now_s() - t0;
    // Two stages, one piece apart: while a helper thread formats and writes piece k (host planes of the last download),
    // this thread stages, uploads and computes piece k + 1 (staging and device buffers only); the download of k + 1 —
    // which overwrites the host planes — waits for the helper.  include/brc.h states this concurrency rule.
    brc_result res[2]; int slot = 0;
    std::thread fmt; int fmt_rc = 0; double fmt_s = 0;
    auto join_fmt = [&]() { if (fmt.joinable()) { fmt.join(); c.t_format += fmt_s; fmt_s = 0; } return fmt_rc; };
    int rc = 0;
    for (int64_t j = 0; j < npieces; ++j) {
        const int64_t b = std::min<int64_t>(a + chunk, end);
        const size_t cur = (size_t)(j % (ahead + 1));
        { const double w0 = now_s(); if (fth[cur].joinable()) fth[cur].join(); c.t_fetch += now_s() - w0; }   // only what the background fetch did not hide
        Fetched& F = bufs[cur];
        if (!F.ok) { join_fmt(); c.complain("bam-readcount: read error: " + F.err + "\n"); return 1; }
        double t1 = now_s();
        if (c.need_engine && !c.need_engine()) { join_fmt(); return 1; }
        rc = brc_begin_region(c.eng, tid, (int32_t)a, (int32_t)b, ref, (int64_t)c.ref.size());
        // (behind brc_begin_region: the buffer piece j - 1 has left may hold arenas the engine adopted — brc_push_reads_pinned —
        // which stay the engine's to read until this call)
        start_fetch(j + ahead);
        // the lines of a region piece are written on the GPU and come back as text (BRC_DEVICE_TEXT=0: host formatter)
        const bool dev_text = g_knobs.device_text;
        brc_set_option(c.eng, BRC_OPT_DEVICE_TEXT, dev_text ? 1 : 0);
        if (dev_text) brc_set_chrom(c.eng, h.names[(size_t)tid].c_str());
        {   // the stripes of a piece arrive as separate batches: tell the engine their total so it sizes its staging once
            size_t nr = 0, nq = 0; for (const Batcher& part : F.parts) { nr += part.pos.size(); nq += part.qual.size(); }
            brc_set_option(c.eng, BRC_OPT_EXPECT_READS, (int64_t)(nr + nr / 8)); brc_set_option(c.eng, BRC_OPT_EXPECT_BASES, (int64_t)(nq + nq / 8));
        }
        bool all_pinned = true;
        for (const Batcher& part : F.parts) if (!part.pos.empty() && !part.pinned) all_pinned = false;
        for (const Batcher& part : F.parts) {
            if (rc || part.pos.empty()) continue;
            const brc_read_batch v = part.view();
            rc = all_pinned ? brc_push_reads_pinned(c.eng, &v) : brc_push_reads(c.eng, &v);
        }
        if (!rc) rc = brc_upload(c.eng);
        if (!rc) rc = brc_compute(c.eng, nullptr);
        double t2 = now_s(); c.t_engine += t2 - t1;
        const int prev_rc = join_fmt();                       // piece k is out: its host planes may be overwritten
        double t3 = now_s(); c.t_write += t3 - t2;           // (time this thread waited for the formatter / writer)
        if (!rc && prev_rc) rc = prev_rc;
        brc_result& R = res[slot]; slot ^= 1;
        if (!rc && c.pre_format) c.pre_format();             // several engines: the writer is done with this engine's previous text
        if (!rc) rc = brc_fetch_result(c.eng, &R);
        c.t_engine += now_s() - t3;
        if (!rc) {
            // an internal piece boundary is not a region boundary: the deletions left pending by the previous piece start at
            // its last position, which is this piece's lead position and queues them again — drop the leftovers (the FIRST
            // piece keeps whatever the previous command-line region left, like the reference, :641-657)
            const bool clear_first = a == beg0 && !keep_queue;
            // a piece after the first continues the piece before it on this engine: its lead position is not processed again
            // and the deletion queues carry over.  (Set between the download of this piece and the download of the next:
            // the formatter thread and the warnings of THIS piece are its only readers.)
            brc_set_option(c.eng, BRC_OPT_CONTINUES_PREVIOUS, a > beg0 ? 1 : (inner_piece ? 2 : 0));
            const char* chrom = h.names[(size_t)tid].c_str();
            fmt_rc = 0;
            fmt = std::thread([&c, &R, chrom, clear_first, &fmt_rc, &fmt_s]() {
                const double f0 = now_s();
                if (clear_first) brc_clear_indel_queue(c.eng);
                const char* const* tparts = nullptr; const size_t* tlens = nullptr; size_t tn = 0;
                fmt_rc = brc_format_region_parts(c.eng, &R, chrom, &tparts, &tlens, &tn);
                if (!fmt_rc) c.emit_region(tparts, tlens, tn);
                fmt_s = now_s() - f0;
            });
            // (the warnings read the staged reads of this piece: before the next brc_begin_region)
            if (c.opt.max_warnings != 0) {
                const char* ev = ""; size_t evn = 0;
                if (brc_region_warnings(c.eng, chrom, c.opt.max_warnings, &ev, &evn) == 0) c.warn_events(ev, evn);
            }
            for (int w = 0; w < BRC_N_WARN; ++w) c.warn[w] += R.warn[w];
        }
        if (rc) { join_fmt(); return engine_failed(c, rc); }
        a = b;
    }
    if ((rc = join_fmt())) return engine_failed(c, rc);
    if (site_mode) brc_clear_indel_queue(c.eng);                                      // :605
    return 0;
}

// ---------------------------------------------------------------- site-list planner
// The reference runs every -l line as an independent fetch + pileup (bamreadcount.cpp:574-607).  Here a batch of lines is
// laid out side by side on one virtual coordinate axis: window i keeps its own reads (fetched exactly like the
// reference would, [beg0-1, end)), translated by delta_i, and its own slice of the reference; the engine runs ONE region
// over the whole axis, and each line's text is cut out of the shared planes with brc_format_window (fresh deletion
// queues, coordinates translated back).  Duplicate and overlapping lines stay exact because every window carries its own
// copy of its reads.  The indexed fetches of a batch run on a pool of threads, each with its own BAM handle (fetch_site_batch).

// pre: the batch's reads when they were fetched ahead (one engine: the main loop overlaps the next batch's fetch with this batch)
int run_site_batch(Ctx& c, const std::vector<Site>& sites, SiteFetch* pre) {
    const size_t n = sites.size();
    const BamHeader& h = c.header();
    SiteFetch own;
    if (!pre) { const double w0 = now_s(); fetch_site_batch(c, sites, own); pre = &own; c.t_site_fetch += now_s() - w0; }
    if (!pre->ok) { c.complain("bam-readcount: read error while fetching sites\n"); return 1; }
    std::vector<Batcher>& parts = pre->parts; const std::vector<int64_t>& lo = pre->lo; const std::vector<int64_t>& hi = pre->hi;
    c.t_site_fetch_threads += pre->seconds; c.n_site_lines += n; c.n_site_clusters += pre->n_clusters;
    // Virtual layout, in sub-batches: the engine keeps planes for every virtual position, and a window's extent is known
    // only now (it includes the overhang of its reads — with long reads far more than the line asked for), so the batch is
    // cut wherever the axis would outgrow the chunk size.  A window wider than that runs alone.
    // (BRC_PLAN_VMAX: tests force tiny sub-batches)
    const int64_t vmax = g_knobs.plan_vmax > 0 ? g_knobs.plan_vmax : std::max<int64_t>(4 * c.opt.chunk_bp, 1 << 20);
    std::vector<int64_t> delta(n);
    for (size_t i0 = 0; i0 < n;) {
        const double tl0 = now_s();
        int64_t V = 1; size_t i1 = i0;
        while (i1 < n && (i1 == i0 || V + (hi[i1] - lo[i1]) + 1 <= vmax)) { delta[i1] = V - lo[i1]; V += (hi[i1] - lo[i1]) + 1; ++i1; }
        if (V >= (int64_t)INT_MAX - 64) { c.complain("bam-readcount: a site-list window is too wide for the planner; rerun with --brc-plan 0\n"); return 1; }
        std::string vref;
        if (c.have_fa) vref.assign((size_t)V + 1, '\0');
        size_t nr = 0, nq = 0;
        for (size_t i = i0; i < i1; ++i) {
            const Site& st = sites[i];
            if (c.have_fa) {
                // The window's slice of the reference, read straight out of the mapped FASTA (Fasta::read_range): a whole-genome list
                // visits every contig, and loading each one whole (fai_fetch, as the reference does per -l line's contig) was a sixth of
                // the run.  Past the contig: the annotator stops at the terminating NUL (x == len, :151) but merely skips positions
                // x > len (site-list mode, :144-148); 'N' reproduces the skip (it never counts as a mismatch, :152).
                const int64_t x0 = std::max<int64_t>(lo[i], 0), x1 = hi[i];
                int64_t clen = 0;
                int64_t got = x1 > x0 ? c.fa.read_range(h.names[(size_t)st.tid], x0, x1 - x0, &vref[(size_t)(x0 + delta[i])], &clen) : 0;
                if (got < 0) {         // (no mapping / unknown contig: the whole contig, as before)
                    load_contig(c, st.tid);
                    clen = (int64_t)c.ref.size();
                    const int64_t xin = std::min(x1, clen);
                    if (xin > x0) memcpy(&vref[(size_t)(x0 + delta[i])], c.ref.data() + x0, (size_t)(xin - x0));
                }
                for (int64_t x = std::max(x0, clen); x < x1; ++x) vref[(size_t)(x + delta[i])] = x == clen ? '\0' : 'N';
            }
            // the line's reads move to its window of the virtual axis where they are (no second copy of the batch)
            Batcher& b = parts[i];
            for (size_t k = 0; k < b.pos.size(); ++k) b.pos[k] = (int32_t)(b.pos[k] + delta[i]);
            nr += b.pos.size(); nq += b.qual.size();
        }
        const double te0 = now_s(); c.t_site_layout += te0 - tl0; c.n_site_reads += nr; ++c.n_site_batches;
        if (c.need_engine && !c.need_engine()) return 1;
        brc_set_option(c.eng, BRC_OPT_DEVICE_TEXT, 0);           // windows are cut out of shared planes on the host
        int rc = brc_begin_region(c.eng, 0, 1, (int32_t)V, c.have_fa ? vref.data() : nullptr, V);
        brc_set_option(c.eng, BRC_OPT_EXPECT_READS, (int64_t)(nr + 16)); brc_set_option(c.eng, BRC_OPT_EXPECT_BASES, (int64_t)(nq + 16));
        for (size_t i = i0; i < i1 && !rc; ++i) {                // window by window, in axis order (= coordinate order)
            if (parts[i].pos.empty()) continue;
            const brc_read_batch v = parts[i].view();
            rc = brc_push_reads(c.eng, &v);
        }
        if (!rc) {         // only the lines' own positions are ever formatted: the engine need not pile up the rest of their reads' extent
            std::vector<int32_t> wb, we;
            for (size_t i = i0; i < i1; ++i) { wb.push_back((int32_t)(sites[i].beg0 + delta[i])); we.push_back((int32_t)(sites[i].end + delta[i])); }
            rc = brc_region_windows(c.eng, wb.data(), we.data(), (int64_t)wb.size());
        }
        brc_result res;
        if (!rc) rc = brc_end_region(c.eng, &res);
        if (rc) return engine_failed(c, rc);
        const double tf0 = now_s(); c.t_site_engine += tf0 - te0;
        for (size_t i = i0; i < i1; ++i) {
            const Site& st = sites[i];
            const char* text = ""; size_t len = 0;
            rc = brc_format_window(c.eng, &res, h.names[(size_t)st.tid].c_str(), (int32_t)(st.beg0 + delta[i]), (int32_t)(st.end + delta[i]), (int32_t)delta[i], &text, &len);
            if (rc) { c.complain(std::string("bam-readcount: engine error: ") + brc_strerror(rc) + "\n"); return 1; }
            c.emit(text, len);
            if (c.opt.max_warnings != 0) { const char* ev = ""; size_t evn = 0; if (brc_window_warnings(c.eng, (int32_t)(st.beg0 + delta[i]), (int32_t)(st.end + delta[i]), c.opt.max_warnings, &ev, &evn) == 0) c.warn_events(ev, evn); }
        }
        for (int w = 0; w < BRC_N_WARN; ++w) c.warn[w] += res.warn[w];
        c.t_site_format += now_s() - tf0;
        i0 = i1;
    }
    return 0;
}

bool open_inputs(Ctx& c, bool quiet) {
    const Options& o = c.opt;
    if (!o.fasta.empty()) {
        if (!c.fa.open(o.fasta)) { if (!quiet) fprintf(stderr, "Fail to open reference file %s\n", o.fasta.c_str()); return false; }
        c.have_fa = true;
    }
    c.is_cram = CramReader::is_cram(o.bam);
    if (c.is_cram ? !c.cram.open(o.bam, c.have_fa ? &c.fa : nullptr) : !c.bam.open(o.bam)) {                                               // :513-516
        if (!quiet) { fprintf(stderr, "Fail to open BAM file %s\n", o.bam.c_str()); if (c.is_cram) fprintf(stderr, "bam-readcount: %s\n", c.cram.error().c_str()); }
        return false;
    }
    c.libs = c.header().libraries();
    return true;
}

int make_engine(Ctx& c, int device) {
    const Options& o = c.opt;
    std::vector<const char*> names; for (const std::string& l : c.libs) names.push_back(l.c_str());
    brc_config cfg; memset(&cfg, 0, sizeof cfg);
    cfg.abi_version = BRC_ABI_VERSION; cfg.min_mapq = o.min_mapq; cfg.min_bq = o.min_bq; cfg.max_cnt = o.max_cnt;
    cfg.per_lib = o.per_lib; cfg.insertion_centric = o.insertion_centric; cfg.n_libs = (int32_t)names.size();
    cfg.lib_names = names.empty() ? nullptr : names.data(); cfg.device = device;
    cfg.ref_len_check = (!o.site_list.empty() && c.have_fa) ? 1 : 0;                                                                        // :594-600
    const int rc = brc_create(&cfg, &c.eng);
    if (rc == 0) brc_set_option(c.eng, BRC_OPT_TEXT_ONLY, 1);      // the command line only prints: no dense planes on the host
    if (rc == 0 && g_format_threads.load()) brc_set_option(c.eng, BRC_OPT_FORMAT_THREADS, (int64_t)g_format_threads.load());
    if (rc == 0 && o.max_cnt <= 0) brc_set_option(c.eng, BRC_OPT_MAX_COUNT, o.max_cnt);   // -d 0 / -d -3 reach the iterator as they are (:592,:651)
    return rc;
}
