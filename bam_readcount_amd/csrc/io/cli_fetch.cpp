// cli_fetch.cpp — reads from the input file into the engine's batch layout: a region piece by a pool of striped readers (fetch_chunk),
// a batch of -l lines by clustered indexed fetches (fetch_site_batch).
#include <algorithm>
#include <atomic>

#include "cli_internal.h"

// from now on this batch's arenas are page-locked, with room for what it held before and a quarter more (an allocation of
// page-locked memory costs milliseconds: once per buffer, not once per growth step)
void Batcher::use_pinned() {
    if (pinned) return;
    try {
        ArenaVec s2{ArenaAlloc<uint8_t>(true)}, q2{ArenaAlloc<uint8_t>(true)};
        s2.reserve(seen_seq + seen_seq / 4 + 4096); q2.reserve(seen_qual + seen_qual / 4 + 4096);
        seq4.swap(s2); qual.swap(q2); pinned = true;
    } catch (...) { pinned = false; }                            // (no page-locked memory to be had: the copying path stays)
}

void Batcher::clear() { seen_seq = std::max(seen_seq, seq4.size()); seen_qual = std::max(seen_qual, qual.size()); names.clear(); name_off.clear(); pos.clear(); l_qseq.clear(); nm.clear(); sm.clear(); flag.clear(); mapq.clear(); tags.clear(); lib.clear(); n_cigar.clear(); cigar.clear(); cig_off.clear(); seq_off.clear(); qual_off.clear(); seq4.clear(); qual.clear(); }

void Batcher::add(const BamRecord& r, int lib_index) {
    pos.push_back(r.pos); flag.push_back(r.flag); mapq.push_back(r.mapq); l_qseq.push_back(r.l_seq); n_cigar.push_back(r.n_cigar);
    lib.push_back((int16_t)lib_index);
    cig_off.push_back(cigar.size()); seq_off.push_back(seq4.size()); qual_off.push_back(qual.size());
    const uint32_t* c = r.cigar(); cigar.insert(cigar.end(), c, c + r.n_cigar);
    seq4.insert(seq4.end(), r.seq(), r.seq() + (r.l_seq + 1) / 2);
    qual.insert(qual.end(), r.qual(), r.qual() + r.l_seq);
    uint8_t t = 0; int32_t vnm = 0, vsm = 0;
    if (r.aux_int("NM", &vnm)) t |= BRC_TAG_NM;      // bam_aux_get + bam_aux2i (BasicStat.cpp:94-96)
    if (r.aux_int("SM", &vsm)) t |= BRC_TAG_SM;      // (BasicStat.cpp:79-81)
    nm.push_back(vnm); sm.push_back(vsm); tags.push_back(t);
    if (keep_names) { name_off.push_back(names.size()); const char* q = r.qname(); const size_t ql = strnlen(q, r.l_qname); names.insert(names.end(), q, q + ql); names.push_back(0); }   // (a record whose name lacks its NUL stays inside the record)
}

brc_read_batch Batcher::view() const {
    brc_read_batch v; memset(&v, 0, sizeof v);
    v.n_reads = (int64_t)pos.size(); v.pos = pos.data(); v.flag = flag.data(); v.mapq = mapq.data(); v.lib = lib.data();
    v.l_qseq = l_qseq.data(); v.n_cigar = n_cigar.data(); v.cigar_off = cig_off.data(); v.seq_off = seq_off.data(); v.qual_off = qual_off.data();
    v.nm = nm.data(); v.sm = sm.data(); v.tags = tags.data(); v.cigar = cigar.data(); v.seq4 = seq4.data(); v.qual = qual.data();
    v.n_cigar_total = cigar.size(); v.seq_bytes = seq4.size(); v.qual_bytes = qual.size();
    name_ptr.resize(name_off.size());
    for (size_t i = 0; i < name_off.size(); ++i) name_ptr[i] = names.data() + name_off[i];
    v.qname = name_ptr.empty() ? nullptr : name_ptr.data();
    return v;
}

static int lib_index(const Ctx& c, const BamRecord& r) {      // bam_get_library: RG tag -> @RG ID -> LB
    const char* rg = r.aux_str("RG");
    if (!rg) return -1;
    auto it = c.header().rg2lb.find(rg);
    if (it == c.header().rg2lb.end()) return -1;
    for (size_t i = 0; i < c.libs.size(); ++i) if (c.libs[i] == it->second) return (int)i;
    return -1;
}

// Reads of one chunk [a-1, b) (the reference's own fetch rule, :602), decoded by a pool of readers: the chunk is cut
// by read START position into K stripes; stripe i keeps the records whose pos lies in its stripe (stripe 0 also the reads
// that start before the chunk), so the stripes concatenated are exactly the single-handle fetch, in file order.
// (BRC_FETCH_STRIPE_MIN: tests force small chunks into stripes)
void fetch_chunk(Ctx& c, int tid, int64_t a, int64_t b, Fetched& out) {
    out.ok = true; out.err.clear();
    const int64_t q0 = a - 1 < 0 ? 0 : a - 1;
    unsigned K = 1;
    if (b - q0 >= g_knobs.fetch_stripe_min) {
        K = effective_cpus() * 3 / 4 / g_engines; if (K < 2) K = 2; if (K > 32) K = 32;
        if (g_knobs.fetch_threads > 0) K = (unsigned)g_knobs.fetch_threads;
        if ((int64_t)K > b - q0) K = (unsigned)(b - q0);          // every stripe at least one position wide (stripe 0 must contain q0)
    }
    if (out.parts.size() < K) out.parts.resize(K);
    for (Batcher& p : out.parts) { p.clear(); p.keep_names = c.opt.max_warnings != 0; }
    // a buffer that has been through one piece knows its sizes: from its second piece on its arenas are page-locked and the engine
    // uploads them in place (run_region: brc_push_reads_pinned)
    if (g_knobs.zero_copy && out.allow_pinned && out.uses++ > 0) for (Batcher& p : out.parts) if (p.seen_qual) p.use_pinned();
    // the readers of this BUFFER, one per stripe, never the context's one — two pieces are fetched side by side (also a piece too short
    // for stripes, K == 1)
    bool share = false;
    if (c.is_cram) {
        // stripes of a CRAM piece: a reader of its own per stripe (a stripe decodes the slices that overlap it — a slice that straddles a
        // stripe boundary twice — and keeps the records that START in it); the contig's bases, which run_region holds, are shared
        while (out.cram_pool.size() < K) {
            out.cram_pool.emplace_back(new CramReader());
            if (!out.cram_pool.back()->open(c.opt.bam, c.have_fa ? &c.fa : nullptr)) { out.ok = false; out.err = out.cram_pool.back()->error(); return; }
        }
        share = c.have_fa && c.ref_tid == tid && !c.ref.empty();
    } else {
        while (out.pool.size() < K) { out.pool.emplace_back(new BamReader()); if (!out.pool.back()->open(c.opt.bam)) { out.ok = false; out.err = "cannot reopen " + c.opt.bam; return; } }
        // --brc-device-inflate: everything the piece's query may read is inflated in one call; the stripes read that window side by side
        // (a block outside it — a record that runs past a chunk's last block — is inflated on demand by the stripe that needs it)
        if (c.inf) {
            for (unsigned i = 0; i < K; ++i) if (!out.pool[i]->external()) out.pool[i]->set_external(c.inf);
            std::shared_ptr<InflatedWindow> w = out.pool[0]->prefetch(c.idx, tid, a - 1, b);
            for (unsigned i = 0; i < K; ++i) out.pool[i]->share_window(w);
        }
    }
    struct DropWindow { Fetched& f; ~DropWindow() { for (auto& r : f.pool) if (r->external()) r->share_window(nullptr); } } drop_window{out};   // (BAM handles only)
    std::atomic<int> failed(0); std::mutex em;
    auto work = [&](unsigned i) {
        const int64_t s0 = q0 + (b - q0) * (int64_t)i / (int64_t)K, s1 = q0 + (b - q0) * (int64_t)(i + 1) / (int64_t)K;
        const int64_t from = i == 0 ? a - 1 : s0;
        auto keep = [&](const BamRecord& r) {
            if (r.pos >= s1 || (i > 0 && r.pos < s0)) return;
            out.parts[i].add(r, c.opt.per_lib ? lib_index(c, r) : 0);
        };
        bool ok; const std::string* why;
        if (c.is_cram) { CramReader& rd = *out.cram_pool[i]; rd.share_reference(tid, share ? &c.ref : nullptr); ok = rd.fetch(tid, from, s1, keep); why = &rd.error(); }
        else { BamReader& rd = *out.pool[i]; ok = rd.fetch(c.idx, tid, from, s1, keep); why = &rd.error(); }
        if (!ok) { failed = 1; std::lock_guard<std::mutex> g(em); if (out.err.empty()) out.err = *why; }      // the first stripe's word
    };
    std::vector<std::thread> th;
    for (unsigned i = 1; i < K; ++i) th.emplace_back(work, i);
    work(0);
    for (std::thread& t : th) t.join();
    if (!failed) return;
    out.ok = false;      // (a CRAM reader's text says what it is by itself)
    if (!c.is_cram) out.err = "read error while fetching a region stripe" + (out.err.empty() ? std::string() : ": " + out.err);
}

void fetch_site_batch(const Ctx& c, const std::vector<Site>& sites, SiteFetch& F) {
    const double ts0 = now_s();
    const size_t n = sites.size();
    std::vector<Batcher>& parts = F.parts; parts.clear(); parts.resize(n);
    for (Batcher& b : parts) b.keep_names = c.opt.max_warnings != 0;
    std::vector<int64_t>& lo = F.lo; std::vector<int64_t>& hi = F.hi; lo.assign(n, 0); hi.assign(n, 0);
    std::atomic<size_t> next(0); std::atomic<int> failed(0);
    // Clusters of consecutive lines that one indexed fetch serves at no extra cost: an index points at 16-kb windows (the
    // linear index; a CSI's finest bins), so a fetch for line k decodes its window from the window's first record up to the
    // line.  A following line in the SAME window (ascending, same contig) would decode the same records again — with one site
    // per kb, sixteen times — so it joins the cluster and every record is handed to the lines it overlaps with exactly
    // samfetch's test.  A line in a LATER window starts a cluster of its own: one fetch over both would also decode
    // everything between them (at the 31-kb spacing of a whole-genome SNV list that was three times the bytes).
    std::vector<std::pair<size_t, size_t> > clusters;
    for (size_t i0 = 0; i0 < n;) {
        size_t i1 = i0 + 1;
        int64_t reach = sites[i0].end;                     // the cluster's fetch decodes up to here anyway
        while (i1 < n && i1 - i0 < 256 && sites[i1].tid == sites[i0].tid && sites[i1].beg0 >= sites[i1 - 1].beg0 && sites[i1].beg0 - sites[i0].beg0 <= 65536 &&
               (((sites[i1].beg0 > 0 ? sites[i1].beg0 - 1 : 0) >> 14) <= (reach >> 14) || sites[i1].beg0 - reach <= 2048)) { reach = std::max(reach, sites[i1].end); ++i1; }
        clusters.push_back(std::make_pair(i0, i1));
        i0 = i1;
    }
    auto work = [&]() {
        BamReader rd;
        if (!rd.open(c.opt.bam)) { failed = 1; return; }
        if (c.inf) rd.set_external(c.inf);
        for (;;) {
            const size_t ci = next.fetch_add(1);
            if (ci >= clusters.size()) break;
            const size_t i0 = clusters[ci].first, i1 = clusters[ci].second;
            int64_t cend = 0;
            for (size_t i = i0; i < i1; ++i) { lo[i] = sites[i].beg0 > 0 ? sites[i].beg0 - 1 : 0; hi[i] = sites[i].end; cend = std::max(cend, sites[i].end); }
            size_t jlo = i0;                       // lines before it end at or before every coming record's start (lines are < 1 kb wide)
            if (!rd.fetch(c.idx, sites[i0].tid, sites[i0].beg0 - 1, cend, [&](const BamRecord& rec) {
                    const int64_t rend = rec.endpos();
                    while (jlo < i1 && sites[jlo].beg0 + 1000 <= rec.pos) ++jlo;
                    for (size_t j = jlo; j < i1 && sites[j].beg0 - 1 < rend; ++j) {
                        const Site& st = sites[j];
                        const int64_t qb = st.beg0 - 1 < 0 ? 0 : st.beg0 - 1;                  // samfetch: beg clamped at 0, pos < end && endpos > beg
                        if (st.end <= qb || rec.pos >= st.end || rend <= qb) continue;
                        parts[j].add(rec, c.opt.per_lib ? lib_index(c, rec) : 0);
                        if (rec.pos < lo[j]) lo[j] = rec.pos;
                        if (rend > hi[j]) hi[j] = rend;
                    }
                })) failed = 1;
            for (size_t i = i0; i < i1; ++i) hi[i] += 64;      // room for deletion alleles read from the reference past the last read
        }
    };
    unsigned nthr = effective_cpus(); if (nthr > 64) nthr = 64;
    if (g_knobs.fetch_threads > 0) nthr = (unsigned)g_knobs.fetch_threads;
    std::vector<std::thread> th;
    for (unsigned k = 1; k < nthr && (size_t)k < clusters.size(); ++k) th.emplace_back(work);
    work();
    for (std::thread& t : th) t.join();
    F.ok = !failed; F.n_clusters = clusters.size(); F.seconds = now_s() - ts0;
}
