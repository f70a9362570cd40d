// brc_inorm_core.h — per-lane functions of the device-side indel normalisation (include/brc_inorm.h), written once for the gfx950
// kernels (brc_inorm.hip) and for the CPU build the tests run (tests/sim_inorm): brc_indels_core.h's pipeline — a counting sort by
// position, a rank inside each run — with the NORMALISED position as key, and a merge of equal neighbours behind it.
//
//   shift_lane   lane = input record: judged or not, the left steps against the reference, npos / shift / flags, and the record
//                counts itself at its normalised position                                                  (atomic)
//   [scan]       cnt[] -> run starts start[], judged total -> tot[0]
//   place_lane   lane = input record: its index goes into its normalised position's run, anywhere in it    (atomic cursor)
//   rank_lane    lane = placed record: how many peers of its run come before it by (library, sign, normalised text, input index)
//   heads_lane   lane = ranked record: a head when it differs from its predecessor in (npos, lib, len, text); its text length
//   [scan]       head[] -> merged indices gidx[], total -> tot[1] = counts[0]
//   [scan]       the heads' text lengths -> aoff[], total -> tot[2] = counts[1]
//   merge_lane   lane = ranked record: group; a head walks its members in order — the sums, metrics13, members, the stores, the text
// The normalised text is never materialised before the last store: character i of a record that went s steps left is read THROUGH THE
// ROTATION (chr below) from the input bytes and the reference.  The scans are cooperative on the device (brc_side_scan.h) and serial
// loops in the CPU build; everything else is the same code.
#ifndef BRC_INORM_CORE_H
#define BRC_INORM_CORE_H

#include <stdint.h>

#include "../../include/brc_inorm.h"
#include "brc_indels_core.h"     // fetch_add, fetch_sub, scan_blocks, SCAN_TILE; brc_dense_core.h: metrics13, put

namespace brcinorm {

using brcdense::NF;
using brcdense::NI;
using brcdense::NM;
using brcdense::put;
using brcindels::fetch_add;
using brcindels::fetch_sub;
using brcindels::scan_blocks;

enum { BLOCK = brcindels::SCAN_TILE };                     // four waves; a scan's tile
static const uint32_t UNJUDGED = 0xFFFFFFFFu;                // wshift of a record that is not judged

// One call's work, BY VALUE in the kernel arguments: the reference slice, the window, the table, the scratch, the destinations (any of
// them nullptr: not wanted).
struct Job {
    const char* ref; int64_t ref_lo, ref_hi, ref_len;
    int64_t first, n, floor; int32_t n_lib; uint32_t max_shift;
    int64_t m, TS, A;                                      // records; istat / fstat planes TS elements apart; alleles_len
    const int32_t *pos, *lib, *len; const uint32_t* rep_read; const int32_t* rep_qpos; const uint32_t* istat; const float* fstat;
    const uint32_t* off; const uint8_t* text;
    int64_t cap, acap;
    // scratch (32-bit words): cnt [n] records per normalised position (counted up by shift_lane, down again by place_lane), start
    // [n + 1] run starts, placed [m] input indices grouped by position, order [m] input index of ranked record j, head [m] 1 where j
    // opens a class, gidx [m + 1] heads before j, alen [m] a head's text length, aoff [m + 1] text offsets, wnpos / wshift [m] the walk's
    // results per input record, part [.] the scans' workgroup partials, tot [3] = judged records, merged records, allele bytes
    uint32_t *cnt, *start, *placed, *order, *head, *gidx, *alen, *aoff; int32_t* wnpos; uint32_t *wshift, *part, *tot;
    uint32_t* o_counts; int32_t* o_npos; uint32_t *o_shift, *o_flags; int32_t* o_group;
    int32_t *o_pos, *o_lib, *o_len; uint32_t* o_rep_read; int32_t* o_rep_qpos; uint32_t *o_members, *o_istat; float *o_fstat, *o_metrics;
    uint32_t* o_aoff; uint8_t* o_alleles; uint32_t* status;
};

// words of scratch for a window of n positions and a table of m records
inline uint64_t workspace_words(uint64_t n, uint64_t m) {
    const uint64_t nb = scan_blocks(n > m + 1 ? n : m + 1) + 1;
    return n + (n + 1) + 6u * m + 2u * (m + 1) + nb + 3;
}
inline size_t workspace_bytes(int64_t n, int64_t m) {
    if (n <= 0 || m <= 0) return 0;
    return (size_t)(workspace_words((uint64_t)n, (uint64_t)m) * 4u);
}
inline void carve(Job& J, void* ws) {
    uint32_t* w = (uint32_t*)ws; const uint64_t n = (uint64_t)J.n, m = (uint64_t)J.m;
    J.cnt = w; w += n; J.start = w; w += n + 1; J.placed = w; w += m; J.order = w; w += m; J.head = w; w += m; J.alen = w; w += m;
    J.wshift = w; w += m; J.gidx = w; w += m + 1; J.aoff = w; w += m + 1; J.wnpos = (int32_t*)w; w += m;
    J.part = w; w += scan_blocks(n > m + 1 ? n : m + 1) + 1; J.tot = w;
}

BRCD_HD void or_bits(uint32_t* p, uint32_t bits) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicOr(p, bits);
#else
    *p |= bits;
#endif
}

// R(p) of include/brc_inorm.h: the raw character, 0 = none
BRCD_HD uint8_t ref_char(const Job& J, int64_t p) {
    return (J.ref && p >= J.ref_lo && p < J.ref_hi && p < J.ref_len && p >= 0) ? (uint8_t)J.ref[p - J.ref_lo] : (uint8_t)0;
}
// base(c): 'A' 'C' 'G' 'T', 0 = none (clearing bit 5 folds a..z onto A..Z, and no other character lands on a letter)
BRCD_HD uint32_t base_of(uint8_t c) {
    const uint32_t u = c & 0xdfu;
    return (u == 'A' || u == 'C' || u == 'G' || u == 'T') ? u : 0u;
}
BRCD_HD bool match(uint8_t a, uint8_t b) {
    const uint32_t x = base_of(a);
    return x != 0u && x == base_of(b);
}

// text(r): its start inside alleles and its length, whatever allele_off holds
BRCD_HD int64_t text_of(const Job& J, int64_t r, int64_t* a) {
    int64_t a0 = J.off[r], a1 = J.off[r + 1];
    if (a0 > J.A) a0 = J.A;
    if (a1 > J.A) a1 = J.A;
    *a = a0;
    return a1 > a0 ? a1 - a0 : 0;
}

// Lane = input record r: ONE load of pos, lib, len and the two offsets, then the walk: per step one reference byte and at most one
// text byte (an insertion compares t[(L - 1 - s) mod L], a deletion t[L - 1 - s] while s < L and R(p + L) from then on).  The table is
// sorted by position: the reference bytes neighbouring lanes walk share cache lines; the loop ends per lane.
BRCD_HD void shift_lane(const Job& J, int64_t r) {
    int64_t p = J.pos[r]; const int64_t l = J.lib[r]; const int32_t ln = J.len[r];
    int64_t a; const int64_t nt = text_of(J, r, &a);
    const int64_t L = ln < 0 ? -(int64_t)ln : (int64_t)ln;
    const bool ins = ln > 0;
    const bool judged = ln != 0 && p >= J.first && p < J.first + J.n && l >= 0 && l < J.n_lib && nt == L + 1 && J.text[a] == (ins ? '+' : '-');
    uint32_t s = 0u, fl = 0u;
    if (!judged) {
        fl = BRC_INORM_NOT_JUDGED;
        J.wshift[r] = UNJUDGED;
        if (J.o_group) put(J.o_group + r, (int32_t)-1);
    } else {
        const uint8_t* t = J.text + a + 1;
        int64_t ti = L - 1;                                // the compared character's place in the input text; below 0: the deletion's text has left its own bytes
        for (;;) {
            const uint8_t tc = (ins || ti >= 0) ? t[ti] : ref_char(J, p + L);
            if (!match(ref_char(J, p), tc)) break;
            if (s == J.max_shift) { fl = BRC_INORM_LIMIT; break; }
            if (p - 1 < J.floor) { fl = BRC_INORM_EDGE; break; }
            --p; ++s; --ti;
            if (ins && ti < 0) ti = L - 1;
        }
        J.wshift[r] = s;
        if (J.cnt) (void)fetch_add(J.cnt + (p - J.first), 1u);
    }
    J.wnpos[r] = (int32_t)p;
    if (J.o_npos) put(J.o_npos + r, (int32_t)p);
    if (J.o_shift) put(J.o_shift + r, s);
    if (J.o_flags) put(J.o_flags + r, fl);
    if (J.status && fl) or_bits(J.status, fl);             // (NOT_JUDGED / LIMIT / EDGE are TABLE_BAD / ANY_LIMIT / ANY_EDGE: the same values)
}
static_assert(BRC_INORM_NOT_JUDGED == BRC_INORM_TABLE_BAD && BRC_INORM_LIMIT == BRC_INORM_ANY_LIMIT && BRC_INORM_EDGE == BRC_INORM_ANY_EDGE,
              "a record's flags are the status bits they set");

// (after the scan of cnt: start[d] is the start of position d's run, cnt[d] its length — counted down here, so the scratch ends as zeros)
BRCD_HD void place_lane(const Job& J, int64_t r) {
    if (J.wshift[r] == UNJUDGED) return;
    const int64_t d = (int64_t)J.wnpos[r] - J.first;
    const uint32_t k = fetch_sub(J.cnt + d, 1u) - 1u;
    J.placed[J.start[d] + k] = (uint32_t)r;
}

// A judged record's normalised text, read through the rotation: t = the input bytes behind the sign, s = its steps, p = npos.
struct Txt { const uint8_t* t; int64_t L, s, p, rot; int32_t lib, len; };
BRCD_HD Txt txt_of(const Job& J, uint32_t r) {
    Txt T; int64_t a;
    (void)text_of(J, r, &a);
    T.t = J.text + a + 1; T.lib = J.lib[r]; T.len = J.len[r];
    T.L = T.len < 0 ? -(int64_t)T.len : (int64_t)T.len;
    T.s = J.wshift[r]; T.p = J.wnpos[r];
    T.rot = T.len > 0 ? (T.L - T.s % T.L) % T.L : 0;       // an insertion's character i is input character (i - s) mod L
    return T;
}
BRCD_HD uint8_t chr(const Job& J, const Txt& T, int64_t i) {
    if (T.len > 0) { int64_t k = i + T.rot; if (k >= T.L) k -= T.L; return T.t[k]; }
    return i < T.s ? ref_char(J, T.p + 1 + i) : T.t[i - T.s];      // a deletion: the reference's raw characters of the stretch, then its own
}

// order of two records of ONE normalised position: library, then the texts as std::string compares them — '+' before '-', bytewise, a
// prefix before the longer text.  < 0: a first.
BRCD_HD int compare(const Job& J, const Txt& a, const Txt& b) {
    if (a.lib != b.lib) return a.lib < b.lib ? -1 : 1;
    if ((a.len > 0) != (b.len > 0)) return a.len > 0 ? -1 : 1;
    const int64_t n = a.L < b.L ? a.L : b.L;
    for (int64_t i = 0; i < n; ++i) {
        const uint8_t ca = chr(J, a, i), cb = chr(J, b, i);
        if (ca != cb) return ca < cb ? -1 : 1;
    }
    return a.L < b.L ? -1 : (a.L > b.L ? 1 : 0);
}

// Lane = placed record j: its rank among the records of its run.  Equal records are ordered by input index, so the members of a class
// are consecutive and ascend.  Quadratic in the run's length: a run is the handful of alleles of one position.
BRCD_HD void rank_lane(const Job& J, int64_t j) {
    if (j >= (int64_t)J.tot[0]) return;
    const uint32_t r = J.placed[j];
    const Txt T = txt_of(J, r);
    const int64_t d = T.p - J.first;
    const uint32_t lo = J.start[d], hi = J.start[d + 1];
    uint32_t rank = 0;
    for (uint32_t x = lo; x < hi; ++x) {
        if (x == (uint32_t)j) continue;
        const uint32_t q = J.placed[x];
        const int c = compare(J, txt_of(J, q), T);
        if (c < 0 || (c == 0 && q < r)) ++rank;
    }
    J.order[lo + rank] = r;
}

// Lane = ranked record j: does it open a class?
BRCD_HD void heads_lane(const Job& J, int64_t j) {
    if (j >= (int64_t)J.tot[0]) return;
    const Txt T = txt_of(J, J.order[j]);
    bool h = j == 0;
    if (!h) {
        const Txt Q = txt_of(J, J.order[j - 1]);
        h = Q.p != T.p || Q.len != T.len || compare(J, Q, T) != 0;
    }
    J.head[j] = h ? 1u : 0u;
    J.alen[j] = h ? (uint32_t)(T.L + 1) : 0u;
}

// Lane = ranked record j in [0, judged]: lane `judged` only closes the offsets.  A merged record at or behind `cap` stores nothing, its
// text included.
BRCD_HD void merge_lane(const Job& J, int64_t j) {
    const int64_t Jt = J.tot[0], M = J.tot[1];
    if (j > Jt) return;
    if (j == Jt) {
        if (J.o_aoff && M <= J.cap) put(J.o_aoff + M, J.aoff[Jt]);
        return;
    }
    const uint32_t r = J.order[j], h = J.head[j];
    const int64_t g = (int64_t)J.gidx[j] + h - 1;
    if (J.o_group) put(J.o_group + r, (int32_t)g);
    if (!h) return;
    const uint32_t a0 = J.aoff[j];
    if (J.o_aoff && g <= J.cap) put(J.o_aoff + g, a0);
    if (g >= J.cap) return;
    const Txt T = txt_of(J, r);
    if (J.o_pos) put(J.o_pos + g, (int32_t)T.p);
    if (J.o_lib) put(J.o_lib + g, T.lib);
    if (J.o_len) put(J.o_len + g, T.len);
    if (J.o_rep_read) put(J.o_rep_read + g, J.rep_read ? J.rep_read[r] : 0u);
    if (J.o_rep_qpos) put(J.o_rep_qpos + g, J.rep_qpos ? J.rep_qpos[r] : (int32_t)0);
    int64_t e = j + 1;
    while (e < Jt && !J.head[e]) ++e;
    if (J.o_members) put(J.o_members + g, (uint32_t)(e - j));
    if (J.o_istat || J.o_fstat || J.o_metrics) {
        uint32_t si[NI]; float sf[NF];
        for (int f = 0; f < NI; ++f) si[f] = J.istat[(int64_t)f * J.TS + r];
        for (int f = 0; f < NF; ++f) sf[f] = J.fstat[(int64_t)f * J.TS + r];
        for (int64_t x = j + 1; x < e; ++x) {              // (ascending input index: the order of the fp32 additions is the definition's)
            const uint32_t q = J.order[x];
            for (int f = 0; f < NI; ++f) si[f] += J.istat[(int64_t)f * J.TS + q];
            for (int f = 0; f < NF; ++f) sf[f] = sf[f] + J.fstat[(int64_t)f * J.TS + q];
        }
        if (J.o_istat) for (int f = 0; f < NI; ++f) put(J.o_istat + (int64_t)f * J.cap + g, si[f]);
        if (J.o_fstat) for (int f = 0; f < NF; ++f) put(J.o_fstat + (int64_t)f * J.cap + g, sf[f]);
        if (J.o_metrics) {
            float mt[NM];
            brcdense::metrics13(si, sf, mt);
            for (int f = 0; f < NM; ++f) put(J.o_metrics + (int64_t)f * J.cap + g, mt[f]);
        }
    }
    if (J.o_alleles && (int64_t)a0 + T.L + 1 <= J.acap) {
        uint8_t* w = J.o_alleles + a0;
        w[0] = (uint8_t)(T.len > 0 ? '+' : '-');
        for (int64_t i = 0; i < T.L; ++i) w[1 + i] = chr(J, T, i);
    }
}

// The argument checks of brc_inorm_table (everything but the kind of memory, which the two libraries check themselves): 0 = fine.
inline int check_job(const brc_device_indels* v, const brc_inorm_params* p, const brc_inorm_source* t, int64_t k0, int64_t n, int64_t cap, int64_t acap,
                     const void* ws, size_t ws_bytes, const char** why) {
    if (!v) { *why = "no view"; return BRC_E_ARG; }
    if (!p) { *why = "no parameters"; return BRC_E_ARG; }
    if (!t) { *why = "no table"; return BRC_E_ARG; }
    if (v->n_lib < 1 || v->n_pos < 0) { *why = "not a view of a computed region"; return BRC_E_ARG; }
    if (k0 < 0 || n < 0 || k0 > v->n_pos || n > v->n_pos - k0) { *why = "the window must lie inside the view's positions"; return BRC_E_ARG; }
    if (cap < 0 || acap < 0) { *why = "negative capacity"; return BRC_E_ARG; }
    if (p->max_shift > BRC_INORM_MAX_SHIFT) { *why = "max_shift above BRC_INORM_MAX_SHIFT"; return BRC_E_ARG; }
    if (p->reserved[0] || p->reserved[1] || p->reserved[2]) { *why = "a reserved word is not 0"; return BRC_E_ARG; }
    if (t->m < 0 || t->stride < t->m) { *why = "a table with m below 0 or stride below m"; return BRC_E_ARG; }
    if (t->alleles_len < 0) { *why = "alleles_len below 0"; return BRC_E_ARG; }
    if ((uint64_t)t->m >= 0x7ffffff0ull || (uint64_t)n >= 0x7ffffff0ull) { *why = "table or window too large: records and positions are indexed with 32 bits"; return BRC_E_ARG; }
    if (t->m > 0 && (!t->pos || !t->lib || !t->len || !t->istat || !t->fstat || !t->allele_off || !t->alleles)) { *why = "a table without its arrays"; return BRC_E_ARG; }
    const size_t need = workspace_bytes(n, t->m);
    if (need && (!ws || ws_bytes < need)) { *why = "workspace missing or smaller than brc_inorm_workspace"; return BRC_E_ARG; }
    return BRC_OK;
}
inline bool wants_records(const Job& J) {
    return J.o_pos || J.o_lib || J.o_len || J.o_rep_read || J.o_rep_qpos || J.o_members || J.o_istat || J.o_fstat || J.o_metrics || J.o_aoff || J.o_alleles;
}
// the sort and the merge behind the walk run when something of the new table is wanted
inline bool wants_table(const Job& J) { return J.o_counts || J.o_group || wants_records(J); }
inline bool wants_anything(const Job& J) { return wants_table(J) || J.o_npos || J.o_shift || J.o_flags || J.status; }
inline Job make_job(const brc_device_indels* v, const brc_inorm_params* p, const brc_inorm_source* t, int64_t k0, int64_t n, void* ws, uint32_t* counts,
                    int32_t* npos, uint32_t* shift, uint32_t* flags, int32_t* group, int64_t cap, int64_t acap, int32_t* pos, int32_t* lib, int32_t* len,
                    uint32_t* rep_read, int32_t* rep_qpos, uint32_t* members, uint32_t* istat, float* fstat, float* metrics, uint32_t* allele_off,
                    uint8_t* alleles, uint32_t* status) {
    Job J;
    J.ref = v->ref; J.ref_lo = v->ref_lo; J.ref_hi = v->ref_hi; J.ref_len = v->ref_len;
    J.first = (int64_t)v->pos0 + k0; J.n = n; J.floor = J.first > J.ref_lo ? J.first : J.ref_lo; J.n_lib = v->n_lib; J.max_shift = p->max_shift;
    J.m = t->m; J.TS = t->stride; J.A = t->alleles_len;
    J.pos = t->pos; J.lib = t->lib; J.len = t->len; J.rep_read = t->rep_read; J.rep_qpos = t->rep_qpos; J.istat = t->istat; J.fstat = t->fstat;
    J.off = t->allele_off; J.text = t->alleles;
    J.cap = cap; J.acap = acap;
    carve(J, ws);
    J.o_counts = counts; J.o_npos = npos; J.o_shift = shift; J.o_flags = flags; J.o_group = group;
    J.o_pos = pos; J.o_lib = lib; J.o_len = len; J.o_rep_read = rep_read; J.o_rep_qpos = rep_qpos; J.o_members = members;
    J.o_istat = istat; J.o_fstat = fstat; J.o_metrics = metrics; J.o_aoff = allele_off; J.o_alleles = alleles; J.status = status;
    if (!wants_table(J)) J.cnt = nullptr;                  // (the walk alone: nothing is counted, sorted or merged)
    return J;
}
// bytes the host can count (brc_inorm_last_timing)
inline void job_bytes(const Job& J, uint64_t* rd, uint64_t* wr) {
    const uint64_t m = (uint64_t)J.m, n = (uint64_t)J.n, tab = wants_table(J) ? 1u : 0u;
    *rd = 4u * m * (5u + 2u + tab * (NI + NF));
    *wr = 4u * (2u * m + tab * (3u * n + 1u + 6u * m + 2u));
}

}  // namespace brcinorm
#endif
