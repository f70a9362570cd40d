// brc_deflate_core.h — compression of up to 0xff00 bytes into ONE BGZF member (SAMv1 4.1: a gzip member, RFC 1952, whose payload is a
// raw deflate stream, RFC 1951) by ONE WORKGROUP of 256 lanes, written once for the device and for the host: brc_deflate.hip runs
// deflate_member() with one workgroup per member, tests/sim_deflate runs the very same function with the lanes of every parallel
// phase executed one after the other.  Output bytes are a pure function of input bytes: every place where lanes meet is a
// commutative LDS / memory atomic (max, add, or), and no phase reads what another lane writes in the same phase.
//
// Written from RFC 1951 / RFC 1952, the BGZF section of the SAM specification and Moffat & Katajainen, "In-place calculation of
// minimum-redundancy codes" (1995); no code of any deflate library is involved.
//
// How the work is divided:
//   * staging: the member's input goes to LDS in 16-byte loads and stays there (matches reach back to the member's first byte,
//     at most 32768 bytes; there is no history across members);
//   * CRC32 of the input: one segment per lane, combined with crc_advance_zeros / gf2_mul of brc_inflate_core.h;
//   * the member is cut into deflate blocks of BLOCK input positions; per block:
//       - match finding, lane = position, STEP = 256 positions at a time: a 4-byte multiplicative hash; the FAR candidate is the
//         head table's entry (the highest position with this hash in any EARLIER step: the step's own positions enter the table,
//         with atomicMax, only after every lane of the step has looked); the NEAR candidate covers what the table cannot know
//         yet — the step's own positions: the nearest of the NEAR positions before this one whose hash (kept in a ring in LDS)
//         is the same, which finds the short periods of the text (`:0.00:0.00:`); both are measured against LDS, 4 bytes per
//         compare, capped at 258 and at the block's end; the longer wins, the nearer on a tie;
//       - parse: lane 0 hops through the lengths, greedy (next = p + (len >= 3 ? len : 1)), and writes the tokens over the
//         match array (token k never lies behind position k);
//       - codes: histogram with LDS atomics; the used symbols are ranked by (count, symbol) by all lanes; lane 0 (literal/length)
//         and lane 64 (distance) run the in-place minimum-redundancy algorithm on the sorted counts and a Kraft fix-up that
//         limits the lengths to 15 bits; lane 0 run-length codes the lengths (symbols 16/17/18) and builds the 7-bit
//         code-length code; the smallest of dynamic, fixed and stored is emitted;
//       - emit: every lane sums the bits of its share of the tokens, lane 0 scans the 256 sums, every lane ORs its tokens at
//         its own bit offset into the member's slot in memory (zeroed before the launch) with atomicOr;
//   * a stream of input length + 5 bytes or more is replaced by one stored block: no member exceeds input + 31 bytes.
#ifndef BRC_DEFLATE_CORE_H
#define BRC_DEFLATE_CORE_H

#include "brc_inflate_core.h"      // gf2_mul, crc_advance_zeros, len_base / len_extra / dist_base / dist_extra, BRCI_HD

#if defined(__HIP_DEVICE_COMPILE__)
#define BRCD_FOR_LANES(l) for (int l = (int)threadIdx.x, brcd_once_ = 1; brcd_once_; brcd_once_ = 0)
#define BRCD_LANE(k) if (threadIdx.x == (unsigned)(k))
#define BRCD_SYNC() __syncthreads()
#define BRCD_MAX(p, v) atomicMax((p), (v))
#define BRCD_ADD(p, v) atomicAdd((p), (v))
#define BRCD_OR(p, v) atomicOr((p), (v))
#else
#define BRCD_FOR_LANES(l) for (int l = 0; l < brcdef::LANES; ++l)
#define BRCD_LANE(k) if (true)
#define BRCD_SYNC() ((void)0)
#define BRCD_MAX(p, v) (*(p) = *(p) > (v) ? *(p) : (v))
#define BRCD_ADD(p, v) (*(p) += (v))
#define BRCD_OR(p, v) (*(p) |= (v))
#endif

namespace brcdef {

constexpr int LANES = 256;
constexpr uint32_t MEMBER_IN = 0xff00;              // input bytes of a member (bgzip's block size)
constexpr uint32_t BLOCK = 16384;                   // input positions of one deflate block
constexpr int HASH_BITS = 12;
constexpr uint32_t NEAR = 32;                       // positions before its own a lane compares hashes with
constexpr uint32_t MAX_DIST = 32768, MAX_LEN = 258;
constexpr uint32_t SLOT = MEMBER_IN + 64;           // bytes of a member's slot in memory (a multiple of 16; header 18, blocks <= input + 5 each, trailer 8)
constexpr uint32_t SLOT_WORDS = SLOT / 4;
constexpr uint32_t HDR = 18, TRAILER = 8;
constexpr uint32_t TOK_LIT = 0x80000000u;
constexpr uint32_t NO_HASH = 0xffffu;
constexpr uint32_t DBASE = 288;                     // hist / lens / code: [0, 286) literal/length symbols, [288, 318) distance symbols

static_assert(BLOCK % LANES == 0 && HASH_BITS <= 15 && NEAR < (uint32_t)LANES, "steps tile a block; the ring holds two steps");

struct Shared {
    uint8_t in[MEMBER_IN + 16];                     // (zero behind the input: a 4-byte compare may read 3 bytes past it)
    uint32_t m[BLOCK];                              // per position len << 16 | dist (0: none); after the parse the block's tokens
    uint32_t head[1 << HASH_BITS];                  // hash -> highest position + 1 of the earlier steps (0: none)
    uint16_t ring[2 * LANES];                       // hash of position p at [p % 512]: this step's and the step's before
    uint32_t crc_tab[256];
    uint32_t hist[320];
    uint32_t A[320]; uint16_t sorted[320];          // the used symbols of both alphabets in ascending (count, symbol), and their counts
    uint8_t lens[320]; uint16_t code[320];          // code lengths; codes, bit-reversed (the stream carries them MSB first)
    uint32_t cnt[2][16];                            // codes per length (canonical numbering)
    uint32_t num[3][16];                            // the length limiter's counts
    uint8_t rle_sym[320], rle_extra[320];           // the code lengths as symbols 0..18 with their extra bits
    uint32_t clA[19]; uint16_t clsorted[19]; uint8_t cllens[19]; uint16_t clcode[19];
    uint32_t lane_bits[LANES];                      // bits of each lane's tokens, then their exclusive prefix sum
    uint32_t part[LANES];                           // per-lane CRC states
    uint32_t ntok, nused[2], cost[3], nrle, hlit, hdist, hclen, hdr_bits, btype, bitpos, crc;
};

BRCI_HD uint32_t ld32(const uint8_t* p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
BRCI_HD uint32_t hash4(uint32_t v) { return (v * 2654435761u) >> (32 - HASH_BITS); }
BRCI_HD uint32_t match_len(const uint8_t* in, uint32_t a, uint32_t p, uint32_t maxlen) {        // a < p; reads in[.., p + maxlen + 3)
    uint32_t i = 0;
    while (i + 4 <= maxlen) { const uint32_t x = ld32(in + a + i) ^ ld32(in + p + i); if (x) return i + ((uint32_t)__builtin_ctz(x) >> 3); i += 4; }
    while (i < maxlen && in[a + i] == in[p + i]) ++i;
    return i;
}
// length 3..258 -> its code 0..28 (symbol 257 + code); distance 1..32768 -> its code 0..29 (RFC 1951 3.2.5)
BRCI_HD uint32_t len_code(uint32_t len) {
    if (len == 258) return 28;
    const uint32_t l = len - 3;
    if (l < 8) return l;
    const uint32_t e = (31u - (uint32_t)__builtin_clz(l)) - 2u;
    return 4u * e + 4u + ((l >> e) & 3u);
}
BRCI_HD uint32_t dist_code(uint32_t dist) {
    const uint32_t d = dist - 1;
    if (d < 4) return d;
    const uint32_t e = (31u - (uint32_t)__builtin_clz(d)) - 1u;
    return 2u * e + 2u + ((d >> e) & 1u);
}
BRCI_HD uint32_t fixed_len(uint32_t i) { return i < 144 ? 8u : i < 256 ? 9u : i < 280 ? 7u : i < DBASE ? 8u : 5u; }
BRCI_HD uint32_t extra_bits(uint32_t i) { return i < 257 ? 0u : i < DBASE ? (i < 286 ? (uint32_t)brcinf::len_extra(i - 257) : 0u) : (i < DBASE + 30 ? (uint32_t)brcinf::dist_extra(i - DBASE) : 0u); }
BRCI_HD uint32_t rev_bits(uint32_t c, uint32_t n) { uint32_t r = 0; for (uint32_t b = 0; b < n; ++b) r |= ((c >> b) & 1u) << (n - 1 - b); return r; }

// n <= 32 bits of v at bit `bit` of the slot (zeroed words; bits of different callers never overlap)
BRCI_HD void put(uint32_t* w, uint32_t bit, uint32_t v, uint32_t n) {
    if (!n) return;
    const uint32_t word = bit >> 5, s = bit & 31u;
    if (word + 1 >= SLOT_WORDS) return;                       // (cannot happen: a block that would outgrow its stored form is stored)
    const uint64_t x = (uint64_t)v << s;
    if ((uint32_t)x) BRCD_OR(w + word, (uint32_t)x);
    if ((uint32_t)(x >> 32)) BRCD_OR(w + word + 1, (uint32_t)(x >> 32));
}

// one token as two bit fields (literal/length code + extra bits, distance code + extra bits)
BRCI_HD void token_fields(const Shared& sh, uint32_t t, uint32_t* v1, uint32_t* n1, uint32_t* v2, uint32_t* n2) {
    if (t & TOK_LIT) { const uint32_t s = t & 0xffu; *v1 = sh.code[s]; *n1 = sh.lens[s]; *v2 = 0; *n2 = 0; return; }
    const uint32_t len = t >> 16, dist = (t & 0xffffu) + 1u;              // (stored as dist - 1: 32768 needs 16 bits)
    const uint32_t lc = len_code(len), dc = dist_code(dist);
    const uint32_t ls = 257 + lc, ds = DBASE + dc;
    *v1 = (uint32_t)sh.code[ls] | (len - brcinf::len_base(lc)) << sh.lens[ls]; *n1 = (uint32_t)sh.lens[ls] + brcinf::len_extra(lc);
    *v2 = (uint32_t)sh.code[ds] | (dist - brcinf::dist_base(dc)) << sh.lens[ds]; *n2 = (uint32_t)sh.lens[ds] + brcinf::dist_extra(dc);
}

// Code lengths of at most maxbits for the n used symbols listed in sorted[] (ascending count; A[]: their counts), one lane.
// Moffat & Katajainen's three in-place passes give the unlimited lengths (A[0] the longest); lengths above maxbits are folded into
// maxbits and the Kraft sum is brought back to one a code at a time: a code leaves maxbits, the deepest shorter code moves one
// level down and the freed leaf's sibling takes the one that left.  The lengths are then dealt out longest first to the rarest.
BRCI_HD void limited_lengths(uint32_t* A, const uint16_t* sorted, uint32_t* num, uint8_t* lens_out, int n, int maxbits) {
    for (int i = 0; i <= maxbits; ++i) num[i] = 0;
    if (n <= 0) return;
    if (n == 1) { lens_out[sorted[0]] = 1; return; }
    A[0] += A[1];
    int root = 0, leaf = 2;
    for (int next = 1; next < n - 1; ++next) {
        if (leaf >= n || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = (uint32_t)next; } else A[next] = A[leaf++];
        if (leaf >= n || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = (uint32_t)next; } else A[next] += A[leaf++];
    }
    A[n - 2] = 0;
    for (int next = n - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
    int avbl = 1, used = 0, dpth = 0, next = n - 1;
    root = n - 2;
    while (avbl > 0) {
        while (root >= 0 && (int)A[root] == dpth) { ++used; --root; }
        while (avbl > used) { A[next--] = (uint32_t)dpth; --avbl; }
        avbl = 2 * used; ++dpth; used = 0;
    }
    for (int i = 0; i < n; ++i) { const uint32_t d = A[i] > (uint32_t)maxbits ? (uint32_t)maxbits : A[i]; ++num[d]; }
    uint32_t total = 0;
    for (int i = 1; i <= maxbits; ++i) total += num[i] << (maxbits - i);
    while (total > (1u << maxbits)) {
        --num[maxbits];
        for (int i = maxbits - 1; i >= 1; --i) if (num[i]) { --num[i]; num[i + 1] += 2; break; }
        --total;
    }
    int idx = 0;
    for (int len = maxbits; len >= 1; --len) for (uint32_t k = 0; k < num[len] && idx < n; ++k) lens_out[sorted[idx++]] = (uint8_t)len;
}

// One member.  src[0, n): the input, 0 < n <= MEMBER_IN (16-byte aligned on the device); slot: SLOT zeroed bytes, 4-byte aligned.
// Every lane of the workgroup calls this (the host: one call runs all lanes); returns the member's size in bytes.
BRCI_HD uint32_t deflate_member(Shared& sh, const uint8_t* src, uint32_t n, uint32_t* slot) {
    uint8_t* out8 = (uint8_t*)slot;
    if (n > MEMBER_IN) n = MEMBER_IN;
    // ---- staging, CRC table, head table
    {
        const uint32_t nvec = n / 16u;
        BRCD_FOR_LANES(l) {
            for (uint32_t v = (uint32_t)l; v < nvec; v += LANES) {
#if defined(__HIP_DEVICE_COMPILE__)
                *(uint4*)(sh.in + v * 16u) = *(const uint4*)(src + v * 16u);
#else
                __builtin_memcpy(sh.in + v * 16u, src + v * 16u, 16);
#endif
            }
            for (uint32_t i = nvec * 16u + (uint32_t)l; i < n + 16u; i += LANES) sh.in[i] = i < n ? src[i] : (uint8_t)0;
            for (int i = l; i < 256; i += LANES) { uint32_t c = (uint32_t)i; for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ 0xedb88320u : c >> 1; sh.crc_tab[i] = c; }
            for (int i = l; i < (1 << HASH_BITS); i += LANES) sh.head[i] = 0;
            for (int i = l; i < 2 * LANES; i += LANES) sh.ring[i] = (uint16_t)NO_HASH;
        }
        BRCD_LANE(0) { sh.bitpos = 0; }
        BRCD_SYNC();
    }
    // ---- CRC32 of the input: lane l takes bytes [l * seg, (l + 1) * seg), advances its register over the bytes behind it
    {
        const uint32_t seg = (n + LANES - 1) / LANES;
        BRCD_FOR_LANES(l) {
            uint32_t b = (uint32_t)l * seg; if (b > n) b = n;
            uint32_t e = b + seg; if (e > n) e = n;
            uint32_t c = l == 0 ? 0xffffffffu : 0u;
            for (uint32_t i = b; i < e; ++i) c = sh.crc_tab[(c ^ sh.in[i]) & 0xffu] ^ (c >> 8);
            sh.part[l] = (e > b || l == 0) ? brcinf::crc_advance_zeros(c, n - e) : 0u;
        }
        BRCD_SYNC();
        BRCD_LANE(0) { uint32_t c = 0; for (int i = 0; i < LANES; ++i) c ^= sh.part[i]; sh.crc = c ^ 0xffffffffu; }
        BRCD_SYNC();
    }
    const uint32_t nblocks = (n + BLOCK - 1) / BLOCK;
    for (uint32_t blk = 0; blk < nblocks; ++blk) {
        const uint32_t bs = blk * BLOCK, be = bs + BLOCK < n ? bs + BLOCK : n, blen = be - bs, last = blk + 1 == nblocks ? 1u : 0u;
        // ---- match finding, a step of 256 positions at a time
        for (uint32_t p0 = bs; p0 < be; p0 += LANES) {
            BRCD_FOR_LANES(l) {
                const uint32_t p = p0 + (uint32_t)l;
                if (p >= (uint32_t)LANES) {                       // the step before enters the head table: nobody looks during this phase
                    const uint32_t q = p - LANES, hq = sh.ring[q & (2 * LANES - 1)];
                    if (hq != NO_HASH) BRCD_MAX(&sh.head[hq], q + 1u);
                }
                sh.ring[p & (2 * LANES - 1)] = (uint16_t)(p + 4u <= n ? hash4(ld32(sh.in + p)) : NO_HASH);
            }
            BRCD_SYNC();
            BRCD_FOR_LANES(l) {
                const uint32_t p = p0 + (uint32_t)l;
                if (p < be) {
                    uint32_t best = 0, bdist = 0;
                    const uint32_t h = sh.ring[p & (2 * LANES - 1)], maxlen = be - p < MAX_LEN ? be - p : MAX_LEN;
                    if (h != NO_HASH && maxlen >= 3) {
                        for (uint32_t d = 1; d <= NEAR && d <= p; ++d) {
                            if (sh.ring[(p - d) & (2 * LANES - 1)] == h) { best = match_len(sh.in, p - d, p, maxlen); bdist = d; break; }
                        }
                        const uint32_t c = sh.head[h];
                        if (c && p - (c - 1u) <= MAX_DIST && best < maxlen) {
                            const uint32_t fl = match_len(sh.in, c - 1u, p, maxlen);
                            if (fl > best) { best = fl; bdist = p - (c - 1u); }
                        }
                        if (best < 3 || (best == 3 && bdist > 4096)) { best = 0; bdist = 1; }
                    }
                    sh.m[p - bs] = best ? (best << 16 | (bdist - 1u)) : 0u;
                }
            }
            BRCD_SYNC();
        }
        // ---- parse (lane 0), and the tables of the block cleared by everyone
        BRCD_FOR_LANES(l) {
            for (int i = l; i < 320; i += LANES) { sh.hist[i] = i == 256 ? 1u : 0u; sh.lens[i] = 0; sh.code[i] = 0; }
            if (l < 3) sh.cost[l] = 0;
            if (l < 2) sh.nused[l] = 0;
        }
        BRCD_LANE(0) {
            uint32_t k = 0, p = 0;
            while (p < blen) {
                const uint32_t t = sh.m[p], len = t >> 16;
                if (len >= 3) { sh.m[k++] = t; p += len; } else { sh.m[k++] = TOK_LIT | sh.in[bs + p]; ++p; }
            }
            sh.ntok = k;
        }
        BRCD_SYNC();
        const uint32_t ntok = sh.ntok;
        BRCD_FOR_LANES(l) {
            for (uint32_t k = (uint32_t)l; k < ntok; k += LANES) {
                const uint32_t t = sh.m[k];
                if (t & TOK_LIT) BRCD_ADD(&sh.hist[t & 0xffu], 1u);
                else { BRCD_ADD(&sh.hist[257 + len_code(t >> 16)], 1u); BRCD_ADD(&sh.hist[DBASE + dist_code((t & 0xffffu) + 1u)], 1u); }
            }
        }
        BRCD_SYNC();
        // ---- the used symbols of both alphabets ranked by (count, symbol)
        BRCD_FOR_LANES(l) {
            for (uint32_t i = (uint32_t)l; i < 320; i += LANES) {
                const uint32_t base = i < DBASE ? 0u : DBASE, ns = i < DBASE ? 286u : 30u, f = sh.hist[i];
                if (i - base >= ns || !f) continue;
                uint32_t rank = 0;
                for (uint32_t j = 0; j < ns; ++j) { const uint32_t g = sh.hist[base + j]; rank += (g && (g < f || (g == f && base + j < i))) ? 1u : 0u; }
                sh.sorted[base + rank] = (uint16_t)(i - base); sh.A[base + rank] = f;
                BRCD_ADD(&sh.nused[base ? 1 : 0], 1u);
            }
        }
        BRCD_SYNC();
        BRCD_LANE(0) { limited_lengths(sh.A, sh.sorted, sh.num[0], sh.lens, (int)sh.nused[0], 15); }
        BRCD_LANE(64) {
            limited_lengths(sh.A + DBASE, sh.sorted + DBASE, sh.num[1], sh.lens + DBASE, (int)sh.nused[1], 15);
            // (a single distance code: a second one-bit code next to it makes the set complete for every decoder)
            if (sh.nused[1] == 1) sh.lens[DBASE + (sh.sorted[DBASE] == 0 ? 1 : 0)] = 1;
        }
        BRCD_SYNC();
        // ---- lane 0: the lengths as symbols 0..18 with runs, the code-length code, the size of the dynamic header
        BRCD_LANE(0) {
            uint32_t hlit = 286, hdist = 30;
            while (hlit > 257 && sh.lens[hlit - 1] == 0) --hlit;
            while (hdist > 1 && sh.lens[DBASE + hdist - 1] == 0) --hdist;
            const uint32_t total = hlit + hdist;
            uint32_t clh[19]; for (int i = 0; i < 19; ++i) clh[i] = 0;
            uint32_t nr = 0, i = 0;
            while (i < total) {
                const uint32_t v = sh.lens[i < hlit ? i : DBASE + (i - hlit)];
                uint32_t run = 1;
                while (i + run < total && sh.lens[i + run < hlit ? i + run : DBASE + (i + run - hlit)] == v) ++run;
                i += run;
                if (v == 0) {
                    while (run >= 11) { const uint32_t r = run < 138 ? run : 138; sh.rle_sym[nr] = 18; sh.rle_extra[nr++] = (uint8_t)(r - 11); ++clh[18]; run -= r; }
                    if (run >= 3) { sh.rle_sym[nr] = 17; sh.rle_extra[nr++] = (uint8_t)(run - 3); ++clh[17]; run = 0; }
                    while (run) { sh.rle_sym[nr] = 0; sh.rle_extra[nr++] = 0; ++clh[0]; --run; }
                } else {
                    sh.rle_sym[nr] = (uint8_t)v; sh.rle_extra[nr++] = 0; ++clh[v]; --run;
                    while (run >= 3) { const uint32_t r = run < 6 ? run : 6; sh.rle_sym[nr] = 16; sh.rle_extra[nr++] = (uint8_t)(r - 3); ++clh[16]; run -= r; }
                    while (run) { sh.rle_sym[nr] = (uint8_t)v; sh.rle_extra[nr++] = 0; ++clh[v]; --run; }
                }
            }
            // the code-length code: 19 symbols, 7 bits; an insertion sort by (count, symbol)
            int nu = 0;
            for (int s = 0; s < 19; ++s) {
                sh.cllens[s] = 0; sh.clcode[s] = 0;
                if (!clh[s]) continue;
                int k = nu++;
                while (k > 0 && sh.clA[k - 1] > clh[s]) { sh.clA[k] = sh.clA[k - 1]; sh.clsorted[k] = sh.clsorted[k - 1]; --k; }
                sh.clA[k] = clh[s]; sh.clsorted[k] = (uint16_t)s;
            }
            uint32_t body = 0;
            for (int k = 0; k < nu; ++k) body += sh.clA[k] * (sh.clsorted[k] == 16 ? 2u : sh.clsorted[k] == 17 ? 3u : sh.clsorted[k] == 18 ? 7u : 0u);
            uint32_t keep[19]; for (int k = 0; k < nu; ++k) keep[k] = sh.clA[k];
            limited_lengths(sh.clA, sh.clsorted, sh.num[2], sh.cllens, nu, 7);
            if (nu == 1) sh.cllens[sh.clsorted[0] == 0 ? 1 : 0] = 1;       // (an incomplete code-length code is refused by decoders)
            for (int k = 0; k < nu; ++k) body += keep[k] * sh.cllens[sh.clsorted[k]];
            {   // canonical codes of the code-length code
                uint32_t code = 0;
                for (uint32_t ln = 1; ln <= 7; ++ln) { for (int s = 0; s < 19; ++s) if (sh.cllens[s] == ln) sh.clcode[s] = (uint16_t)rev_bits(code++, ln); code <<= 1; }
            }
            const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
            uint32_t hclen = 19;
            while (hclen > 4 && sh.cllens[order[hclen - 1]] == 0) --hclen;
            sh.nrle = nr; sh.hlit = hlit; sh.hdist = hdist; sh.hclen = hclen;
            sh.hdr_bits = 3 + 5 + 5 + 4 + 3 * hclen + body;
        }
        // (meanwhile) the cost of the block's symbols under the dynamic and the fixed code, and their extra bits
        BRCD_FOR_LANES(l) {
            for (uint32_t i = (uint32_t)l; i < 320; i += LANES) {
                const uint32_t f = sh.hist[i];
                if (!f) continue;
                BRCD_ADD(&sh.cost[0], f * sh.lens[i]); BRCD_ADD(&sh.cost[1], f * fixed_len(i)); BRCD_ADD(&sh.cost[2], f * extra_bits(i));
            }
            if (l < 32) sh.cnt[l >> 4][l & 15] = 0;
        }
        BRCD_SYNC();
        BRCD_LANE(0) {
            const uint32_t bp = sh.bitpos;
            const uint32_t dyn = sh.hdr_bits + sh.cost[0] + sh.cost[2], fix = 3 + sh.cost[1] + sh.cost[2];
            const uint32_t sto = 3 + ((8u - ((bp + 3u) & 7u)) & 7u) + 32 + 8 * blen;
            sh.btype = (dyn < fix && dyn < sto) ? 2u : (fix < sto ? 1u : 0u);
        }
        BRCD_SYNC();
        const uint32_t btype = sh.btype, bp0 = sh.bitpos;
        if (btype == 0) {
            // ---- stored: header bits, up to the next byte, LEN, ~LEN, the bytes
            const uint32_t at = HDR + (bp0 + 3u + 7u) / 8u;
            BRCD_LANE(0) {
                put(slot, HDR * 8 + bp0, last, 3);
                out8[at] = (uint8_t)blen; out8[at + 1] = (uint8_t)(blen >> 8); out8[at + 2] = (uint8_t)~blen; out8[at + 3] = (uint8_t)(~blen >> 8);
            }
            BRCD_FOR_LANES(l) { for (uint32_t i = (uint32_t)l; i < blen; i += LANES) out8[at + 4 + i] = sh.in[bs + i]; }
            BRCD_SYNC();                                      // every lane has read sh.bitpos (bp0) before lane 0 moves it
            BRCD_LANE(0) { sh.bitpos = (at - HDR + 4 + blen) * 8; }
            BRCD_SYNC();
            continue;
        }
        if (btype == 1) {
            BRCD_FOR_LANES(l) { for (uint32_t i = (uint32_t)l; i < 320; i += LANES) sh.lens[i] = (uint8_t)fixed_len(i); }
            BRCD_SYNC();
        }
        // ---- canonical codes: lane L < 16 counts the literal/length codes of length L, lanes 16..31 the distance codes
        BRCD_FOR_LANES(l) {
            if (l < 32) {
                const uint32_t base = l < 16 ? 0u : DBASE, ns = l < 16 ? 288u : 32u, ln = (uint32_t)l & 15u;
                uint32_t c = 0;
                if (ln) for (uint32_t s = 0; s < ns; ++s) c += sh.lens[base + s] == ln ? 1u : 0u;
                sh.cnt[l >> 4][ln] = c;
            }
        }
        BRCD_SYNC();
        BRCD_FOR_LANES(l) {
            for (uint32_t i = (uint32_t)l; i < 320; i += LANES) {
                const uint32_t base = i < DBASE ? 0u : DBASE, ln = sh.lens[i];
                if (!ln) continue;
                uint32_t first = 0;
                for (uint32_t q = 1; q < ln; ++q) first = (first + sh.cnt[base ? 1 : 0][q]) << 1;
                uint32_t k = 0;
                for (uint32_t s = base; s < i; ++s) k += sh.lens[s] == ln ? 1u : 0u;
                sh.code[i] = (uint16_t)rev_bits(first + k, ln);
            }
        }
        BRCD_SYNC();
        // ---- emit: the header (lane 0), every lane's share of the tokens at its own bit offset, the end-of-block code
        const uint32_t per = (ntok + LANES - 1) / LANES;
        BRCD_FOR_LANES(l) {
            uint32_t k0 = (uint32_t)l * per, k1 = k0 + per, bits = 0;
            if (k1 > ntok) k1 = ntok;
            for (uint32_t k = k0; k < k1; ++k) { uint32_t v1, n1, v2, n2; token_fields(sh, sh.m[k], &v1, &n1, &v2, &n2); bits += n1 + n2; }
            sh.lane_bits[l] = bits;
        }
        BRCD_SYNC();
        BRCD_LANE(0) {
            uint32_t bit = HDR * 8 + bp0;
            put(slot, bit, last | btype << 1, 3); bit += 3;
            if (btype == 2) {
                const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
                put(slot, bit, sh.hlit - 257, 5); bit += 5;
                put(slot, bit, sh.hdist - 1, 5); bit += 5;
                put(slot, bit, sh.hclen - 4, 4); bit += 4;
                for (uint32_t i = 0; i < sh.hclen; ++i) { put(slot, bit, sh.cllens[order[i]], 3); bit += 3; }
                for (uint32_t i = 0; i < sh.nrle; ++i) {
                    const uint32_t s = sh.rle_sym[i], eb = s == 16 ? 2u : s == 17 ? 3u : s == 18 ? 7u : 0u;
                    put(slot, bit, sh.clcode[s], sh.cllens[s]); bit += sh.cllens[s];
                    put(slot, bit, sh.rle_extra[i], eb); bit += eb;
                }
            }
            uint32_t run = bit;
            for (int i = 0; i < LANES; ++i) { const uint32_t b = sh.lane_bits[i]; sh.lane_bits[i] = run; run += b; }
            put(slot, run, sh.code[256], sh.lens[256]); run += sh.lens[256];
            sh.bitpos = run - HDR * 8;
        }
        BRCD_SYNC();
        BRCD_FOR_LANES(l) {
            uint32_t k0 = (uint32_t)l * per, k1 = k0 + per, bit = sh.lane_bits[l];
            if (k1 > ntok) k1 = ntok;
            for (uint32_t k = k0; k < k1; ++k) {
                uint32_t v1, n1, v2, n2; token_fields(sh, sh.m[k], &v1, &n1, &v2, &n2);
                put(slot, bit, v1, n1); bit += n1;
                put(slot, bit, v2, n2); bit += n2;
            }
        }
        BRCD_SYNC();
    }
    // ---- a stream that is no shorter than the stored form: one stored block instead
    uint32_t stream = (sh.bitpos + 7u) / 8u;
    if (n == 0) { BRCD_LANE(0) { out8[HDR] = 3; out8[HDR + 1] = 0; } stream = 2; }        // (no input: an empty fixed-code block)
    else if (stream >= n + 5u) {
        BRCD_LANE(0) { out8[HDR] = 1; out8[HDR + 1] = (uint8_t)n; out8[HDR + 2] = (uint8_t)(n >> 8); out8[HDR + 3] = (uint8_t)~n; out8[HDR + 4] = (uint8_t)(~n >> 8); }
        BRCD_FOR_LANES(l) { for (uint32_t i = (uint32_t)l; i < n; i += LANES) out8[HDR + 5 + i] = sh.in[i]; }
        stream = n + 5u;
    }
    const uint32_t total = HDR + stream + TRAILER;
    BRCD_LANE(0) {
        const uint8_t hd[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
        for (int i = 0; i < 16; ++i) out8[i] = hd[i];
        out8[16] = (uint8_t)(total - 1); out8[17] = (uint8_t)((total - 1) >> 8);
        uint8_t* t = out8 + HDR + stream;
        const uint32_t crc = sh.crc;
        t[0] = (uint8_t)crc; t[1] = (uint8_t)(crc >> 8); t[2] = (uint8_t)(crc >> 16); t[3] = (uint8_t)(crc >> 24);
        t[4] = (uint8_t)n; t[5] = (uint8_t)(n >> 8); t[6] = 0; t[7] = 0;
    }
    BRCD_SYNC();
    return total;
}

// ---- the host side of every build
constexpr uint32_t EOF_LEN = 28;
static inline const uint8_t* eof_member() {    // the BGZF end-of-file member (SAMv1 4.1.2): an empty fixed-code block
    static const uint8_t e[EOF_LEN] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    return e;
}
static inline size_t n_members(size_t src_len) { return (src_len + MEMBER_IN - 1) / MEMBER_IN; }
static inline size_t bound(size_t src_len) { return src_len + n_members(src_len) * (size_t)(HDR + 5 + TRAILER); }

}  // namespace brcdef
#endif
