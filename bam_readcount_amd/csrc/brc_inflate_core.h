// brc_inflate_core.h — raw-deflate (RFC 1951) decoding of one BGZF member (SAMv1 4.1; a gzip member, RFC 1952, of at most 64 KB
// of output) by ONE WAVE of 64 lanes, written once for the device and for the host: brc_inflate.hip runs inflate_member() with one
// wave per member, tests/sim_inflate runs the very same function with the lanes of every parallel phase executed one after the other.
//
// Written from RFC 1951 / RFC 1952 and the BGZF section of the SAM specification; no code of any inflate library is involved.
//
// How the work is divided:
//   * the Huffman SYMBOL STREAM is serial: lane 0 decodes it, up to NTOK tokens at a time, into a token list in LDS;
//   * everything else is done by the wave: the CRC table, the code-length histogram / sort / lookup tables of every block
//     (build_huff), stored-block copies, the literals of a token batch (one lane each), every match copy (64 bytes per step,
//     `j % dist` resolves a match that overlaps its own output), the CRC32 of the output (one segment per lane, advanced by the
//     zero bytes behind it — multiplication by x^(8n) modulo the CRC polynomial — and XORed together) and the copy of the
//     finished window to memory in 16-byte stores;
//   * the member's output window lives in LDS until it is complete and its CRC32 is right: nothing partial reaches `dst`.
//
// The decoder is TOTAL: for any bytes it ends with a status.  It reads src[0, clen) only (BitReader::refill is the one place that
// reads input, bounded by clen; stored copies are checked against clen first) and writes win[0, isize) / dst[0, isize) only (every
// token is checked against isize before it is listed).  Loop bounds: blocks <= clen * 8 / 3 + 1 (a block header takes 3 bits),
// token batches <= clen * 8 + 2 (a symbol takes at least one bit and a batch lists at least one symbol or ends the block), copies
// by the checked lengths.
#ifndef BRC_INFLATE_CORE_H
#define BRC_INFLATE_CORE_H

#include <stdint.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define BRCI_HD __host__ __device__ __forceinline__
#define BRCI_HDM __host__ __device__ __forceinline__      // (member functions)
#else
#define BRCI_HD static inline __attribute__((always_inline))
#define BRCI_HDM inline __attribute__((always_inline))
#endif

// A parallel phase: on the device every lane runs the body once with its own index, on the host the lanes run one after the other.
// Phases never read what another lane writes in the same phase, so both orders give the same bytes.
#if defined(__HIP_DEVICE_COMPILE__)
#define BRCI_FOR_LANES(l) for (int l = (int)threadIdx.x, brci_once_ = 1; brci_once_; brci_once_ = 0)
#define BRCI_LANE0 if (threadIdx.x == 0)
#define BRCI_SYNC() __syncthreads()
#else
#define BRCI_FOR_LANES(l) for (int l = 0; l < brcinf::LANES; ++l)
#define BRCI_LANE0 if (true)
#define BRCI_SYNC() ((void)0)
#endif

namespace brcinf {

enum Status { ST_OK = 0, ST_BAD_HEADER = 1, ST_BAD_STREAM = 2, ST_SIZE_MISMATCH = 3, ST_CRC_MISMATCH = 4, ST_TRUNCATED = 5 };

constexpr int LANES = 64;
constexpr uint32_t WINDOW = 65536;        // BGZF: ISIZE <= 65536
constexpr int NTOK = 64;                  // tokens lane 0 lists before the wave executes them
constexpr int LIT_FAST = 10, DIST_FAST = 8;   // bits of the one-step lookup tables
constexpr uint32_t TOK_LIT = 0x80000000u;

// Canonical Huffman code (RFC 1951 3.2.2): count[l] codes of length l, symbol[] sorted by (length, value); fast[] maps the next FAST
// bits of the stream to (symbol << 4 | length) for codes of at most FAST bits (0: longer code or no code — decode() walks the lengths)
template <int NSYM, int FAST> struct Huff { uint16_t count[16], offs[16], first[16]; uint16_t symbol[NSYM]; uint16_t fast[1 << FAST]; };

struct Shared {
    uint8_t win[WINDOW];
    uint32_t crc_tab[256];
    uint32_t tok[NTOK]; uint16_t tokpos[NTOK];
    uint8_t lens[320];                     // code lengths of the block: literal/length symbols, then distance symbols
    uint8_t cl_lens[32];                   // ... of the code-length code (19 used)
    Huff<288, LIT_FAST> lit; Huff<32, DIST_FAST> dist;
    uint32_t part[LANES];                  // per-lane CRC states
    // what lane 0 tells the wave
    uint32_t status, pos, mode, final_block, ntok, eob, a, b, nlen, ndist;
};

struct BitReader {
    const uint8_t* src; uint32_t clen, inpos; uint64_t buf; uint32_t cnt;
    BRCI_HDM void init(const uint8_t* s, uint32_t n) { src = s; clen = n; inpos = 0; buf = 0; cnt = 0; }
    BRCI_HDM void refill() { while (cnt <= 56 && inpos < clen) { buf |= (uint64_t)src[inpos++] << cnt; cnt += 8; } }
    // n <= 32 bits; false: the input ends first
    BRCI_HDM bool take(uint32_t n, uint32_t* out) {
        if (cnt < n) { refill(); if (cnt < n) return false; }
        *out = (uint32_t)(buf & ((1ull << n) - 1)); buf >>= n; cnt -= n; return true;
    }
    BRCI_HDM void align_byte() { const uint32_t k = cnt & 7; buf >>= k; cnt -= k; }
    // (stored blocks) bytes still unread, counting whole bytes waiting in buf; and the offset in src of the next unread byte
    BRCI_HDM uint32_t byte_pos() const { return inpos - cnt / 8; }
    BRCI_HDM void skip_bytes_from(uint32_t p) { inpos = p; buf = 0; cnt = 0; }
};

// ---- wave-built code tables.  lens[0, n): code lengths 0..15.  Returns through *status (lane 0 writes): over-subscribed sets and
// incomplete sets are refused, except the two incomplete sets the format allows: no code at all (allow_empty: a block without
// matches has no distance code) and a single code of one bit.
template <int NSYM, int FAST>
BRCI_HD void build_huff(Shared& sh, Huff<NSYM, FAST>& h, const uint8_t* lens, int n, bool allow_empty) {
    BRCI_FOR_LANES(l) {                                       // histogram: lane L counts the codes of length L
        if (l < 16) { uint32_t c = 0; for (int s = 0; s < n; ++s) c += (lens[s] == l) ? 1u : 0u; h.count[l] = (uint16_t)c; }
        for (int i = l; i < (1 << FAST); i += LANES) h.fast[i] = 0;
    }
    BRCI_SYNC();
    BRCI_LANE0 {
        int left = 1; uint32_t off = 0, code = 0, used = 0, maxl = 0;
        h.offs[0] = 0; h.first[0] = 0;
        for (int l = 1; l < 16; ++l) {
            left <<= 1; left -= (int)h.count[l];
            if (left < 0) { if (sh.status == ST_OK) sh.status = ST_BAD_STREAM; left = 0; }        // over-subscribed
            code = (code + (l > 1 ? h.count[l - 1] : 0u)) << 1;
            h.first[l] = (uint16_t)code; h.offs[l] = (uint16_t)off; off += h.count[l]; used += h.count[l];
            if (h.count[l]) maxl = (uint32_t)l;
        }
        if (left > 0 && !(used == 0 ? allow_empty : (used == 1 && maxl == 1)) && sh.status == ST_OK) sh.status = ST_BAD_STREAM;   // incomplete
    }
    BRCI_SYNC();
    BRCI_FOR_LANES(l) {                                       // sort: lane L places the symbols of length L, in symbol order
        if (l >= 1 && l < 16 && h.count[l]) { uint32_t k = h.offs[l]; for (int s = 0; s < n; ++s) if (lens[s] == l && k < (uint32_t)NSYM) h.symbol[k++] = (uint16_t)s; }
    }
    BRCI_SYNC();
    BRCI_FOR_LANES(l) {                                       // lookup table: the lanes share the sorted symbols
        uint32_t total = 0; for (int q = 1; q < 16; ++q) total += h.count[q];
        if (total > (uint32_t)NSYM) total = NSYM;
        for (uint32_t i = (uint32_t)l; i < total; i += LANES) {
            const uint32_t s = h.symbol[i]; const uint32_t ln = lens[s];
            if (ln == 0 || ln > (uint32_t)FAST) continue;
            const uint32_t code = (uint32_t)h.first[ln] + (i - h.offs[ln]);
            if (code >> ln) continue;                         // (only in an over-subscribed set, which is refused anyway)
            uint32_t rev = 0; for (uint32_t b = 0; b < ln; ++b) rev |= ((code >> b) & 1u) << (ln - 1 - b);    // the stream carries codes MSB first
            for (uint32_t k = rev; k < (1u << FAST); k += 1u << ln) h.fast[k] = (uint16_t)(s << 4 | ln);
        }
    }
    BRCI_SYNC();
}

// next symbol, or -1 (no such code), -2 (input ends)
template <int NSYM, int FAST>
BRCI_HD int decode(const Huff<NSYM, FAST>& h, BitReader& br) {
    if (br.cnt < 15) br.refill();
    const uint32_t e = h.fast[br.buf & ((1u << FAST) - 1)];
    if (e) { const uint32_t ln = e & 15u; if (ln > br.cnt) return -2; br.buf >>= ln; br.cnt -= ln; return (int)(e >> 4); }
    uint32_t code = 0, first = 0, index = 0;
    for (uint32_t ln = 1; ln < 16; ++ln) {
        if (br.cnt < ln) return -2;
        code |= (uint32_t)(br.buf >> (ln - 1)) & 1u;
        const uint32_t c = h.count[ln];
        if (code - first < c && code >= first) { const uint32_t k = index + (code - first); br.buf >>= ln; br.cnt -= ln; return k < (uint32_t)NSYM ? (int)h.symbol[k] : -1; }
        index += c; first += c; first <<= 1; code <<= 1;
    }
    return -1;
}

// ---- CRC-32 (RFC 1952 8), reflected polynomial 0xedb88320
BRCI_HD uint32_t gf2_mul(uint32_t a, uint32_t b) {             // a * b modulo the CRC polynomial, bit-reflected operands
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) { if (a & (0x80000000u >> i)) p ^= b; b = (b & 1u) ? (b >> 1) ^ 0xedb88320u : b >> 1; }
    return p;
}
BRCI_HD uint32_t crc_advance_zeros(uint32_t state, uint32_t nbytes) {   // the register after nbytes more zero bytes: state * x^(8 nbytes)
    uint32_t r = 0x80000000u, q = 0x00800000u;                 // x^0, x^8
    for (int i = 0; i < 18; ++i) { if (nbytes & 1u) r = gf2_mul(r, q); q = gf2_mul(q, q); nbytes >>= 1; }
    return gf2_mul(state, r);
}

BRCI_HD uint16_t len_base(uint32_t k) { const uint16_t t[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258}; return t[k]; }
BRCI_HD uint8_t len_extra(uint32_t k) { return (k < 8 || k == 28) ? 0 : (uint8_t)((k - 4) >> 2); }
BRCI_HD uint32_t dist_base(uint32_t k) { return k < 4 ? k + 1 : ((2u + (k & 1u)) << ((k >> 1) - 1)) + 1; }
BRCI_HD uint8_t dist_extra(uint32_t k) { return k < 4 ? 0 : (uint8_t)((k >> 1) - 1); }

// One member.  src[0, clen): the raw-deflate payload; dst[0, isize): the member's slot (written only when the status is ok);
// want_crc: the CRC32 of the trailer.  Every lane of the wave calls this (the host: one call runs all lanes); returns the status.
BRCI_HD int inflate_member(Shared& sh, const uint8_t* src, uint32_t clen, uint8_t* dst, uint32_t isize, uint32_t want_crc) {
    BitReader br; br.init(src, clen);
    if (isize > WINDOW) return ST_BAD_HEADER;
    BRCI_FOR_LANES(l) {
        for (int i = l; i < 256; i += LANES) { uint32_t c = (uint32_t)i; for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ 0xedb88320u : c >> 1; sh.crc_tab[i] = c; }
    }
    BRCI_LANE0 { sh.status = ST_OK; sh.pos = 0; sh.final_block = 0; }
    BRCI_SYNC();
    const uint32_t max_blocks = clen * 8u / 3u + 1u, max_batches = clen * 8u + 2u;
    for (uint32_t blk = 0; blk < max_blocks; ++blk) {
        BRCI_LANE0 {                                          // block header (RFC 1951 3.2.3)
            uint32_t v = 0; sh.mode = 3;
            if (!br.take(3, &v)) sh.status = ST_TRUNCATED;
            else {
                sh.final_block = v & 1u; sh.mode = v >> 1;
                if (sh.mode == 3) sh.status = ST_BAD_STREAM;
                else if (sh.mode == 0) {                      // stored: LEN, ~LEN on a byte boundary, then LEN bytes
                    br.align_byte();
                    uint32_t ln = 0, nl = 0;
                    if (!br.take(16, &ln) || !br.take(16, &nl)) sh.status = ST_TRUNCATED;
                    else if ((ln ^ nl) != 0xffffu) sh.status = ST_BAD_STREAM;
                    else {
                        const uint32_t p = br.byte_pos();
                        if (ln > clen - p) sh.status = ST_TRUNCATED;
                        else if (ln > isize - sh.pos) sh.status = ST_SIZE_MISMATCH;
                        else { sh.a = p; sh.b = ln; br.skip_bytes_from(p + ln); }
                    }
                } else if (sh.mode == 2) {                    // dynamic: HLIT, HDIST, HCLEN and the code-length code's lengths
                    uint32_t hl = 0, hd = 0, hc = 0;
                    if (!br.take(5, &hl) || !br.take(5, &hd) || !br.take(4, &hc)) sh.status = ST_TRUNCATED;
                    else if (hl + 257 > 286 || hd + 1 > 30) sh.status = ST_BAD_STREAM;
                    else {
                        const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
                        sh.nlen = hl + 257; sh.ndist = hd + 1;
                        for (int i = 0; i < 19; ++i) sh.cl_lens[i] = 0;
                        for (uint32_t i = 0; i < hc + 4 && sh.status == ST_OK; ++i) { uint32_t x = 0; if (!br.take(3, &x)) sh.status = ST_TRUNCATED; else sh.cl_lens[order[i]] = (uint8_t)x; }
                    }
                }
            }
        }
        BRCI_SYNC();
        if (sh.status != ST_OK) break;
        const uint32_t mode = sh.mode, final_block = sh.final_block;
        if (mode == 0) {
            const uint32_t a = sh.a, n = sh.b, p = sh.pos;
            BRCI_FOR_LANES(l) { for (uint32_t i = (uint32_t)l; i < n; i += LANES) sh.win[p + i] = src[a + i]; }
            BRCI_SYNC();
            BRCI_LANE0 { sh.pos = p + n; }
            BRCI_SYNC();
        } else {
            if (mode == 2) {
                build_huff(sh, sh.dist, sh.cl_lens, 19, false);       // (the code-length code borrows the distance tables: 19 symbols, 7 bits)
                BRCI_LANE0 {
                    if (sh.status == ST_OK) {
                        const uint32_t total = sh.nlen + sh.ndist; uint32_t i = 0;
                        while (i < total) {                   // (every pass consumes at least one bit or ends)
                            const int s = decode(sh.dist, br);
                            if (s < 0) { sh.status = s == -2 ? ST_TRUNCATED : ST_BAD_STREAM; break; }
                            if (s < 16) { sh.lens[i++] = (uint8_t)s; continue; }
                            uint32_t rep = 0, x = 0; uint8_t val = 0;
                            if (s == 16) { if (i == 0) { sh.status = ST_BAD_STREAM; break; } val = sh.lens[i - 1]; if (!br.take(2, &x)) { sh.status = ST_TRUNCATED; break; } rep = 3 + x; }
                            else if (s == 17) { if (!br.take(3, &x)) { sh.status = ST_TRUNCATED; break; } rep = 3 + x; }
                            else if (s == 18) { if (!br.take(7, &x)) { sh.status = ST_TRUNCATED; break; } rep = 11 + x; }
                            else { sh.status = ST_BAD_STREAM; break; }
                            if (rep > total - i) { sh.status = ST_BAD_STREAM; break; }
                            for (uint32_t k = 0; k < rep; ++k) sh.lens[i++] = val;
                        }
                        if (sh.status == ST_OK && sh.lens[256] == 0) sh.status = ST_BAD_STREAM;      // no end-of-block code
                    }
                }
                BRCI_SYNC();
            } else {                                          // fixed codes (RFC 1951 3.2.6); 286/287 and 30/31 take part in the code and are refused when met
                BRCI_FOR_LANES(l) {
                    for (int i = l; i < 320; i += LANES) sh.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
                }
                BRCI_LANE0 { sh.nlen = 288; sh.ndist = 32; }
                BRCI_SYNC();
            }
            if (sh.status != ST_OK) break;
            build_huff(sh, sh.lit, sh.lens, (int)sh.nlen, false);
            build_huff(sh, sh.dist, sh.lens + sh.nlen, (int)sh.ndist, true);
            if (sh.status != ST_OK) break;
            uint32_t eob = 0;
            for (uint32_t batch = 0; batch < max_batches; ++batch) {
                BRCI_LANE0 {                                  // the serial part: symbols -> tokens
                    uint32_t n = 0, pos = sh.pos; sh.eob = 0;
                    while (n < (uint32_t)NTOK) {
                        const int s = decode(sh.lit, br);
                        if (s < 0) { sh.status = s == -2 ? ST_TRUNCATED : ST_BAD_STREAM; break; }
                        if (s < 256) {
                            if (pos >= isize) { sh.status = ST_SIZE_MISMATCH; break; }
                            sh.tok[n] = TOK_LIT | (uint32_t)s; sh.tokpos[n] = (uint16_t)pos; ++n; ++pos; continue;
                        }
                        if (s == 256) { sh.eob = 1; break; }
                        if (s > 285) { sh.status = ST_BAD_STREAM; break; }
                        uint32_t x = 0, y = 0;
                        const uint32_t li = (uint32_t)s - 257u;
                        if (!br.take(len_extra(li), &x)) { sh.status = ST_TRUNCATED; break; }
                        const uint32_t len = len_base(li) + x;
                        const int d = decode(sh.dist, br);
                        if (d < 0) { sh.status = d == -2 ? ST_TRUNCATED : ST_BAD_STREAM; break; }
                        if (d > 29) { sh.status = ST_BAD_STREAM; break; }
                        if (!br.take(dist_extra((uint32_t)d), &y)) { sh.status = ST_TRUNCATED; break; }
                        const uint32_t dist = dist_base((uint32_t)d) + y;
                        if (dist > pos) { sh.status = ST_BAD_STREAM; break; }          // reaches before the member's output
                        if (len > isize - pos) { sh.status = ST_SIZE_MISMATCH; break; }
                        sh.tok[n] = len << 16 | dist; sh.tokpos[n] = (uint16_t)pos; ++n; pos += len;
                    }
                    sh.ntok = n; sh.pos = pos;
                }
                BRCI_SYNC();
                if (sh.status != ST_OK) break;
                const uint32_t ntok = sh.ntok; eob = sh.eob;
                BRCI_FOR_LANES(l) { if ((uint32_t)l < ntok && (sh.tok[l] & TOK_LIT)) sh.win[sh.tokpos[l]] = (uint8_t)sh.tok[l]; }     // literals: one lane each
                BRCI_SYNC();
                for (uint32_t k = 0; k < ntok; ++k) {         // matches in stream order, each copied by the wave
                    const uint32_t t = sh.tok[k];
                    if (t & TOK_LIT) continue;
                    const uint32_t len = t >> 16, dist = t & 0xffffu, p = sh.tokpos[k];
                    BRCI_FOR_LANES(l) {
                        for (uint32_t j = (uint32_t)l; j < len; j += LANES) sh.win[p + j] = sh.win[p - dist + (dist >= len ? j : j % dist)];
                    }
                    BRCI_SYNC();
                }
                BRCI_SYNC();                                  // every lane has read this batch's list before lane 0 writes the next (free for one wave; needed as soon as a workgroup is more than one)
                if (eob) break;
                if (ntok == 0) { BRCI_LANE0 { sh.status = ST_BAD_STREAM; } BRCI_SYNC(); break; }    // (cannot happen: a batch without tokens ends its block or fails)
            }
            if (sh.status != ST_OK) break;
            if (!eob) { BRCI_LANE0 { sh.status = ST_BAD_STREAM; } BRCI_SYNC(); break; }
        }
        BRCI_SYNC();                                          // (the same: sh.status / sh.mode of this block are read, the next header may be written)
        if (final_block) break;
    }
    BRCI_SYNC();
    BRCI_LANE0 {
        if (sh.status == ST_OK && !sh.final_block) sh.status = ST_TRUNCATED;          // (the block bound ran out)
        if (sh.status == ST_OK && sh.pos != isize) sh.status = ST_SIZE_MISMATCH;
    }
    BRCI_SYNC();
    if (sh.status != ST_OK) return (int)sh.status;
    // CRC32 of the window: lane l takes bytes [l * seg, (l + 1) * seg), advances its register over the bytes behind it
    const uint32_t seg = (isize + LANES - 1) / LANES;
    BRCI_FOR_LANES(l) {
        uint32_t b = (uint32_t)l * seg; if (b > isize) b = isize;
        uint32_t e = b + seg; if (e > isize) e = isize;
        uint32_t c = l == 0 ? 0xffffffffu : 0u;
        for (uint32_t i = b; i < e; ++i) c = sh.crc_tab[(c ^ sh.win[i]) & 0xffu] ^ (c >> 8);
        sh.part[l] = crc_advance_zeros(c, isize - e);
    }
    BRCI_SYNC();
    BRCI_LANE0 { uint32_t c = 0; for (int i = 0; i < LANES; ++i) c ^= sh.part[i]; if ((c ^ 0xffffffffu) != want_crc) sh.status = ST_CRC_MISMATCH; }
    BRCI_SYNC();
    if (sh.status != ST_OK) return (int)sh.status;
    // the window -> memory: bytes up to the first 16-byte boundary of dst, 16-byte stores, the rest
    {
        uint32_t head = (uint32_t)((16u - ((uintptr_t)dst & 15u)) & 15u); if (head > isize) head = isize;
        const uint32_t nvec = (isize - head) / 16u, tail0 = head + nvec * 16u;
        BRCI_FOR_LANES(l) {
            if ((uint32_t)l < head) dst[l] = sh.win[l];
            for (uint32_t v = (uint32_t)l; v < nvec; v += LANES) {
                const uint8_t* w = sh.win + head + v * 16u;
                uint32_t x[4];
                for (int q = 0; q < 4; ++q) x[q] = (uint32_t)w[4 * q] | (uint32_t)w[4 * q + 1] << 8 | (uint32_t)w[4 * q + 2] << 16 | (uint32_t)w[4 * q + 3] << 24;
                uint32_t* o = (uint32_t*)(dst + head + v * 16u);
#if defined(__HIP_DEVICE_COMPILE__)
                *(uint4*)o = make_uint4(x[0], x[1], x[2], x[3]);
#else
                typedef uint32_t v4 __attribute__((vector_size(16)));                 // (the host's 16-byte store asks for the same alignment:
                *(v4*)o = v4{x[0], x[1], x[2], x[3]};                                  //  a wrong `head` is a sanitizer report there too)
#endif
            }
            if (tail0 + (uint32_t)l < isize) dst[tail0 + l] = sh.win[tail0 + l];
        }
    }
    return ST_OK;
}

// ---- the member chain (host side of every build).  One BGZF member header at p[0, avail): 0 = ok (*total = BSIZE + 1 bytes, *hdr =
// bytes before the payload), 1 = not a member that can be stepped over (magic, FEXTRA, no BC subfield), 2 = the bytes end first.
BRCI_HD int member_header(const uint8_t* p, size_t avail, uint32_t* total, uint32_t* hdr) {
    if (avail < 18) return 2;
    if (p[0] != 31 || p[1] != 139 || p[2] != 8 || !(p[3] & 4)) return 1;
    const uint32_t xlen = (uint32_t)p[10] | (uint32_t)p[11] << 8;
    if (avail < 12u + xlen) return 2;
    int bsize = -1;
    for (uint32_t o = 0; o + 4 <= xlen;) {
        const uint32_t slen = (uint32_t)p[12 + o + 2] | (uint32_t)p[12 + o + 3] << 8;
        if (p[12 + o] == 66 && p[12 + o + 1] == 67 && slen == 2 && o + 6 <= xlen) bsize = (int)((uint32_t)p[12 + o + 4] | (uint32_t)p[12 + o + 5] << 8);
        o += 4 + slen;
    }
    if (bsize < 0) return 1;
    *total = (uint32_t)bsize + 1; *hdr = 12u + xlen;
    return 0;
}

struct Member { uint64_t src_off, dst_off; uint32_t clen, isize, crc, pre_status; };     // src_off: of the deflate payload

}  // namespace brcinf
#endif
