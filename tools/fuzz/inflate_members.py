"""BGZF members for the inflater's tests and fuzzing (tests/test_inflate.py): builders over zlib, the fixed list of malformed members
with the status the format demands for each, and a seeded mutator.  The mutated members are for the CPU build of the inflater under
the host sanitizers (tests/sim_inflate: make asan) — never for a GPU.

Next to them a deflate encoder that owes nothing to zlib's compressor (stored_block / fixed_block / dynamic_block, tables of RFC 1951
3.2.5): the valid streams that compressor never writes — a fixed list (handmade_cases) and a seeded generator (random_valid).  The tests
hold every one of them against zlib's DECODER before the inflater sees it.

    python tools/fuzz/inflate_members.py --seed 7 --count 20000     # a longer fuzz run than the suite's, same checks
"""
import bisect
import collections
import struct
import zlib

import numpy as np

OK, BAD_HEADER, BAD_STREAM, SIZE_MISMATCH, CRC_MISMATCH, TRUNCATED = range(6)
E_ARG = -1

Case = collections.namedtuple("Case", "name chain rc status outputs slots")


def wrap(deflate, crc, isize, extra_before=b"", extra_after=b"", bc=True, bsize=None):
    """gzip member header (RFC 1952) with the BC subfield (SAMv1 4.1) around a raw-deflate payload."""
    extra = extra_before + (b"BC\x02\x00\x00\x00" if bc else b"bc\x02\x00\x00\x00") + extra_after
    total = 12 + len(extra) + len(deflate) + 8
    if total > 65536:
        return None
    k = len(extra_before) + 4
    extra = extra[:k] + struct.pack("<H", (total - 1) if bsize is None else bsize) + extra[k + 2:]
    return b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff" + struct.pack("<H", len(extra)) + extra + deflate + struct.pack("<II", crc & 0xffffffff, isize & 0xffffffff)


def deflate(payload, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=()):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    out, last = [], 0
    for cut in flush_at:
        out.append(c.compress(payload[last:cut])); out.append(c.flush(zlib.Z_FULL_FLUSH)); last = cut
    out.append(c.compress(payload[last:])); out.append(c.flush())
    return b"".join(out)


def member(payload, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=(), **kw):
    return wrap(deflate(payload, level, strategy, flush_at), zlib.crc32(payload), len(payload), **kw)


EOF_MEMBER = wrap(b"\x03\x00", 0, 0)


def payload_of(m):
    xlen, = struct.unpack_from("<H", m, 10)
    return m[12 + xlen:-8]


def split_members(raw, decode=True):
    members, payloads, o = [], [], 0
    while o < len(raw):
        xlen, = struct.unpack_from("<H", raw, o + 10)
        x, bsize = 0, None
        while x + 4 <= xlen:
            si, slen = raw[o + 12 + x:o + 14 + x], struct.unpack_from("<H", raw, o + 14 + x)[0]
            if si == b"BC" and slen == 2:
                bsize, = struct.unpack_from("<H", raw, o + 16 + x)
            x += 4 + slen
        m = raw[o:o + bsize + 1]
        members.append(m)
        if decode:
            payloads.append(zlib.decompress(payload_of(m), -15))
        o += bsize + 1
    return members, payloads


class Bits:
    """deflate's bit order: fields LSB first, Huffman codes MSB first (RFC 1951 3.1.1)"""

    def __init__(self):
        self.out, self.v, self.k = bytearray(), 0, 0          # whole bytes written, the bits waiting behind them

    @property
    def n(self):
        return len(self.out) * 8 + self.k

    def field(self, value, nbits):
        self.v |= value << self.k; self.k += nbits
        if self.k >= 64:
            nb = self.k >> 3
            self.out += (self.v & ((1 << 8 * nb) - 1)).to_bytes(nb, "little"); self.v >>= 8 * nb; self.k -= 8 * nb
        return self

    def code(self, value, nbits):
        return self.field(int(format(value, "0%db" % nbits)[::-1], 2), nbits) if nbits else self

    def align(self):
        return self.field(0, -self.k & 7)

    def raw(self, data):
        assert self.k % 8 == 0
        self.out += self.v.to_bytes(self.k // 8, "little") + data; self.v = self.k = 0
        return self

    def bytes(self):
        return bytes(self.out) + self.v.to_bytes((self.k + 7) // 8, "little")


# ---- a deflate encoder written from RFC 1951 alone: the caller chooses every code length, every token and every symbol of the header,
# so it writes the valid forms that zlib's compressor never does (and, for the malformed list, the invalid ones next to them)
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]     # 3.2.5
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]                                                  # 3.2.7
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8                                                                         # 3.2.6
FIXED_DIST = [5] * 32


def canonical(lens):
    """code lengths -> [(code, nbits) or None per symbol] (3.2.2)"""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1; nxt[b] = code
    out = [None] * len(lens)
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l); nxt[l] += 1
    return out


def len_symbol(length):
    return 28 if length == 258 else bisect.bisect_right(LEN_BASE, length) - 1


def dist_symbol(dist):
    return bisect.bisect_right(DIST_BASE, dist) - 1


def put_tokens(bits, lit, dist, tokens):
    """tokens: a literal is an int, a match (len, dist) — or (len, dist, length symbol) where the symbol is not the usual one (258 as 284 + 31)"""
    for t in tokens:
        if isinstance(t, int):
            bits.code(*lit[t]); continue
        k = t[2] - 257 if len(t) > 2 else len_symbol(t[0])
        j = dist_symbol(t[1])
        assert 0 <= t[0] - LEN_BASE[k] < 1 << LEN_EXTRA[k] and 0 <= t[1] - DIST_BASE[j] < 1 << DIST_EXTRA[j]
        bits.code(*lit[257 + k]).field(t[0] - LEN_BASE[k], LEN_EXTRA[k])
        bits.code(*dist[j]).field(t[1] - DIST_BASE[j], DIST_EXTRA[j])


def expand(tokens, out=None):
    """What tokens mean, byte by byte (3.2.3); out: the bytes in front of them, extended in place."""
    out = bytearray() if out is None else out
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            for _ in range(t[0]):
                out.append(out[-t[1]])
    return bytes(out)


def stored_block(bits, final, data):
    assert len(data) <= 0xffff
    bits.field(final, 1).field(0, 2).align().field(len(data), 16).field(len(data) ^ 0xffff, 16).raw(data)


def fixed_block(bits, final, tokens):
    bits.field(final, 1).field(1, 2)
    put_tokens(bits, _FIXED[0], _FIXED[1], tokens)
    bits.code(*_FIXED[0][256])


_FIXED = (canonical(FIXED_LIT), canonical(FIXED_DIST))


def balanced_lens(k):
    """a complete code over k >= 2 symbols, as flat as it can be"""
    d = k.bit_length() - 1
    return [d] * ((2 << d) - k) + [d + 1] * (2 * (k - (1 << d)))


def cl_expand(cl_seq):
    """the code lengths a sequence of code-length symbols stands for: ints 0..15, (16, repeats), (17, zeros), (18, zeros)"""
    lens = []
    for s in cl_seq:
        if isinstance(s, int):
            lens.append(s)
        else:
            assert 3 <= s[1] <= (6, 10, 138)[s[0] - 16] and (s[0] != 18 or s[1] >= 11)
            lens += [lens[-1] if s[0] == 16 else 0] * s[1]
    return lens


def dynamic_block(bits, final, lit_lens, dist_lens, tokens, cl_seq=None, cl_lens=None, hclen=None, eob=True):
    """lit_lens (HLIT + 257 of them) and dist_lens (HDIST + 1) as they stand in the header; cl_seq: the code-length symbols that carry
    them (default: one symbol per length, no runs); cl_lens: the 19 lengths of the code-length code (default: a complete, flat code over
    the symbols cl_seq uses); hclen: how many of them the header lists, 4..19 (default: as few as cl_lens allows).  Nothing is checked
    beyond what the bit fields can hold: the malformed list is written with it too."""
    cl_seq = list(lit_lens) + list(dist_lens) if cl_seq is None else cl_seq
    if cl_lens is None:
        used = sorted({s if isinstance(s, int) else s[0] for s in cl_seq})
        if len(used) == 1:
            used = sorted(used + [(used[0] + 1) % 19])
        cl_lens = [0] * 19
        for s, l in zip(used, balanced_lens(len(used))):
            cl_lens[s] = l
    if hclen is None:
        hclen = max(4, 1 + max(i for i, s in enumerate(CL_ORDER) if cl_lens[s]))
    bits.field(final, 1).field(2, 2).field(len(lit_lens) - 257, 5).field(len(dist_lens) - 1, 5).field(hclen - 4, 4)
    for s in CL_ORDER[:hclen]:
        bits.field(cl_lens[s], 3)
    cl = canonical(cl_lens)
    for s in cl_seq:
        if isinstance(s, int):
            bits.code(*cl[s])
        else:
            bits.code(*cl[s[0]]).field(s[1] - (3, 3, 11)[s[0] - 16], (2, 3, 7)[s[0] - 16])
    lit, dist = canonical(lit_lens), canonical(dist_lens)
    put_tokens(bits, lit, dist, tokens)
    if eob:
        bits.code(*lit[256])
    return lit, dist


def lens_of(n, given):
    out = [0] * n
    for s, l in given.items():
        out[s] = l
    return out


class _Stream:
    """a raw-deflate stream and the bytes it stands for, built side by side"""

    def __init__(self):
        self.bits, self.out = Bits(), bytearray()

    def stored(self, final, data):
        stored_block(self.bits, final, data); self.out += data; return self

    def fixed(self, final, tokens):
        fixed_block(self.bits, final, tokens); expand(tokens, self.out); return self

    def dynamic(self, final, lit_lens, dist_lens, tokens, cl_seq=None, **kw):
        assert cl_seq is None or cl_expand(cl_seq) == list(lit_lens) + list(dist_lens)
        dynamic_block(self.bits, final, lit_lens, dist_lens, tokens, cl_seq, **kw); expand(tokens, self.out); return self

    def case(self, name, behind=b""):
        return name, self.bits.bytes() + behind, bytes(self.out)


OVERLAP_DISTS = list(range(1, 17)) + [31, 32, 33, 63, 64, 65, 127, 128, 129]
OVERLAP_LENS = [3, 4, 63, 64, 65, 66, 127, 128, 129, 257, 258]
TRAILING = "bytes_behind_the_final_block"


def symbol_sweep():
    """matches over every length symbol and every distance symbol, each with its extra bits all 0 and all 1; they need 32 KB in front"""
    toks = []
    for k in range(29):
        toks.append((LEN_BASE[k], 1 + 1111 * k))
        toks.append((LEN_BASE[k] + (1 << LEN_EXTRA[k]) - 1, 32768 - 1111 * k, 257 + k))      # (k = 27: 258 written as 284 + 31)
    for j in range(30):
        toks.append((3 + j % 4, DIST_BASE[j]))
        toks.append((3 + j % 5, DIST_BASE[j] + (1 << DIST_EXTRA[j]) - 1))
    return toks


def handmade_cases():
    """(name, raw deflate, the bytes it stands for): valid streams in the forms zlib's compressor never writes (RFC 1951 3.2.7: no
    distance code, one distance code of one bit, runs of code lengths across the two tables, ...) and at the decoder's own boundaries.
    The tests check every one against zlib's DECODER first."""
    rng = np.random.default_rng(1951)
    cases = []
    ab = {97: 2, 98: 2, 256: 2, 257: 2}
    # one distance code of one bit: symbol 0 (distance 1), matches of 3 and 258 bytes; then the lone code on symbol 3 (distance 4)
    cases.append(_Stream().dynamic(1, lens_of(286, {97: 2, 256: 2, 257: 2, 285: 2}), [1], [97, (3, 1), (258, 1), 97, 97, (3, 1), (258, 1)]).case("lone_distance_code"))
    cases.append(_Stream().dynamic(1, lens_of(286, {97: 2, 98: 2, 256: 2, 257: 3, 285: 3}), lens_of(4, {3: 1}), [97, 98, 98, 97, (3, 4), (258, 4), 98, (258, 4)]).case("lone_distance_code_on_symbol_3"))
    # HDIST = 0 and the one length 0: literals only
    cases.append(_Stream().dynamic(1, lens_of(257, {120: 2, 121: 2, 122: 2, 256: 2}), [0], list(b"xyzzy" * 5)).case("no_distance_code"))
    # the literal/length code is the end-of-block code alone, one bit
    cases.append(_Stream().dynamic(1, lens_of(257, {256: 1}), [0], []).case("only_end_of_block"))
    # 15-bit codes on both tables (lengths 1, 2, ..., 14, 15, 15), every code used; the header lists all 19 code-length lengths (symbol 15
    # is the last of them) and the code-length code has 7-bit codes
    lits = [65, 67, 71, 84, 78, 10, 48, 49, 50, 51, 52, 53, 54, 55]
    lit_lens = lens_of(258, dict(zip(lits, [3, 1, 4, 2, 7, 5, 6, 10, 8, 9, 12, 11, 14, 13])))
    lit_lens[256] = lit_lens[257] = 15
    dsyms = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 16, 19]
    dist_lens = lens_of(20, dict(zip(dsyms, [15, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15])))
    toks = lits + [lits[int(i)] for i in rng.integers(0, 14, 1100)]
    for j in dsyms:
        toks += [(3, DIST_BASE[j]), lits[j % 14], (3, DIST_BASE[j] + (1 << DIST_EXTRA[j]) - 1)]
    cl_lens = lens_of(19, dict(zip(range(16), [2, 4, 4, 4, 4, 4, 4, 4, 5, 5, 3, 4, 5, 6, 7, 7])))
    cases.append(_Stream().dynamic(1, lit_lens, dist_lens, toks, cl_lens=cl_lens, hclen=19).case("fifteen_bit_codes_hclen_19"))
    # the fewest code-length lengths a block with any code can list: 5 (16, 17, 18, 0, 8 — with 4 every length is 0 and the block has
    # no end-of-block code: that one is in malformed_cases()); 256 codes of 8 bits
    cases.append(_Stream().dynamic(1, [8] * 255 + [0, 8], [0], list(range(0, 255, 7)), cl_lens=lens_of(19, {0: 1, 8: 1})).case("hclen_5"))
    # a run of zeros across the end of the literal/length lengths: symbol 17 (2 + 2 lengths), symbol 18 (12 + 5)
    lit_lens = lens_of(260, ab); dist_lens = lens_of(4, {2: 1, 3: 1})
    cases.append(_Stream().dynamic(1, lit_lens, dist_lens, [97, 98, 98, 97, (3, 3), (3, 4)], cl_seq=lit_lens[:258] + [(17, 4), 1, 1]).case("zero_run_17_crosses_tables"))
    lit_lens = lens_of(270, ab); dist_lens = lens_of(7, {5: 1, 6: 1})
    cases.append(_Stream().dynamic(1, lit_lens, dist_lens, [97, 98] * 6 + [98, (3, 7), (3, 12), 97, (3, 8), (3, 9)], cl_seq=lit_lens[:258] + [(18, 17), 1, 1]).case("zero_run_18_crosses_tables"))
    # symbol 16 repeats the last literal/length length as the first distance lengths; and a run that begins inside the first table
    lit_lens = lens_of(258, {97: 2, 98: 2, 256: 2, 99: 3, 257: 3}); dist_lens = [3] * 8
    toks = [97, 98, 99] * 6 + [(3, 1), (3, 2), 97, (3, 3), (3, 4), 98, (3, 6), (3, 8), 99, (3, 12), (3, 16)]
    cases.append(_Stream().dynamic(1, lit_lens, dist_lens, toks, cl_seq=lit_lens + [(16, 6), 3, 3]).case("copy_run_16_crosses_tables"))
    lit_lens = lens_of(258, {97: 2, 98: 2, 99: 2, 256: 3, 257: 3})
    cases.append(_Stream().dynamic(1, lit_lens, dist_lens, toks, cl_seq=lit_lens[:257] + [(16, 6), 3, 3, 3]).case("copy_run_16_begins_in_the_first_table"))
    # every length symbol and every distance symbol at both ends of its extra bits, behind 32 KB: fixed codes, then a dynamic block
    prefix = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    cases.append(_Stream().fixed(1, list(prefix) + symbol_sweep()).case("every_symbol_fixed"))
    toks = symbol_sweep()
    toks = [t for pair in zip(toks, [0, 1] * (len(toks) // 2)) for t in pair]
    cases.append(_Stream().stored(0, prefix).dynamic(1, lens_of(286, dict([(0, 5), (1, 5)] + [(s, 5) for s in range(256, 286)])), [4, 4] + [5] * 28, toks).case("every_symbol_dynamic"))
    s = _Stream().stored(0, prefix).fixed(1, [7, 9] + [(258, 32768)] * 127)
    assert len(s.out) == 65536
    cases.append(s.case("length_258_at_32768_ends_at_65536"))
    # a match over its own output (dist < len) and next to it, around the 64 lanes of the copy; distinct bytes in front show a wrong residue
    toks = []
    for d in OVERLAP_DISTS:
        for n in OVERLAP_LENS:
            toks += [(d * 11 + n + 37 * j) & 255 for j in range(d)] + [(n, d)]
    cases.append(_Stream().fixed(1, toks).case("overlap_sweep"))
    # blocks that end at, before and behind the decoder's batches of 64 tokens: literals alone, then a match as the last token
    counts = (63, 64, 65, 127, 128, 129)
    s = _Stream()
    for i, n in enumerate(counts):
        s.fixed(i == len(counts) - 1, [(i * 50 + j) & 255 for j in range(n)])
    cases.append(s.case("batch_boundary_literals"))
    s = _Stream()
    for i, n in enumerate(counts):
        s.fixed(i == len(counts) - 1, [(i * 50 + 3 * j) & 255 for j in range(n)] + [(7 + i, 5 + 9 * i)])
    cases.append(s.case("batch_boundary_literals_then_a_match"))
    s = _Stream().fixed(0, [1, 2, 3])
    for i, n in enumerate((64, 63, 65)):
        s.fixed(i == 2, [(3 + (j * 5) % 40, 1 + (j * 7) % 3) for j in range(n)])
    cases.append(s.case("blocks_of_matches"))
    cases.append(_Stream().fixed(1, [1, 2, 3, 4, 5, (5, 5), (10, 3), (3, 13), (20, 20), 6, (70, 1), (64, 64), (130, 65)]).case("match_from_its_own_batch"))
    # many blocks: 3000 fixed blocks of one literal and an empty final one
    s = _Stream()
    for i in range(3000):
        s.fixed(0, [i & 255])
    cases.append(s.fixed(1, []).case("three_thousand_blocks"))
    # fixed, stored, dynamic, stored (empty), fixed: the stored blocks begin at every bit offset 0..7
    at = set()
    for k in range(8):
        s = _Stream().fixed(0, [65, 66] + [200 + j for j in range(k)])           # (literals from 144 on take 9 bits)
        at.add(s.bits.n % 8)
        s.stored(0, b"stored %d" % k).dynamic(0, lens_of(258, {97: 1, 98: 2, 256: 3, 257: 3}), [1], [98] + [97] * k + [(3, 1)])
        at.add(8 + s.bits.n % 8)
        cases.append(s.stored(0, b"").fixed(1, [67, (4, 2)]).case("mixed_blocks_%d" % k))
    assert at == set(range(16))
    # three bytes of the payload behind the final block: neither ISIZE nor CRC32 covers them; the member is good (htslib takes it too)
    cases.append(_Stream().fixed(1, [72, 105, (6, 2)]).case(TRAILING, b"\xde\xad\xbf"))
    return cases


def handmade_malformed():
    """(name, raw deflate, CRC32 and ISIZE of the trailer, status): dynamic blocks that break one rule of RFC 1951 each, written with
    the encoder above; the rule stands next to each.  They join malformed_cases()."""
    ab = {97: 2, 98: 2, 256: 2, 257: 2}
    out = []

    def add(name, bits, status=BAD_STREAM):
        out.append((name, bits.bytes() + b"\0" * 16, 0, 10, status))

    # 3.2.7: HLIT + 257 literal/length lengths, 257..286 — the field can say 287 and 288 (3.2.6: symbols 286 and 287 never occur in a stream)
    b = Bits(); dynamic_block(b, 1, lens_of(287, ab), [1], [97, 98]); add("hlit_30", b)
    # ... HDIST + 1 distance lengths: symbols 30 and 31 never occur either, and zlib refuses a count above 30
    b = Bits(); dynamic_block(b, 1, lens_of(257, {97: 1, 256: 1}), [1] + [0] * 30, [97]); add("hdist_30", b)
    # 3.2.7: 16 copies the PREVIOUS code length — the first symbol of the sequence has none
    lit_lens = lens_of(257, {97: 2, 98: 2, 99: 2, 256: 2})
    b = Bits(); dynamic_block(b, 1, lit_lens, [0], [97], cl_seq=[(16, 3)] + lit_lens[3:] + [0]); add("repeat_without_a_previous_length", b)
    # 3.2.7: the sequence holds HLIT + 257 + HDIST + 1 lengths; here a run of 3 zeros begins at the last of them
    b = Bits(); dynamic_block(b, 1, lit_lens, [0], [97], cl_seq=lit_lens + [(17, 3)]); add("run_past_the_last_length", b)
    # 3.2.3 / 3.2.7: every block ends with symbol 256, so a code without it (complete otherwise: two codes of one bit) cannot be a block's
    b = Bits(); dynamic_block(b, 1, lens_of(257, {97: 1, 98: 1}), [0], [97, 98], eob=False); add("no_end_of_block_code", b)
    # 3.2.2: the lengths must describe a prefix code that uses its whole code space: {1 bit, 2 bits} leaves a quarter of it unused
    b = Bits(); dynamic_block(b, 1, lens_of(257, {97: 1, 256: 2}), [0], [97]); add("literal_set_incomplete", b)
    # 3.2.7: "if only one distance code is used, it is encoded using one bit, not zero bits" — and not two
    b = Bits(); dynamic_block(b, 1, lens_of(258, ab), [2], [97, (3, 1)]); add("lone_distance_code_of_two_bits", b)
    # ... the exemption is for ONE code: two codes of 1 and 2 bits are an incomplete set like any other
    b = Bits(); dynamic_block(b, 1, lens_of(258, ab), [1, 2], [97, (3, 1)]); add("distance_set_of_two_incomplete", b)
    # ... the lone code is the bit 0; "one unused code" is the bit 1, and it stands for no distance
    b = Bits(); lit, _ = dynamic_block(b, 1, lens_of(258, ab), [1], [97], eob=False)
    b.code(*lit[257]).field(1, 1).code(*lit[256]); add("unused_half_of_the_lone_distance_code", b)
    # 3.2.7: "one distance code of zero bits means that there are no distance codes used at all (the data is all literals)"
    b = Bits(); lit, _ = dynamic_block(b, 1, lens_of(258, ab), [0], [97], eob=False)
    b.code(*lit[257]).field(0, 5).code(*lit[256]); add("match_without_a_distance_code", b)
    # 3.2.7: HCLEN + 4 = 4 lists the lengths of 16, 17, 18 and 0 alone: every code length is then 0 and there is no end-of-block code
    b = Bits(); dynamic_block(b, 1, [0] * 257, [0], [], cl_seq=[(18, 138), (18, 120)], cl_lens=lens_of(19, {18: 1, 0: 1}), hclen=4, eob=False); add("hclen_4", b)
    # 3.2.3: BFINAL is set "if and only if this is the last block": a stream whose blocks are all whole, none of them final, is cut short
    data = b"no final block"
    b = Bits(); stored_block(b, 0, data)
    out.append(("no_final_block", b.bytes(), zlib.crc32(data), len(data), TRUNCATED))
    return out


HANDMADE_MALFORMED = [c[0] for c in handmade_malformed()]


def malformed_cases():
    """Every case: good member A, the malformed member, good member B in one chain (the two cases that break the chain itself have
    nothing behind the break).  The expected status follows from the format:"""
    pa, pb = b"the first good member " * 40, bytes(range(256)) * 9
    A, B = member(pa, 6), member(pb, 1)
    p = (b"ACGTTGCA" * 500 + bytes(range(200))) * 3
    d = deflate(p, 6)
    cases = []

    def mid(name, bad, status, slot=None):
        cases.append(Case(name, A + bad + B, 0, [OK, status, OK], [pa, None, pb], [len(pa), len(p) if slot is None else slot, len(pb)]))

    # the trailer's CRC32 is not the CRC32 of the output (RFC 1952 2.3.1)
    mid("crc_flipped", wrap(d, zlib.crc32(p) ^ 0x00010000, len(p)), CRC_MISMATCH)
    # ISIZE says one byte more / one byte less than the stream yields
    mid("isize_plus_one", wrap(d, zlib.crc32(p), len(p) + 1), SIZE_MISMATCH, len(p) + 1)
    mid("isize_minus_one", wrap(d, zlib.crc32(p), len(p) - 1), SIZE_MISMATCH, len(p) - 1)
    # the stream runs far past ISIZE (the CRC32 is even that of the first ISIZE bytes)
    mid("runs_past_isize", wrap(d, zlib.crc32(p[:1000]), 1000), SIZE_MISMATCH, 1000)
    # the payload ends inside the stream: the end-of-block code and the final bytes are gone (BSIZE fits what is left)
    mid("payload_cut_short", wrap(d[:-7], zlib.crc32(p), len(p)), TRUNCATED)
    s0 = deflate(b"stored bytes" * 20, 0)
    assert s0[0] == 1 and struct.unpack_from("<H", s0, 1)[0] == 240
    # a stored block whose NLEN is not the complement of LEN (RFC 1951 3.2.4)
    mid("len_nlen_mismatch", wrap(s0[:3] + bytes([s0[3] ^ 0x10]) + s0[4:], zlib.crc32(b"stored bytes" * 20), 240), BAD_STREAM, 240)
    # a stored block that promises more bytes than the payload holds
    mid("stored_cut_short", wrap(s0[:100], zlib.crc32(b"stored bytes" * 20), 240), TRUNCATED, 240)
    # BTYPE 11 is reserved (3.2.3)
    mid("block_type_3", wrap(Bits().field(1, 1).field(3, 2).field(0, 5).bytes() + b"\0" * 8, 0, 10), BAD_STREAM, 10)
    # dynamic block, code-length code with 19 codes of one bit: over-subscribed (3.2.2: the lengths must form a prefix code)
    over = Bits().field(1, 1).field(2, 2).field(0, 5).field(0, 5).field(15, 4)
    for _ in range(19):
        over.field(1, 3)
    mid("code_lengths_over_subscribed", wrap(over.bytes() + b"\0" * 16, 0, 10), BAD_STREAM, 10)
    # ... with a single code of two bits: incomplete (three quarters of the code space lead nowhere)
    inc = Bits().field(1, 1).field(2, 2).field(0, 5).field(0, 5).field(0, 4).field(0, 3).field(0, 3).field(0, 3).field(2, 3)
    mid("code_lengths_incomplete", wrap(inc.bytes() + b"\0" * 16, 0, 10), BAD_STREAM, 10)
    # literal/length lengths over-subscribed: a valid code-length code {0: 1 bit, 1: 1 bit} assigning one bit to all 258 symbols
    lit = Bits().field(1, 1).field(2, 2).field(0, 5).field(0, 5).field(14, 4)
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    for s in order[:18]:
        lit.field(1 if s in (0, 1) else 0, 3)
    for _ in range(258):
        lit.code(1, 1)                 # symbol 1 = "length 1"
    mid("literal_lengths_over_subscribed", wrap(lit.bytes() + b"\0" * 16, 0, 10), BAD_STREAM, 10)
    # fixed codes, first symbol a match (length 3, distance 1) with no output in front of it (3.2.5: a distance cannot reach before the start)
    far = Bits().field(1, 1).field(1, 2).code(1, 7).code(0, 5).code(0, 7)
    mid("distance_before_start", wrap(far.bytes(), 0, 3), BAD_STREAM, 3)
    # ... a literal, then distance 2 with one byte of output
    far2 = Bits().field(1, 1).field(1, 2).code(0x30 + 65, 8).code(1, 7).code(1, 5).code(0, 7)
    mid("distance_before_start_after_a_literal", wrap(far2.bytes(), 0, 4), BAD_STREAM, 4)
    # fixed codes: length symbol 286 (8-bit code 11000110) and distance symbol 30 are reserved (3.2.6)
    mid("reserved_length_symbol_286", wrap(Bits().field(1, 1).field(1, 2).code(0x30 + 65, 8).code(0xc6, 8).code(0, 5).code(0, 7).bytes(), 0, 4), BAD_STREAM, 4)
    mid("reserved_distance_symbol_30", wrap(Bits().field(1, 1).field(1, 2).code(0x30 + 65, 8).code(1, 7).code(30, 5).code(0, 7).bytes(), 0, 4), BAD_STREAM, 4)
    # ISIZE beyond what a BGZF member may hold: refused before any decoding, takes no room in dst
    mid("isize_above_65536", wrap(d, zlib.crc32(p), 0x80000000 | len(p)), BAD_HEADER, 0)
    # dynamic-block headers and code sets that break one rule each (handmade_malformed)
    for name, raw, crc, isize, status in handmade_malformed():
        mid(name, wrap(raw, crc, isize), status, isize)
    # the chain breaks: BSIZE points beyond src / no BC subfield — BRC_E_ARG, the whole members in front are inflated
    good = member(p, 6)
    cases.append(Case("bsize_beyond_src", A + B + wrap(d, zlib.crc32(p), len(p), bsize=len(good) + 40), E_ARG, [OK, OK], [pa, pb], [len(pa), len(pb)]))
    cases.append(Case("no_bc_subfield", A + wrap(d, zlib.crc32(p), len(p), bc=False) + B, E_ARG, [OK], [pa], [len(pa)]))
    return cases


def mutations(seed, count):
    """count chains of three small members, the middle one mutated somewhere behind its header (BSIZE stays right, so the chain holds)."""
    rng = np.random.default_rng(seed)
    base = []
    for k in range(12):
        n = int(rng.integers(1, 3000))
        kind = k % 4
        if kind == 0:
            p = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        elif kind == 1:
            p = rng.choice(np.frombuffer(b"ACGTN", np.uint8), n).tobytes()
        elif kind == 2:
            p = (b"%d:" % k) * n
        else:
            p = bytes(rng.integers(0, 4, n, dtype=np.uint8) * 60)
        level, strategy = [(0, 0), (1, 0), (6, 0), (9, 0), (6, zlib.Z_FIXED), (6, zlib.Z_HUFFMAN_ONLY), (6, zlib.Z_RLE)][k % 7]
        base.append(member(p, level, strategy, flush_at=(n // 2,) if k % 5 == 0 else ()))
    chains, meta = [], []
    for i in range(count):
        a, m, b = (base[int(x)] for x in rng.integers(0, len(base), 3))
        m = bytearray(m)
        lo = 18
        how = int(rng.integers(0, 5))
        for _ in range(int(rng.integers(1, 4))):
            j = int(rng.integers(lo, len(m)))
            if how == 0:
                m[j] ^= 1 << int(rng.integers(0, 8))
            elif how == 1:
                m[j] = int(rng.integers(0, 256))
            elif how == 2:                                    # a stretch of the payload replaced by noise
                e = min(len(m) - 8, j + int(rng.integers(1, 40)))
                m[j:e] = rng.integers(0, 256, max(e - j, 0), dtype=np.uint8).tobytes()
            elif how == 3:                                    # the first bytes of the stream (block headers, code lengths)
                j = int(rng.integers(lo, min(lo + 24, len(m))))
                m[j] ^= 1 << int(rng.integers(0, 8))
            else:                                             # the trailer
                j = int(rng.integers(len(m) - 8, len(m) - 2))  # (not the high bytes of ISIZE: the slot stays small)
                m[j] ^= 1 << int(rng.integers(0, 8))
        isize, = struct.unpack("<I", bytes(m[-4:]))
        if isize > 65536:
            m[-4:] = struct.pack("<I", isize & 0xffff)
        chains.append(a + bytes(m) + b); meta.append(how)
    return chains, meta


def random_lens(rng, k, maxlen, deep=0.0):
    """k >= 2 code lengths of a complete code: leaves split at random (with odds `deep` the deepest one) down to maxlen"""
    leaves = [1, 1]
    while len(leaves) < k:
        cand = [i for i, l in enumerate(leaves) if l < maxlen]
        i = max(cand, key=leaves.__getitem__) if rng.random() < deep else cand[int(rng.integers(len(cand)))]
        l = leaves.pop(i); leaves += [l + 1, l + 1]
    return [int(x) for x in rng.permutation(leaves)]


def random_cl_seq(rng, lens, nlen, p_run):
    """lens as code-length symbols, a run taken with odds p_run wherever one is possible -> (sequence, a run crosses nlen)"""
    seq, i, crossing = [], 0, False
    run = [1] * len(lens)                                     # equal lengths from i on
    for k in range(len(lens) - 2, -1, -1):
        if lens[k] == lens[k + 1]:
            run[k] = run[k + 1] + 1
    while i < len(lens):
        v, r = lens[i], run[i]
        opts = [s for s, ok in ((16, i > 0 and lens[i - 1] == v and r >= 3), (17, v == 0 and r >= 3), (18, v == 0 and r >= 11)) if ok]
        if opts and rng.random() < p_run:
            sym = opts[int(rng.integers(len(opts)))]
            lo, hi = {16: (3, 6), 17: (3, 10), 18: (11, 138)}[sym]
            rep = min(hi, r) if rng.random() < 0.5 else int(rng.integers(lo, min(hi, r) + 1))
            crossing |= i < nlen < i + rep
            seq.append((sym, rep)); i += rep
        else:
            seq.append(v); i += 1
    return seq, crossing


def random_tokens(rng, lits, lsyms, dsyms, pos, room):
    toks, end = [], pos + room
    while pos < end:
        if lsyms and dsyms and rng.random() < 0.4:
            k = lsyms[int(rng.integers(len(lsyms)))]; n = LEN_BASE[k] + int(rng.integers(1 << LEN_EXTRA[k]))
            near = [j for j in dsyms if DIST_BASE[j] <= pos]
            if near and n <= end - pos:
                j = near[int(rng.integers(len(near)))]
                toks.append((n, min(pos, DIST_BASE[j] + int(rng.integers(1 << DIST_EXTRA[j]))), 257 + k)); pos += n
                continue
        toks.append(lits[int(rng.integers(len(lits)))]); pos += 1
    return toks


def random_valid(seed, count):
    """count valid raw-deflate streams -> [(raw, the bytes it stands for, tags)]: 1..4 blocks (stored, fixed, mostly dynamic), at most
    4 KB of output; random complete code-length sets down to 15 bits — and the two incomplete distance sets the format allows —,
    random tokens over them, random runs in the header, random HCLEN.  tags: "lone" / "none" (a block with one distance code of one bit
    / without any), "crossing" (a run of the header crosses from the literal/length lengths into the distance lengths)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        s, tags = _Stream(), set()
        nblocks, budget = int(rng.integers(1, 5)), int(4097 ** rng.random()) - 1
        for b in range(nblocks):
            final, room, kind = int(b == nblocks - 1), budget * (b + 1) // nblocks - len(s.out), rng.random()
            if kind < 0.1:
                s.stored(final, rng.integers(0, 256, room, dtype=np.uint8).tobytes()); continue
            if kind < 0.25:
                s.fixed(final, random_tokens(rng, range(256), range(29), range(30), len(s.out), room)); continue
            lits = [int(x) for x in rng.choice(256, int(rng.integers(1, 1 + (3, 20, 120)[int(rng.integers(3))])), replace=False)]
            lsyms = sorted(int(x) for x in rng.choice(29, int(rng.integers(0, 30)), replace=False))
            how = rng.random()
            if how < 0.2:                                      # no distance code: HDIST + 1 lengths, all 0
                tags.add("none"); dsyms, dist_lens = [], [0] * int(rng.integers(1, 31))
            elif how < 0.4:                                    # one distance code of one bit
                tags.add("lone"); dsyms = [int(30 ** rng.random()) - 1 if rng.random() < 0.7 else int(rng.integers(30))]
                dist_lens = lens_of(int(rng.integers(dsyms[0] + 1, 31)), {dsyms[0]: 1})
            else:
                dsyms = sorted(int(x) for x in rng.choice(30, int(rng.integers(2, 31)), replace=False))
                dist_lens = lens_of(int(rng.integers(dsyms[-1] + 1, 31)), dict(zip(dsyms, random_lens(rng, len(dsyms), 15, (0, 0.5, 0.95)[int(rng.integers(3))]))))
            syms = lits + [256] + [257 + k for k in lsyms]
            lit_lens = lens_of(int(rng.integers(max(syms) + 1, 287)), dict(zip(syms, random_lens(rng, len(syms), 15, (0, 0.5, 0.95)[int(rng.integers(3))]))))
            cl_seq, crossing = random_cl_seq(rng, lit_lens + dist_lens, len(lit_lens), (0.0, 0.5, 1.0)[int(rng.integers(3))])
            if crossing:
                tags.add("crossing")
            used = sorted({c if isinstance(c, int) else c[0] for c in cl_seq})
            if len(used) == 1:
                used = sorted(used + [(used[0] + 1) % 19])
            cl_lens = lens_of(19, dict(zip(used, random_lens(rng, len(used), 7, (0, 0.9)[int(rng.integers(2))]))))
            least = 1 + max(i for i, c in enumerate(CL_ORDER) if cl_lens[c])
            s.dynamic(final, lit_lens, dist_lens, random_tokens(rng, lits, lsyms, dsyms, len(s.out), room), cl_seq=cl_seq, cl_lens=cl_lens,
                      hclen=int(rng.integers(max(4, least), 20)))
        out.append((s.bits.bytes(), bytes(s.out), tags))
    return out


if __name__ == "__main__":
    import argparse
    import os
    import subprocess
    import tempfile
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--count", type=int, default=20000)
    a = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sim = os.path.join(root, "tests", "sim_inflate")
    subprocess.check_call(["make", "-s", "-C", sim, "asan"])
    chains, _ = mutations(a.seed, a.count)
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "cases.bin"), "wb") as f:
            for c in chains:
                f.write(struct.pack("<I", len(c))); f.write(c)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
        subprocess.check_call([os.path.join(sim, "inflate_check_asan"), os.path.join(d, "cases.bin"), os.path.join(d, "res.bin")], env=env)
    print("no sanitizer report in %d mutated chains" % len(chains))
