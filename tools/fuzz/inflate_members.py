"""BGZF members for the inflater's tests and fuzzing (tests/test_inflate.py): builders over zlib, the fixed list of malformed members
with the status the format demands for each, and a seeded mutator.  The mutated members are for the CPU build of the inflater under
the host sanitizers (tests/sim_inflate: make asan) — never for a GPU.

    python tools/fuzz/inflate_members.py --seed 7 --count 20000     # a longer fuzz run than the suite's, same checks
"""
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
        self.v, self.n = 0, 0

    def field(self, value, nbits):
        self.v |= value << self.n; self.n += nbits; return self

    def code(self, value, nbits):
        for k in range(nbits - 1, -1, -1):
            self.field((value >> k) & 1, 1)
        return self

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


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
