"""A decoder of one BGZF member's deflate payload for the deflater's tests (tests/test_deflate.py): not what the bytes stand for — zlib
says that — but HOW they were written: every block's type and span of input positions, a dynamic block's header field by field, and the
tokens.  Written from RFC 1951 over the tables of tools/fuzz/inflate_members.py; it checks itself against zlib on every member."""
import collections
import heapq
import os
import sys
import zlib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "fuzz"))
import inflate_members as im  # noqa: E402

# btype 0 / 1 / 2 (stored / fixed / dynamic); final: BFINAL; [start, end): the input positions the block stands for; tokens: a literal
# is an int, a match (length, distance) — a stored block has none.  Dynamic blocks only (None otherwise): hlit, hdist, hclen as counts
# (257..286, 1..30, 4..19); cl_lens: the 19 lengths of the code-length code by symbol; cl_seq: the code-length symbols as written, an
# int 0..15 or (16 / 17 / 18, repeats); lit_lens, dist_lens: the hlit and hdist code lengths they stand for.
Block = collections.namedtuple("Block", "btype final start end tokens hlit hdist hclen cl_lens cl_seq lit_lens dist_lens")


def unlimited_depth(histogram):
    """The longest code of a Huffman code without a length limit for these counts (zeros take no part)."""
    h = [(c, 0) for c in histogram if c]
    if not h:
        return 0
    heapq.heapify(h)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        heapq.heappush(h, (a[0] + b[0], max(a[1], b[1]) + 1))
    return h[0][1]


class _Reader:
    def __init__(self, data):
        self.d, self.pos = data + b"\0" * 8, 0

    def peek(self, n):
        return (int.from_bytes(self.d[self.pos >> 3:(self.pos >> 3) + 4], "little") >> (self.pos & 7)) & ((1 << n) - 1)

    def bits(self, n):
        v = self.peek(n); self.pos += n
        return v


def _table(lens):
    """code lengths -> (longest, {the next `longest` bits of the stream, LSB first: (symbol, its length)})"""
    longest, t = max(lens), {}
    for s, c in enumerate(im.canonical(list(lens))):
        if c:
            rev = int(format(c[0], "0%db" % c[1])[::-1], 2)
            for hi in range(1 << (longest - c[1])):
                t[rev | hi << c[1]] = (s, c[1])
    return longest, t


def _symbol(r, table):
    s, n = table[1][r.peek(table[0])]           # (KeyError: bits that are no code of an incomplete set)
    r.pos += n
    return s


_FIXED = (_table(im.FIXED_LIT), _table(im.FIXED_DIST))


def decode(member):
    """The blocks of a member, in order.  Asserts that they stand for zlib.decompress(member, 31) and end where the payload ends."""
    payload = im.payload_of(member)
    r, out, blocks = _Reader(payload), bytearray(), []
    while True:
        final, btype, start = r.bits(1), r.bits(2), len(out)
        assert btype < 3
        hdr = (None,) * 7
        if btype == 0:
            r.pos = (r.pos + 7) & ~7
            n, nn = r.bits(16), r.bits(16)
            assert n ^ nn == 0xffff
            out += payload[r.pos >> 3:(r.pos >> 3) + n]; r.pos += 8 * n
            tokens = []
        else:
            if btype == 1:
                lit, dist = _FIXED
            else:
                hlit, hdist, hclen = r.bits(5) + 257, r.bits(5) + 1, r.bits(4) + 4
                cl_lens = [0] * 19
                for s in im.CL_ORDER[:hclen]:
                    cl_lens[s] = r.bits(3)
                cl, cl_seq, lens = _table(cl_lens), [], []
                while len(lens) < hlit + hdist:
                    s = _symbol(r, cl)
                    if s < 16:
                        cl_seq.append(s); lens.append(s)
                    else:
                        rep = (3, 3, 11)[s - 16] + r.bits((2, 3, 7)[s - 16])
                        cl_seq.append((s, rep)); lens += [lens[-1] if s == 16 else 0] * rep
                assert len(lens) == hlit + hdist
                hdr = (hlit, hdist, hclen, cl_lens, cl_seq, lens[:hlit], lens[hlit:])
                lit, dist = _table(lens[:hlit]), (_table(lens[hlit:]) if any(lens[hlit:]) else None)
            tokens = []
            while True:
                s = _symbol(r, lit)
                if s == 256:
                    break
                if s < 256:
                    tokens.append(s); out.append(s); continue
                assert s < 286
                length = im.LEN_BASE[s - 257] + r.bits(im.LEN_EXTRA[s - 257])
                j = _symbol(r, dist)
                assert j < 30
                d = im.DIST_BASE[j] + r.bits(im.DIST_EXTRA[j])
                assert d <= len(out)
                tokens.append((length, d))
                for _ in range(length):
                    out.append(out[-d])
        blocks.append(Block(btype, final, start, len(out), tokens, *hdr))
        if final:
            break
    assert (r.pos + 7) >> 3 == len(payload), ((r.pos + 7) >> 3, len(payload))
    assert bytes(out) == zlib.decompress(member, 31)
    return blocks
