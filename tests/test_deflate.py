"""The BGZF deflater (include/brc_deflate.h): the compressor of bam_readcount_amd/csrc/brc_deflate_core.h behind its C-ABI, on the GPU
([hip]: libbrc_deflate_hip.so) and lane for lane on the CPU ([sim]: tests/sim_deflate).  The references are zlib (zlib.decompress with
wbits 31, member by member) and the repository's own inflater; equality is byte for byte.  The compression floor is zlib's
Z_HUFFMAN_ONLY on the same 0xff00 pieces: no encoder without a working match stage gets under it.

The seeded fuzz runs on the CPU build under the host sanitizers only; the GPU sees the fixed list.  What the fixed list makes the
compressor do is read back with tests/deflate_stream.py and asserted on the CPU build (test_new_inputs_reach_their_paths,
test_every_encoder_path_is_reached); the device shares it through byte equality."""
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

from conftest import ROOT
from test_cli import SIM_CLI, _write_fasta

sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tools", "fuzz"))
import inflate_members as im  # noqa: E402
import deflate_stream as ds  # noqa: E402

SIM_DIR = os.path.join(ROOT, "tests", "sim_deflate")
SIM_LIB = os.path.join(SIM_DIR, "libbrc_deflate_sim.so")
SIM_INFLATE_DIR = os.path.join(ROOT, "tests", "sim_inflate")
M = 0xff00
BLOCK = 16384                                  # input positions of one deflate block (brcdef::BLOCK)
SMALL_ZEROS = [2, 3, 4, 5, 15, 16, 17, 255, 256, 257]
TEXT_SIZES = [2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 255, 256, 257, 32767, 32768, 32769, 49151, 49152, 49153]
EOF_BLOCK = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
HEADER = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0])


def _sim():
    from bam_readcount_amd import capi
    subprocess.check_call(["make", "-s", "-C", SIM_DIR])
    d = capi.Deflater(SIM_LIB)
    assert d.kind() == "sim"
    return d


@pytest.fixture(scope="module", params=["sim", pytest.param("hip", marks=pytest.mark.gpu)])
def deflater(request):
    """[hip]: the product's deflater library (fails loudly when it was not built or has no device); [sim]: the CPU build."""
    from bam_readcount_amd import capi
    if request.param == "hip":
        d = capi.Deflater()
        assert d.kind() == "hip-gfx950"
        return d
    return _sim()


@pytest.fixture(scope="module")
def inflater(deflater):
    """The repository's own inflater of the same kind as the deflater under test."""
    from bam_readcount_amd import capi
    if deflater.kind() == "hip-gfx950":
        return capi.Inflater()
    subprocess.check_call(["make", "-s", "-C", SIM_INFLATE_DIR])
    return capi.Inflater(os.path.join(SIM_INFLATE_DIR, "libbrc_inflate_sim.so"))


@pytest.fixture(scope="module")
def text(tmp_path_factory):
    """What the simulator's command line prints for a seeded synthetic BAM (insertion centric): at least 4 MB of lines."""
    import bamio
    import synth
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "sim")])
    d = tmp_path_factory.mktemp("deflate_text")
    rng = np.random.default_rng(17)
    ref = synth.make_ref(rng, 40000)
    arrs = synth.make_batch(73, ref, 5000, style="indel")
    bamio.write_bam(str(d / "t.bam"), [("chrA", 40000)], arrs, np.zeros(len(arrs["pos"]), int), block_bytes=20000)
    _write_fasta(d / "t.fa", [("chrA", ref)])
    p = subprocess.run([SIM_CLI, "-w", "0", "-i", "-f", "t.fa", "t.bam", "chrA"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-500:]
    assert len(p.stdout) >= 4 << 20, len(p.stdout)
    return p.stdout


def _fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def _de_bruijn2(k):
    """The de Bruijn sequence B(k, 2) by Lyndon words: every ordered pair of k values once."""
    a, seq = [0] * (2 * k), []

    def db(t, p):
        if t > 2:
            if 2 % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]; db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j; db(t + 1, t)
    db(1, 1)
    return seq


def fixed_inputs(text):
    rng = np.random.default_rng(29)
    # a one-block member of literals whose counts follow the Fibonacci numbers 1, 1, 2 ... 2584 (18 of them and a filler), every other
    # byte: the bytes between them run through a de Bruijn sequence of 91 other values, so no two 4-byte windows are equal, nothing
    # is matched and the block's histogram is the bytes' own
    fib_lit = np.zeros(16384, np.uint8)
    exact = np.concatenate([np.full(f, i, np.uint8) for i, f in enumerate(_fib(18))] + [np.full(8192 - sum(_fib(18)), 18, np.uint8)])
    fib_lit[0::2] = rng.permutation(exact)
    fib_lit[1::2] = 75 + np.array(_de_bruijn2(91)[:8192], np.uint8)
    fib_lit = fib_lit.tobytes()
    # the same for distances: 4-byte copies from distances of 20 distance codes with Fibonacci counts, a fresh byte between them
    out = bytearray(rng.integers(0, 256, 1100, dtype=np.uint8).tobytes())
    codes = np.arange(3, 20); wd = np.array(_fib(len(codes)), float)
    for k in rng.choice(codes, 12000, p=wd / wd.sum()):
        lo = 4 if k == 3 else ((2 + (k & 1)) << ((k >> 1) - 1)) + 1
        hi = ((2 + ((k + 1) & 1)) << (((k + 1) >> 1) - 1)) + 1
        dist = int(rng.integers(lo, hi))
        for _ in range(4):
            out.append(out[-dist])
        out.append(int(rng.integers(0, 256)))
        if len(out) > 64000:
            break
    inputs = {
        "empty": b"", "one": b"Q",
        "text_m-1": text[:M - 1], "text_m": text[1000:1000 + M], "text_m+1": text[5000:5000 + M + 1], "text_3m": text[70000:70000 + 3 * M],
        "zeros": bytes(65280), "period2": b"xy" * 30001, "period3": b"abc" * 21000,
        "period259": rng.integers(0, 256, 259, dtype=np.uint8).tobytes() * 250,
        "random": rng.integers(0, 256, 65280, dtype=np.uint8).tobytes(), "all256": bytes(range(256)),
        "high": rng.integers(144, 256, 50000, dtype=np.uint8).tobytes(), "fib_literals": fib_lit, "fib_distances": bytes(out),
        # a block of text, a block no code shortens, a block of text: the middle one stays a stored block inside the stream
        "mixed_text_random_text": text[:16384] + rng.integers(0, 256, 16384, dtype=np.uint8).tobytes() + text[16384:32768],
    }
    # ---- inputs built for one path of the encoder each (test_new_inputs_reach_their_paths has the condition of every one).  Structure
    # stands on a background of zero bytes: a run of zeros ends exactly where the next other byte stands, so the parse arrives at the
    # intended position, and zeros fill one bucket of the head table, so the background displaces no intended candidate.  (Among the
    # 600 windows of P some share a bucket; with this seed none of the later ones shares that of a window a condition stands on.)
    rng2 = np.random.default_rng(32)
    A = rng2.integers(1, 256, 300, dtype=np.uint8).tobytes()
    G = bytes([0xc3, 0x5a, 0x17, 0xe9])
    P = rng2.integers(1, 200, 600, dtype=np.uint8).tobytes()
    noise = rng2.integers(0, 256, 16384 + 100, dtype=np.uint8).tobytes()
    for gap in (32767, 32768, 32769):                   # A again at this distance: the longest one, one short of it, one beyond
        inputs["a_again_at_%d" % gap] = A + bytes(gap - 300) + A
    for d in (4096, 4097):                              # G's first three bytes end block 0: a match of 3, allowed up to 4096 only
        z = bytearray(BLOCK + 50); z[BLOCK - 3 - d:BLOCK + 1 - d] = G; z[BLOCK - 3:BLOCK + 1] = G
        inputs["len3_at_%d" % d] = bytes(z)
    for back in (258, 259, 100, 2, 1):                  # P again, beginning this far before block 0 ends
        z = bytearray(BLOCK + 700); z[100:700] = P; z[BLOCK - back:BLOCK - back + 600] = P
        inputs["p_again_%d_before_the_block_ends" % back] = bytes(z)
    inputs["random_text_random"] = noise[:16384] + text[:16384] + noise[16384:]
    for n in SMALL_ZEROS + [BLOCK + 1, BLOCK + 3, BLOCK + 4]:
        inputs["zeros_%d" % n] = bytes(n)
    for n in TEXT_SIZES:
        inputs["short_text_%d" % n] = text[3000:3000 + n]
    inputs["abc_four_times"] = b"abcabcabcabc"
    # literals 0..15 and 27..42 alone: the 11 code lengths between them are the shortest run of zeros that symbol 18 can carry
    inputs["literals_with_a_gap_of_11"] = (rng2.integers(0, 32, 4000, dtype=np.uint8) // 16 * 27 + rng2.integers(0, 16, 4000, dtype=np.uint8)).astype(np.uint8).tobytes()
    return inputs


def check_chain(out, src):
    """Whole members with exact header bytes, BSIZE and ISIZE, each at most 0xff00 bytes of input; returns the members."""
    members, _ = im.split_members(out, decode=False) if out else ([], [])
    assert len(members) == (len(src) + M - 1) // M
    assert sum(len(m) for m in members) == len(out)
    o = 0
    for m in members:
        want = min(M, len(src) - o)
        assert m[:16] == HEADER and struct.unpack_from("<H", m, 16)[0] == len(m) - 1 and len(m) <= 65536
        assert struct.unpack("<II", m[-8:]) == (zlib.crc32(src[o:o + want]), want)
        assert zlib.decompress(m, 31) == src[o:o + want]
        o += want
    return members


def dynamic_header_max_lengths(m):
    """(max literal/length code length, max distance code length) of the FIRST block of a member, None when it is not dynamic."""
    b = ds.decode(m)[0]
    return (max(b.lit_lens), max(b.dist_lens)) if b.btype == 2 else None


def test_round_trip_of_the_fixed_list(deflater, inflater, text):
    for name, src in fixed_inputs(text).items():
        out = deflater.deflate(src)
        members = check_chain(out, src)
        if out:
            got, off, st = inflater.inflate(out)
            assert st.tolist() == [0] * len(members), name
            assert got == src, name
        if name == "empty":
            assert out == b""
        if name == "random":
            assert len(out) <= len(src) + 31 and members[0][18] == 1          # one stored block
        if name in ("zeros", "period2", "period3"):
            assert len(out) < 400, (name, len(out))                            # self-overlapping matches of length 258
        if name == "period259":
            assert len(out) < 3000, len(out)
        if name.startswith("text"):
            assert len(out) < len(src) // 3, (name, len(out))
        if name == "fib_literals":
            assert dynamic_header_max_lengths(members[0])[0] <= 15
            print("fib_literals: unlimited depth", ds.unlimited_depth(np.bincount(np.frombuffer(src, np.uint8), minlength=256).tolist() + [1]),
                  "max code lengths", dynamic_header_max_lengths(members[0]))
        if name == "mixed_text_random_text":
            assert dynamic_header_max_lengths(members[0]) is not None                 # (not the whole-member fallback)
            assert 16384 + 4 < len(out) < 16384 + 2 * 16384 // 3, len(out)           # the random block as it is, the text blocks compressed
            assert src[16384:32768] in out                                            # ... stored, on a byte boundary
        if name == "fib_distances":
            print("fib_distances: max code lengths", dynamic_header_max_lengths(members[0]))


def test_two_calls_give_the_same_bytes(deflater, text):
    for name, src in fixed_inputs(text).items():
        assert deflater.deflate(src) == deflater.deflate(src), name
    other = type(deflater)(deflater.path)
    assert other.deflate(text[:200000]) == deflater.deflate(text[:200000])
    other.close()


@pytest.mark.gpu
def test_device_bytes_equal_the_cpu_build(text):
    from bam_readcount_amd import capi
    hip, sim = capi.Deflater(), _sim()
    for name, src in fixed_inputs(text).items():
        assert hip.deflate(src) == sim.deflate(src), name
    assert hip.deflate(text[:2 << 20]) == sim.deflate(text[:2 << 20])


@pytest.mark.gpu
def test_many_members_in_one_call(text):
    """513 members in one call: two rounds of workgroups on 256 CUs, k_scan_sizes with three members per lane, and — the members' sizes
    differ widely — k_gather at every alignment of its destination.  The text tiled with another rotation per tile, a member of random
    bytes and a member of zeros every 50 members.  A smaller call on the same handle afterwards carries nothing over."""
    from bam_readcount_amd import capi
    n, rng = 513, np.random.default_rng(513)
    t = np.frombuffer(text, np.uint8)
    src = np.concatenate([np.roll(t, -int(rng.integers(len(t)))) for _ in range(n * M // len(t) + 1)])[:n * M].copy()
    for k in range(25, n, 50):
        src[k * M:(k + 1) * M] = rng.integers(0, 256, M, dtype=np.uint8)
        src[(k + 1) * M:(k + 2) * M] = 0
    src = src.tobytes()
    hip, sim = capi.Deflater(), _sim()
    rc, out, nm = hip.deflate_raw(src)
    assert rc == 0 and nm == n
    assert out == sim.deflate(src)
    members = check_chain(out, src)
    offs = np.concatenate([[0], np.cumsum([len(m) for m in members])])
    assert {int(o) & 3 for o in offs[:n]} == {0, 1, 2, 3}
    rc, again, nm = hip.deflate_raw(src[:257 * M])
    assert rc == 0 and nm == 257
    assert again == out[:int(offs[257])]
    hip.close()


@pytest.fixture(scope="module")
def sim_blocks(text):
    """name -> (the input, the decoded blocks of each of its members) for the fixed list on the CPU build.  What is asserted on them
    holds for the device through test_device_bytes_equal_the_cpu_build."""
    sim, res = _sim(), {}
    for name, src in fixed_inputs(text).items():
        res[name] = (src, [ds.decode(m) for m in check_chain(sim.deflate(src), src)])
    return res


def _matches(blocks):
    return [t for b in blocks for t in b.tokens if not isinstance(t, int)]


def test_new_inputs_reach_their_paths(sim_blocks):
    """The condition each built input of fixed_inputs() stands for, read from the decoded stream."""
    def one_member(name):
        src, members = sim_blocks[name]
        assert len(members) == 1, name
        return src, members[0]

    # every block of every member stands for its own BLOCK positions: no token reaches past its block's end
    for name, (src, members) in sim_blocks.items():
        for k, blocks in enumerate(members):
            n = min(M, len(src) - k * M)
            if len(blocks) == 1 and blocks[0].btype == 0:            # (the whole member as one stored block)
                assert (blocks[0].start, blocks[0].end) == (0, n), name
                continue
            assert [(b.start, b.end) for b in blocks] == [(s, min(s + BLOCK, n)) for s in range(0, max(n, 1), BLOCK)], (name, k)
            assert [b.final for b in blocks] == [0] * (len(blocks) - 1) + [1], (name, k)
            # length 3 counts within 4096 only, and no distance code beyond 32768 exists
            assert all(d <= (4096 if ln == 3 else 32768) for ln, d in _matches(blocks)), (name, k)
    # the longest distance: A again 32768 behind is matched whole, at 32769 not at all
    _, b = one_member("a_again_at_32768")
    assert b[2].btype == 1 and b[2].tokens == [(258, 32768), (42, 32768)]
    _, b = one_member("a_again_at_32769")
    assert b[2].btype == 0 and b[2].tokens == [] and b[2].end - b[2].start == 301
    _, b = one_member("a_again_at_32767")
    assert isinstance(b[1].tokens[-1], int) and b[2].tokens == [(258, 32767), (41, 32767)]
    # length 3 at 4096 and at 4097
    src, b = one_member("len3_at_4096")
    assert b[0].tokens[-1] == (3, 4096) and b[1].tokens == [(50, 4096)]
    src, b = one_member("len3_at_4097")
    assert b[0].tokens[-3:] == list(src[BLOCK - 3:BLOCK]) and all(src[BLOCK - 3:BLOCK]) and b[1].tokens == [(50, 4097)]
    assert not [t for t in _matches(b[:1]) if t[0] == 3 and t[1] > 4096]
    # a match that ends on the block's last byte, one byte before it, and matches the block's end cuts
    for back, tail in ((258, [(258, 16026)]), (259, [(258, 16025), None]), (100, [(100, 16184)]), (2, [None, None]), (1, [None])):
        src, b = one_member("p_again_%d_before_the_block_ends" % back)
        want = [src[BLOCK - len(tail) + i] if t is None else t for i, t in enumerate(tail)]
        assert b[0].tokens[-len(tail):] == want and all(src[BLOCK - min(back, 2):BLOCK]), (back, b[0].tokens[-3:])
        assert b[1].tokens[0] == (258, BLOCK - back - 100), (back, b[1].tokens[:2])
    # stored first, dynamic, stored last
    _, b = one_member("random_text_random")
    assert [x.btype for x in b] == [0, 2, 0] and b[2].final == 1
    # small members
    for n in SMALL_ZEROS:
        _, b = one_member("zeros_%d" % n)
        assert len(b) == 1 and b[0].btype == 1 and b[0].tokens == ([0, (n - 1, 1)] if n >= 5 else [0] * n), n
    for extra, want in ((1, [0]), (3, [0, 0, 0]), (4, [(4, 1)])):
        _, b = one_member("zeros_%d" % (BLOCK + extra))
        assert len(b) == 2 and b[1].btype == 1 and b[1].tokens == want, extra
    for n in TEXT_SIZES:
        src, b = one_member("short_text_%d" % n)
        assert len(src) == n
        if 15 <= n <= 33:
            assert len(b) == 1 and b[0].btype == 1 and _matches(b), n
        if 255 <= n <= 257:
            assert len(b) == 1 and b[0].btype == 2, n
    _, b = one_member("abc_four_times")
    assert len(b) == 1 and b[0].btype == 1 and b[0].tokens == [97, 98, 99, (9, 3)]


def _block_histograms(b):
    """the counts a block's own tokens give the two alphabets (with the end-of-block code)"""
    lit, dist = [0] * 286, [0] * 30
    lit[256] = 1
    for t in b.tokens:
        if isinstance(t, int):
            lit[t] += 1
        else:
            lit[257 + im.len_symbol(t[0])] += 1; dist[im.dist_symbol(t[1])] += 1
    return lit, dist


def test_every_encoder_path_is_reached(sim_blocks):
    """A census of the paths of brc_deflate_core.h the fixed list reaches on the CPU build — a condition on the INPUTS: when the
    compressor changes and an input no longer reaches its path, this says which, and the suite does not silently cover less.  The
    deepest codes emitted are printed next to the depth an unlimited code would have had (no input reaches the 15-bit limiter: DESIGN.md 6b;
    test_length_limiter_on_the_device runs it)."""
    seen, deepest = set(), {"literal/length": (0, 0, ""), "distance": (0, 0, ""), "code length": (0, 0, "")}
    nblocks = [0, 0, 0]
    for name, (src, members) in sim_blocks.items():
        for k, blocks in enumerate(members):
            if len(blocks) == 1 and blocks[0].btype == 0 and len(src) - k * M > BLOCK:
                seen.add("a member replaced by one stored block")
            seen.add("last block of type %d" % blocks[-1].btype)
            for a, b in zip(blocks, blocks[1:]):
                seen.add("type %d followed by type %d" % (a.btype, b.btype))
            for b in blocks:
                seen.add("block type %d" % b.btype); nblocks[b.btype] += 1
                for ln, d in _matches([b]):
                    if ln in (3, 258):
                        seen.add("length %d" % ln)
                    if d == 32768:
                        seen.add("distance 32768")
                    if im.dist_symbol(d) == 29:
                        seen.add("distance code 29")
                if b.btype != 2:
                    continue
                seen.add("hlit %d" % b.hlit); seen.add("hdist %d" % b.hdist); seen.add("hclen %d" % b.hclen)
                lit, dist = _block_histograms(b)
                assert [bool(x) for x in b.lit_lens] == [bool(x) for x in lit[:b.hlit]] and not any(lit[b.hlit:]), name
                used = [j for j, c in enumerate(dist) if c]
                if not used:
                    assert b.dist_lens == [0], name
                    seen.add("no distance code")
                elif len(used) == 1:                                    # completed by a second code of one bit: symbol 1 next to symbol 0, else symbol 0
                    other = 1 if used[0] == 0 else 0
                    assert b.dist_lens == [1 if j in (used[0], other) else 0 for j in range(b.hdist)], name
                    seen.add("a single distance code, symbol 0" if used[0] == 0 else "a single distance code, not symbol 0")
                for s in b.cl_seq:
                    if not isinstance(s, int) and s[1] in {16: (3, 6), 17: (3, 10), 18: (11, 138)}[s[0]]:
                        seen.add("code-length symbol %d with %d repeats" % s)
                clh = [0] * 19
                for s in b.cl_seq:
                    clh[s if isinstance(s, int) else s[0]] += 1
                need = ds.unlimited_depth(clh)
                if need > 7 and max(b.cl_lens) == 7:
                    seen.add("the 7-bit limiter engaged")
                for what, lens, hist in (("literal/length", b.lit_lens, lit), ("distance", b.dist_lens, dist), ("code length", b.cl_lens, clh)):
                    deepest[what] = max(deepest[what], (max(lens), ds.unlimited_depth(hist), name))
    print("census: %d members of %d inputs; blocks stored %d, fixed %d, dynamic %d" % (sum(len(m) for _, m in sim_blocks.values()), len(sim_blocks), *nblocks))
    for what, (got, need, name) in deepest.items():
        print("census: deepest %s code emitted %d bits (an unlimited code of that block: %d), in %s" % (what, got, need, name))
    print("census: hclen seen", sorted(int(s.split()[1]) for s in seen if s.startswith("hclen")))
    want = (["block type %d" % t for t in range(3)] + ["last block of type %d" % t for t in range(3)]
            + ["type 0 followed by type 2", "type 2 followed by type 0", "a member replaced by one stored block",
               "distance code 29", "distance 32768", "hdist 30", "hdist 1", "no distance code",
               "a single distance code, symbol 0", "a single distance code, not symbol 0", "hlit 257", "hlit 286", "length 258", "length 3"]
            + ["code-length symbol %d with %d repeats" % (s, r) for s, r in ((16, 3), (16, 6), (17, 3), (17, 10), (18, 11), (18, 138))]
            + ["the 7-bit limiter engaged"])
    missing = [w for w in want if w not in seen]
    assert not missing, missing


def _zlib_pieces(data, level, strategy):
    total = 0
    for o in range(0, len(data), M):
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
        total += len(c.compress(data[o:o + M]) + c.flush()) + 26
    return total


def test_compression_floor(deflater, text):
    """A condition: on the product's own text the members are no larger than zlib's Z_HUFFMAN_ONLY on the same pieces (26 bytes of
    framing per member on both sides).  The ratio to zlib level 1 is printed, not asserted."""
    out = deflater.deflate(text)
    check_chain(out[:0], b"")
    members, _ = im.split_members(out, decode=False)
    assert b"".join(zlib.decompress(m, 31) for m in members) == text
    floor = _zlib_pieces(text, 6, zlib.Z_HUFFMAN_ONLY)
    z1 = _zlib_pieces(text, 1, zlib.Z_DEFAULT_STRATEGY)
    print("deflate: %d bytes of text -> %d; Z_HUFFMAN_ONLY %d; zlib level 1 %d; ratio to level 1 %.3f" % (len(text), len(out), floor, z1, len(out) / z1))
    assert len(out) <= floor, (len(out), floor)


def test_abi_edges(deflater):
    from bam_readcount_amd import capi
    assert deflater.kind() in ("sim", "hip-gfx950")
    assert deflater.eof_block() == EOF_BLOCK == im.EOF_MEMBER
    assert zlib.decompress(deflater.eof_block(), 31) == b""
    # the bound: every member stored
    for n in (0, 1, M - 1, M, M + 1, 10 * M + 7):
        assert deflater.bound(n) == n + 31 * ((n + M - 1) // M)
    src = b"hello, world\n" * 9000            # two members
    rc, out, nm = deflater.deflate_raw(src)
    assert rc == 0 and nm == 2
    check_chain(out, src)
    # dst_cap below the bound: BRC_E_ARG, nothing written
    rc, out, nm = deflater.deflate_raw(src, dst_cap=deflater.bound(len(src)) - 1)
    assert rc == capi.E_ARG and out == b"\xa5" * (deflater.bound(len(src)) - 1)
    # a NULL handle
    rc, out, nm = deflater.deflate_raw(src, handle=False)
    assert rc == capi.E_ARG and set(out) == {0xA5}
    # no input: no member
    rc, out, nm = deflater.deflate_raw(b"")
    assert rc == 0 and out == b"" and nm == 0
    # two deflaters alive at once
    other = capi.Deflater(deflater.path)
    assert other.deflate(src) == deflater.deflate(src)
    other.close()
    t = deflater.last_timing()
    assert t["bytes_in"] == len(src) and 0 < t["bytes_out"] < len(src) and t["call_s"] >= t["kernel_s"] >= 0


def test_product_library_without_a_device_says_so():
    """Not gpu-marked: where there is no GPU the product library has no CPU path to return to.  Skips where a device exists."""
    from bam_readcount_amd import capi
    assert os.path.exists(capi.DEFLATE_LIB), "libbrc_deflate_hip.so is not built (make -C bam_readcount_amd/csrc)"
    try:
        d = capi.Deflater()
    except capi.BrcError as e:
        assert getattr(e, "rc", None) == capi.E_NODEVICE
        return
    d.close()
    pytest.skip("a device exists here: the [hip] tests cover the product library")


def test_seeded_fuzz_under_the_host_sanitizers(tmp_path, text):
    """300 seeded inputs — text-like, binary and mixed, lengths around the member boundaries — through the CPU build with
    -fsanitize=address,undefined: no report, and zlib returns every input."""
    subprocess.check_call(["make", "-s", "-C", SIM_DIR, "asan"])
    rng = np.random.default_rng(20250311)
    cases = []
    lengths = [0, 1, 2, 3, 4, 5, 15, 16, 17, 255, 256, 257, 258, 259, 16383, 16384, 16385, M - 1, M, M + 1, 2 * M - 1, 2 * M, 2 * M + 1]
    for i in range(300):
        n = lengths[i % len(lengths)] if i < 3 * len(lengths) else int(rng.integers(0, 3 * M))
        kind = i % 3
        if kind == 0:
            o = int(rng.integers(0, len(text) - n - 1)); c = text[o:o + n]
        elif kind == 1:
            c = rng.integers(0, int(rng.choice([2, 4, 16, 256])), n, dtype=np.uint8).tobytes()
        else:
            o = int(rng.integers(0, len(text) - n - 1)); a = bytearray(text[o:o + n])
            for _ in range(int(rng.integers(0, 6))):
                if n:
                    p = int(rng.integers(0, n)); q = min(n, p + int(rng.integers(1, 3000)))
                    a[p:q] = rng.integers(0, 256, q - p, dtype=np.uint8).tobytes() if rng.random() < 0.5 else bytes([int(rng.integers(0, 256))]) * (q - p)
            c = bytes(a)
        cases.append(c)
    with open(tmp_path / "cases.bin", "wb") as f:
        for c in cases:
            f.write(struct.pack("<I", len(c))); f.write(c)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([os.path.join(SIM_DIR, "deflate_check_asan"), str(tmp_path / "cases.bin"), str(tmp_path / "res.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    assert p.stdout.decode().strip() == "300 cases"
    d = open(tmp_path / "res.bin", "rb").read(); o = 0
    for c in cases:
        rc, nm, got = struct.unpack_from("<iQQ", d, o); o += 20
        assert rc == 0 and nm == (len(c) + M - 1) // M
        check_chain(d[o:o + got], c); o += got
    assert o == len(d)


def _limited(counts, maxbits):
    subprocess.check_call(["make", "-s", "-C", SIM_DIR, "limit_check"])
    p = subprocess.run([os.path.join(SIM_DIR, "limit_check"), str(maxbits)] + [str(c) for c in counts], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return [int(x) for x in p.stdout.split()]


def _prefix_code_round_trip(lens, symbols):
    """Canonical codes from the lengths (RFC 1951 3.2.2), the symbols written with them and read back bit by bit."""
    code, codes = 0, {}
    for ln in range(1, max(lens) + 1):
        for s, l in enumerate(lens):
            if l == ln:
                codes[s] = format(code, "0%db" % ln); code += 1
        code <<= 1
    bits = "".join(codes[s] for s in symbols)
    back, rev, cur = [], {v: k for k, v in codes.items()}, ""
    for b in bits:
        cur += b
        if cur in rev:
            back.append(rev[cur]); cur = ""
    return back == list(symbols) and cur == ""


def _fibonacci_histograms():
    """(symbols of the alphabet, symbols used, the limit, the counts, the used symbols, a message over them): counts that follow the
    Fibonacci numbers over 23 literal/length symbols, 23 distance symbols and 12 symbols of the code-length code"""
    rng, out = np.random.default_rng(3), []
    for nsym, used, maxbits in ((286, 23, 15), (30, 23, 15), (19, 12, 7)):
        counts = [0] * nsym
        where = sorted(rng.choice(nsym, used, replace=False).tolist())
        for s, f in zip(rng.permutation(where).tolist(), _fib(used)):
            counts[s] = f
        out.append((nsym, used, maxbits, counts, where, rng.choice(where, 3000).tolist() + where))
    return out


def test_length_limiter_on_fibonacci_counts():
    """Counts that follow the Fibonacci numbers over 23 literals (a member's worth cannot be one 16-k block of this compressor, so the
    counts go to the limiter itself, as the kernel hands them over): an unlimited Huffman code is 22 bits deep; the limiter's lengths
    stay within 15, use all 15, form a complete prefix code that gives rarer symbols no shorter codes, and a message written
    with them reads back.  The same over 23 distance symbols of 30, and for the 7-bit code-length code over 12 of its 19 symbols."""
    for nsym, used, maxbits, counts, where, msg in _fibonacci_histograms():
        assert ds.unlimited_depth(counts) == used - 1 > maxbits
        lens = _limited(counts, maxbits)
        assert len(lens) == nsym and all((l > 0) == (c > 0) for l, c in zip(lens, counts))
        assert max(lens) == maxbits
        assert sum(2 ** (maxbits - l) for l in lens if l) == 2 ** maxbits              # Kraft: complete, nothing over-subscribed
        # rarer symbols never get shorter codes
        order = sorted((c, l) for c, l in zip(counts, lens) if c)
        assert all(a[1] >= b[1] for a, b in zip(order, order[1:]))
        import heapq
        h = [(c, 0) for c in counts if c]; heapq.heapify(h); best = 0
        while len(h) > 1:
            a, b = heapq.heappop(h), heapq.heappop(h); best += a[0] + b[0]; heapq.heappush(h, (a[0] + b[0], 0))
        cost = sum(c * l for c, l in zip(counts, lens))
        # no prefix code beats the unlimited Huffman code; a code within the limit costs at most `maxbits` per symbol (the fix-up is
        # a heuristic, not package-merge: how close it comes to the best limited code is printed, not asserted)
        assert best <= cost <= maxbits * sum(counts), (cost, best)
        print("limiter: %d symbols, limit %d: cost %d, unlimited %d (%.3f)" % (used, maxbits, cost, best, cost / best))
        assert _prefix_code_round_trip(lens, msg)
    # counts that need no limiting come out as the unlimited code
    lens = _limited([5, 1, 1, 2, 8, 0, 3], 15)
    assert sum(c * l for c, l in zip([5, 1, 1, 2, 8, 0, 3], lens)) == 45 and lens[5] == 0


def _steep_histogram(rng, nsym, maxbits):
    """Counts whose unlimited Huffman code is deeper than maxbits: a chain of Fibonacci numbers, each times a small factor, on a random
    subset of the alphabet, and any number of further symbols with counts of the same kind."""
    while True:
        chain = int(rng.integers(maxbits + 2, min(nsym, maxbits + 14) + 1))
        more = int(rng.integers(0, nsym - chain + 1)) if rng.random() < 0.5 else 0
        fib = _fib(chain)
        values = [f * int(rng.integers(1, 4)) for f in fib] + [fib[int(rng.integers(chain))] * int(rng.integers(1, 4)) for _ in range(more)]
        counts = [0] * nsym
        for s, v in zip(rng.choice(nsym, chain + more, replace=False).tolist(), values):
            counts[s] = v
        if ds.unlimited_depth(counts) > maxbits:
            return counts


def _limiter_cases():
    """Three histograms a case (literal/length, distance, code length: limits 15, 15, 7), every one deeper than its limit: the Fibonacci
    counts of test_length_limiter_on_fibonacci_counts, then 200 seeded cases."""
    rng = np.random.default_rng(1951)
    return [[h[3] for h in _fibonacci_histograms()]] + [[_steep_histogram(rng, nsym, maxbits) for nsym, maxbits in ((286, 15), (30, 15), (19, 7))] for _ in range(200)]


def _host_lengths(cases, program):
    """The 335 code lengths of every case from a host build of limit_check.cpp, one start of the program."""
    subprocess.check_call(["make", "-s", "-C", SIM_DIR, program])
    lines = ["%d %s\n" % (maxbits, " ".join(map(str, h))) for c in cases for h, maxbits in zip(c, (15, 15, 7))]
    p = subprocess.run([os.path.join(SIM_DIR, program), "-"], input="".join(lines).encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    host = [[int(x) for x in ln.split()] for ln in p.stdout.decode().splitlines()]
    assert [len(h) for h in host] == [286, 30, 19] * len(cases)
    return [host[3 * k] + host[3 * k + 1] + host[3 * k + 2] for k in range(len(cases))]


def _check_limited_cases(cases, lengths):
    assert len(lengths) == len(cases)
    for k, (c, d) in enumerate(zip(cases, lengths)):
        assert len(d) == 335, k
        for counts, lens, maxbits in zip(c, (d[:286], d[286:316], d[316:]), (15, 15, 7)):
            assert ds.unlimited_depth(counts) > maxbits
            assert len(lens) == len(counts) and all((l > 0) == (n > 0) for l, n in zip(lens, counts)), k
            assert max(lens) == maxbits, k
            assert sum(2 ** (maxbits - l) for l in lens if l) == 2 ** maxbits, k         # Kraft: complete, nothing over-subscribed
            order = sorted((n, -l) for n, l in zip(counts, lens) if n)                   # a rarer symbol never has the shorter code
            assert all(a[1] <= b[1] for a, b in zip(order, order[1:])), k


def test_length_limiter_on_seeded_counts():
    """The cases of test_length_limiter_on_the_device through the host build under the sanitizers: no report, and the properties hold."""
    cases = _limiter_cases()
    _check_limited_cases(cases, _host_lengths(cases, "limit_check"))


@pytest.mark.gpu
def test_length_limiter_on_the_device(tmp_path):
    """No input of the suite brings a block's own histogram beyond 13 bits (test_every_encoder_path_is_reached prints the depths), so
    inside the compressor the limiter never runs.  limit_check_hip runs limited_lengths() on the device as deflate_member() does: a
    workgroup of 256 lanes per case, lane 0 on the literal/length counts while lane 64 is on the distance counts, then lane 0 on the
    code-length counts at 7 bits, on the arrays of brcdef::Shared in LDS.  The device's lengths are those of the host build of the same
    function (limit_check.cpp without the sanitizers: they stay on the CPU suite, test_length_limiter_on_seeded_counts), and the
    properties hold.  The program is started once, under a time limit."""
    cases = _limiter_cases()
    host = _host_lengths(cases, "limit_check_plain")
    subprocess.check_call(["make", "-s", "-C", SIM_DIR, "limit_check_hip"])
    with open(tmp_path / "cases.txt", "w") as f:
        for c in cases:
            f.write(" ".join(str(x) for h in c for x in h) + "\n")
    p = subprocess.run(["timeout", "-k", "10", "60", os.path.join(SIM_DIR, "limit_check_hip"), str(tmp_path / "cases.txt")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, (p.returncode, p.stderr.decode()[-2000:])
    device = [[int(x) for x in ln.split()] for ln in p.stdout.decode().splitlines()]
    assert device == host
    _check_limited_cases(cases, device)
