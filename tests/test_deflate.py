"""The BGZF deflater (include/brc_deflate.h): the compressor of bam_readcount_amd/csrc/brc_deflate_core.h behind its C-ABI, on the GPU
([hip]: libbrc_deflate_hip.so) and lane for lane on the CPU ([sim]: tests/sim_deflate).  The references are zlib (zlib.decompress with
wbits 31, member by member) and the repository's own inflater; equality is byte for byte.  The compression floor is zlib's
Z_HUFFMAN_ONLY on the same 0xff00 pieces: no encoder without a working match stage gets under it.

The seeded fuzz runs on the CPU build under the host sanitizers only; the GPU sees the fixed list."""
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

SIM_DIR = os.path.join(ROOT, "tests", "sim_deflate")
SIM_LIB = os.path.join(SIM_DIR, "libbrc_deflate_sim.so")
SIM_INFLATE_DIR = os.path.join(ROOT, "tests", "sim_inflate")
M = 0xff00
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


def unlimited_huffman_depth(counts):
    """The longest code of a Huffman code without a length limit for these counts (zeros take no part)."""
    import heapq
    h = [(c, 0) for c in counts if c]
    heapq.heapify(h)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        heapq.heappush(h, (a[0] + b[0], max(a[1], b[1]) + 1))
    return h[0][1]


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
    return {
        "empty": b"", "one": b"Q",
        "text_m-1": text[:M - 1], "text_m": text[1000:1000 + M], "text_m+1": text[5000:5000 + M + 1], "text_3m": text[70000:70000 + 3 * M],
        "zeros": bytes(65280), "period2": b"xy" * 30001, "period3": b"abc" * 21000,
        "period259": rng.integers(0, 256, 259, dtype=np.uint8).tobytes() * 250,
        "random": rng.integers(0, 256, 65280, dtype=np.uint8).tobytes(), "all256": bytes(range(256)),
        "high": rng.integers(144, 256, 50000, dtype=np.uint8).tobytes(), "fib_literals": fib_lit, "fib_distances": bytes(out),
        # a block of text, a block no code shortens, a block of text: the middle one stays a stored block inside the stream
        "mixed_text_random_text": text[:16384] + rng.integers(0, 256, 16384, dtype=np.uint8).tobytes() + text[16384:32768],
    }


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
    """(max literal/length code length, max distance code length) of the FIRST dynamic block of a member, None when it is not dynamic."""
    d = m[18:-8]; pos = [0]

    def bits(n):
        v = 0
        for i in range(n):
            v |= ((d[pos[0] >> 3] >> (pos[0] & 7)) & 1) << i; pos[0] += 1
        return v
    if (bits(3) >> 1) != 2:
        return None
    hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
    cl = [0] * 19
    for i in range(hclen):
        cl[[16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15][i]] = bits(3)
    code, table = 0, {}
    for ln in range(1, 8):
        for s in range(19):
            if cl[s] == ln:
                table[(ln, code)] = s; code += 1
        code <<= 1
    lens = []
    while len(lens) < hlit + hdist:
        c, ln = 0, 0
        while (ln, c) not in table:
            c = c << 1 | bits(1); ln += 1
            assert ln <= 7
        s = table[(ln, c)]
        if s < 16:
            lens.append(s)
        elif s == 16:
            lens += [lens[-1]] * (3 + bits(2))
        else:
            lens += [0] * ((3 + bits(3)) if s == 17 else (11 + bits(7)))
    assert len(lens) == hlit + hdist
    return max(lens[:hlit]), max(lens[hlit:])


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
            print("fib_literals: unlimited depth", unlimited_huffman_depth(np.bincount(np.frombuffer(src, np.uint8), minlength=256).tolist() + [1]),
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


def test_length_limiter_on_fibonacci_counts():
    """Counts that follow the Fibonacci numbers over 23 literals (a member's worth cannot be one 16-k block of this compressor, so the
    counts go to the limiter itself, as the kernel hands them over): an unlimited Huffman code is 22 bits deep; the limiter's lengths
    stay within 15, use all 15, form a complete prefix code that gives rarer symbols no shorter codes, and a message written
    with them reads back.  The same over 23 distance symbols of 30, and for the 7-bit code-length code over 12 of its 19 symbols."""
    rng = np.random.default_rng(3)
    for nsym, used, maxbits in ((286, 23, 15), (30, 23, 15), (19, 12, 7)):
        counts = [0] * nsym
        where = sorted(rng.choice(nsym, used, replace=False).tolist())
        for s, f in zip(rng.permutation(where).tolist(), _fib(used)):
            counts[s] = f
        assert unlimited_huffman_depth(counts) == used - 1 > maxbits
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
        msg = rng.choice(where, 3000).tolist() + where
        assert _prefix_code_round_trip(lens, msg)
    # counts that need no limiting come out as the unlimited code
    lens = _limited([5, 1, 1, 2, 8, 0, 3], 15)
    assert sum(c * l for c, l in zip([5, 1, 1, 2, 8, 0, 3], lens)) == 45 and lens[5] == 0
