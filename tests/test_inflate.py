"""The BGZF inflater (include/brc_inflate.h): the decoder of bam_readcount_amd/csrc/brc_inflate_core.h behind its C-ABI, on the GPU
([hip]: libbrc_inflate_hip.so) and lane for lane on the CPU ([sim]: tests/sim_inflate).  The reference is zlib itself
(zlib.decompress(payload, -15), zlib.crc32); equality is byte for byte.

zlib's COMPRESSOR writes only part of what RFC 1951 allows (never a block without a distance code or with a single one, never a run of
code lengths across the two tables, ...), so next to the members it makes stand streams written WITHOUT it: by the hand encoder of
tools/fuzz/inflate_members.py (handmade_cases: a fixed list at the format's corners and at the decoder's own boundaries; random_valid: a
seeded generator).  The reference for those is zlib's DECODER: every such stream must first be accepted by zlib.decompressobj(-15) and
give the bytes the builder meant ("builder wrong" otherwise), then the inflater must give the same bytes.

The malformed members are a fixed list, each with the status the FORMAT demands (RFC 1951 / RFC 1952 / SAMv1 4.1; the reasoning
stands next to each case).  They are error paths of a total decoder: the list first runs on the CPU build under the host sanitizers
(every step outside a member's payload or slot would be a report), then on the plain CPU build, then — the identical list, once — on
the GPU.  The random-corruption fuzz runs under the sanitizers only; the random valid streams run there first, then a part of them
through [sim] and [hip]."""
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tools", "fuzz"))
import inflate_members as im  # noqa: E402  (member builders, the malformed list, the mutator: shared with tools/fuzz)

SIM_DIR = os.path.join(ROOT, "tests", "sim_inflate")
SIM_LIB = os.path.join(SIM_DIR, "libbrc_inflate_sim.so")


@pytest.fixture(scope="module", params=["sim", pytest.param("hip", marks=pytest.mark.gpu)])
def inflater(request):
    """[hip]: the product's inflater library (fails loudly when it was not built or has no device); [sim]: the CPU build."""
    from bam_readcount_amd import capi
    if request.param == "hip":
        inf = capi.Inflater()
        assert inf.kind() == "hip-gfx950"
        return inf
    subprocess.check_call(["make", "-s", "-C", SIM_DIR])
    inf = capi.Inflater(SIM_LIB)
    assert inf.kind() == "sim"
    return inf


def _payloads():
    rng = np.random.default_rng(11)
    bam = b"".join(im.split_members(open(os.path.join(GOLDEN, "test.bam"), "rb").read())[1])
    return {
        "empty": b"", "one": b"Q", "zeros": bytes(65280), "random": rng.integers(0, 256, 65280, dtype=np.uint8).tobytes(),
        "period32768": rng.integers(0, 256, 32768, dtype=np.uint8).tobytes() * 2,          # matches at the maximum distance
        "runs258": b"".join(bytes([65 + i % 7]) * 777 for i in range(80)),                  # long runs: length-258 matches
        "bam": bam[1000:1000 + 65280], "acgt": rng.choice(np.frombuffer(b"ACGT", np.uint8), 65536).tobytes(),
        "full65536": rng.integers(0, 4, 65536, dtype=np.uint8).tobytes(),
    }


STRATEGIES = [(0, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY),
              (6, zlib.Z_FIXED), (6, zlib.Z_HUFFMAN_ONLY), (6, zlib.Z_RLE)]


def test_known_answer_members(inflater):
    """Every payload x every way zlib can write it (stored, fast, default, best, fixed codes, Huffman only, RLE = distance-1 matches that
    overlap their own output), a full flush in the middle (several deflate blocks, an empty stored block), ISIZE 0 / 1 / 65280 / 65536,
    extra subfields before and after BC: output == payload, status ok."""
    pay = _payloads()
    members, want = [], []
    for level, strategy in STRATEGIES:
        for name, p in pay.items():
            m = im.member(p, level, strategy)
            if m is None:          # (does not fit a member: incompressible bytes stored with their 5-byte block headers)
                p = p[:65000]; m = im.member(p, level, strategy)
            members.append(m); want.append(p)
    for name in ("bam", "runs258", "acgt"):
        members.append(im.member(pay[name], 6, zlib.Z_DEFAULT_STRATEGY, flush_at=(len(pay[name]) // 3, 2 * len(pay[name]) // 3))); want.append(pay[name])
    members.append(im.EOF_MEMBER); want.append(b"")
    assert len(im.EOF_MEMBER) == 28
    for p in (b"", b"x", pay["bam"], pay["full65536"]):
        members.append(im.member(p, 6, zlib.Z_DEFAULT_STRATEGY, extra_before=b"XY\x03\x00abc", extra_after=b"ZZ\x00\x00")); want.append(p)
    assert all(m is not None and len(m) <= 65536 for m in members)
    sizes = {len(w) for w in want}
    assert {0, 1, 65280, 65536} <= sizes
    out, off, st = inflater.inflate(b"".join(members))
    assert st.tolist() == [0] * len(members)
    assert off.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    for i, w in enumerate(want):
        assert out[int(off[i]):int(off[i + 1])] == w, i
    # one at a time too (a slot that starts at offset 0)
    for m, w in list(zip(members, want))[::9]:
        o1, f1, s1 = inflater.inflate(m)
        assert s1.tolist() == [0] and o1 == w


def test_whole_files_in_one_call(inflater, tmp_path):
    """Every member of the golden BAMs and of a BAM of thousands of small blocks, one call per file; dst_off is the ISIZE prefix sum."""
    import bamio
    import synth
    rng = np.random.default_rng(3)
    ref = synth.make_ref(rng, 60000)
    arrs = synth.make_batch(78, ref, 40000, style="indel")
    bamio.write_bam(str(tmp_path / "many.bam"), [("chrA", 60000)], arrs, np.zeros(len(arrs["pos"]), int), block_bytes=3000)
    for path, least in ((os.path.join(GOLDEN, "test.bam"), 8), (os.path.join(GOLDEN, "test_bad_rg.bam"), 8), (str(tmp_path / "many.bam"), 2000)):
        raw = open(path, "rb").read()
        members, payloads = im.split_members(raw)
        assert len(members) >= least, (path, len(members))
        out, off, st = inflater.inflate(raw)
        assert len(st) == len(members) and not st.any()
        isize = [struct.unpack("<I", m[-4:])[0] for m in members]
        assert off.tolist() == np.concatenate([[0], np.cumsum(isize)]).tolist()
        assert out == b"".join(payloads)


def _check_case(case, rc, n, st, out):
    assert rc == case.rc, (case.name, rc)
    assert n == len(case.status) and list(st) == case.status, (case.name, n, list(st))
    o = 0
    for k, (s, w) in enumerate(zip(case.status, case.outputs)):
        if s == 0:
            assert out[o:o + len(w)] == w, (case.name, k)
        else:
            assert out[o:o + case.slots[k]] == b"\xa5" * case.slots[k], (case.name, k, "a failed member wrote into its slot")
        o += case.slots[k]


def _run_asan(cases, tmp_path):
    subprocess.check_call(["make", "-s", "-C", SIM_DIR, "asan"])
    with open(tmp_path / "cases.bin", "wb") as f:
        for c in cases:
            f.write(struct.pack("<I", len(c))); f.write(c)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([os.path.join(SIM_DIR, "inflate_check_asan"), str(tmp_path / "cases.bin"), str(tmp_path / "res.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    assert p.stdout.decode().strip() == "%d cases" % len(cases)
    d = open(tmp_path / "res.bin", "rb").read(); o = 0; res = []
    for _ in cases:
        rc, n = struct.unpack_from("<iI", d, o); o += 8
        st = list(d[o:o + n]); o += n
        total, = struct.unpack_from("<Q", d, o); o += 8
        res.append((rc, n, st, d[o:o + total])); o += total
    assert o == len(d)
    return res


def test_malformed_members_under_the_host_sanitizers(tmp_path):
    cases = im.malformed_cases()
    assert len(cases) >= 30 and set(im.HANDMADE_MALFORMED) <= {c.name for c in cases}
    for case, (rc, n, st, out) in zip(cases, _run_asan([c.chain for c in cases], tmp_path)):
        _check_case(case, rc, n, st, out)


def test_malformed_members(inflater):
    """The fixed list, each case with its expected status; the good members of the same call come out right; a failed member leaves its
    slot untouched.  ([hip] runs it once, after the sanitizer build and the CPU build have passed the same list.)"""
    for case in im.malformed_cases():
        rc, out, off, st, n = inflater.inflate_raw(case.chain)
        _check_case(case, rc, n, st, out)


def test_added_malformed_cases_are_refused_by_zlib():
    """The hand-built malformed streams of the list (im.handmade_malformed) are what they claim to be: zlib's decoder refuses each —
    it raises, or, for the stream without a final block, never reaches the end — and each expects the status the format demands."""
    cases = {c.name: c for c in im.malformed_cases()}
    assert len(im.HANDMADE_MALFORMED) == 12
    for name in im.HANDMADE_MALFORMED:
        case = cases[name]
        assert case.status == [0, im.TRUNCATED if name == "no_final_block" else im.BAD_STREAM, 0], name
        raw = im.payload_of(im.split_members(case.chain, decode=False)[0][1])
        d = zlib.decompressobj(-15)
        try:
            d.decompress(raw)
        except zlib.error:
            continue
        assert not d.eof, ("builder wrong: zlib takes it", name)


def _members_checked_by_zlib(cases):
    """(name, raw deflate, the bytes the builder meant) -> members, after zlib's decoder has agreed with the builder about every one"""
    members = []
    for name, raw, want in cases:
        d = zlib.decompressobj(-15)
        try:
            got = d.decompress(raw)
        except zlib.error as e:
            raise AssertionError(("builder wrong: zlib refuses it", name, str(e)))
        assert d.eof and got == want, ("builder wrong", name, d.eof, len(got), len(want))
        assert d.unused_data == (raw[-3:] if name == im.TRAILING else b""), ("builder wrong", name)
        m = im.wrap(raw, zlib.crc32(got), len(got))
        assert m is not None, ("builder wrong: does not fit a member", name)
        members.append(m)
    return members


def _inflate_and_compare(inflater, names, members, want):
    out, off, st = inflater.inflate(b"".join(members))
    assert st.tolist() == [0] * len(members), [(names[i], s) for i, s in enumerate(st.tolist()) if s]
    assert off.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    for i, w in enumerate(want):
        assert out[int(off[i]):int(off[i + 1])] == w, names[i]


def test_handmade_valid_streams(inflater):
    """Valid streams written by hand (im.handmade_cases), none by zlib's compressor: one distance code of one bit, no distance code, the
    end-of-block code alone, 15-bit codes on both tables, the fewest and the most code-length lengths, runs of code lengths across the
    two tables (16, 17, 18), every length and distance symbol at both ends of its extra bits, matches over their own output around 64,
    blocks that end around the token batches, thousands of blocks, stored blocks at every bit offset, bytes behind the final block.
    zlib's decoder is the reference; all of them in one call, a stride of them one at a time."""
    cases = im.handmade_cases()
    names = [c[0] for c in cases]
    assert len(set(names)) == len(names) >= 28 and im.TRAILING in names
    want = [c[2] for c in cases]
    assert {0, 65536} <= {len(w) for w in want}
    members = _members_checked_by_zlib(cases)
    _inflate_and_compare(inflater, names, members, want)
    for name, m, w in list(zip(names, members, want))[::3]:
        o1, f1, s1 = inflater.inflate(m)
        assert s1.tolist() == [0] and f1.tolist() == [0, len(w)] and o1 == w, name


def test_slot_geometry(inflater):
    """The CRC32 (ceil(ISIZE / 64) bytes per lane, lanes without bytes) and the store to dst (bytes up to the first 16-byte boundary,
    16-byte stores, the rest): members of every ISIZE 0..130, 255..257, 4095..4097 behind a leading member of 0..16 bytes, every group a
    multiple of 16 bytes long, so that every ISIZE up to 48 begins at every offset modulo 16.  (zlib-made members: the decoder is not the
    subject.)  Bytes equal, dst_off equal, and the 64 bytes of dst behind the last member still hold their fill."""
    rng = np.random.default_rng(16)
    sizes = list(range(131)) + [255, 256, 257, 4095, 4096, 4097]
    want = []
    for a in range(17):
        group = [a] + sizes
        group.append(-sum(group) % 16)
        want += [rng.integers(65, 81, n, dtype=np.uint8).tobytes() for n in group]
    members = [im.member(w, 6) for w in want]
    offs = np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    assert {(o % 16, len(w)) for o, w in zip(offs, want)} >= {(r, n) for r in range(16) for n in range(49)}
    total = offs[-1]
    rc, out, off, st, n = inflater.inflate_raw(b"".join(members), dst_cap=total + 64, whole=True)
    assert rc == 0 and n == len(members) and not st.any()
    assert off.tolist() == offs
    assert len(out) == total + 64 and out[total:] == b"\xa5" * 64
    for i, w in enumerate(want):
        assert out[offs[i]:offs[i + 1]] == w, (i, offs[i] % 16, len(w))


RANDOM_VALID_SEED = 19510596


def _random_valid_checked(count):
    rv = im.random_valid(RANDOM_VALID_SEED, count)
    names = ["random_valid_%d" % i for i in range(count)]
    members = _members_checked_by_zlib([(n, raw, w) for n, (raw, w, _) in zip(names, rv)])      # (fails on the first one zlib does not take)
    return rv, names, members


def test_random_valid_streams_under_the_host_sanitizers(tmp_path):
    """2000 seeded valid streams of the generator (random complete code sets down to 15 bits and the two incomplete distance sets the
    format allows, random tokens, random runs in the header), every one accepted by zlib's decoder; eight members to a chain through
    the sanitizer build: status ok and zlib's bytes.  At least 100 of them each have a lone distance code, no distance code, a run
    across the two tables."""
    rv, names, members = _random_valid_checked(2000)
    for tag in ("lone", "none", "crossing"):
        assert sum(tag in tags for _, _, tags in rv) >= 100, tag
    assert max(len(w) for _, w, _ in rv) <= 4096
    chains = [b"".join(members[i:i + 8]) for i in range(0, len(members), 8)]
    for k, (rc, n, st, out) in enumerate(_run_asan(chains, tmp_path)):
        part = rv[8 * k:8 * k + 8]
        assert rc == 0 and n == len(part) and st == [0] * n, (names[8 * k], rc, n, st)
        assert out == b"".join(w for _, w, _ in part), names[8 * k]


def test_random_valid_streams(inflater):
    """The first 200 of the same streams in one call."""
    rv, names, members = _random_valid_checked(200)
    _inflate_and_compare(inflater, names, members, [w for _, w, _ in rv])


def test_random_corruption_fuzz_under_the_host_sanitizers(tmp_path):
    """A few thousand seeded mutations (bit flips, byte changes, cuts and swaps inside the payload, trailer flips) of small members, CPU
    sanitizer build only: the decoder ends with a status every time, stays inside its bounds, and whenever it says ok its bytes are
    the ones zlib gets from the same mutated payload and their CRC32 is the trailer's."""
    chains, meta = im.mutations(seed=20240607, count=4000)
    res = _run_asan(chains, tmp_path)
    n_ok = n_bad = 0
    for (rc, n, st, out), chain in zip(res, chains):
        assert rc == 0 and n == 3, (rc, n)
        members, _ = im.split_members(chain, decode=False)
        o = 0
        for m, s in zip(members, st):
            isize, = struct.unpack("<I", m[-4:])
            if s == 0:
                w = zlib.decompressobj(-15).decompress(im.payload_of(m))
                assert out[o:o + isize] == w and zlib.crc32(w) == struct.unpack("<I", m[-8:-4])[0]
                n_ok += 1
            else:
                assert s in (2, 3, 4, 5)
                assert out[o:o + isize] == b"\xa5" * isize
                n_bad += 1
            o += isize
    assert n_ok >= 8000 and n_bad >= 2000, (n_ok, n_bad)      # (two untouched members per chain; most mutations must be noticed)


def test_abi_edges(inflater, tmp_path):
    from bam_readcount_amd import capi
    assert inflater.kind() in ("sim", "hip-gfx950")
    good = im.member(b"hello, world" * 100, 6, zlib.Z_DEFAULT_STRATEGY)
    chain = good + im.member(b"second" * 50, 1, zlib.Z_DEFAULT_STRATEGY)
    # a short dst_cap: BRC_E_ARG, the sizes are still reported, nothing is written
    rc, out, off, st, n = inflater.inflate_raw(chain, dst_cap=1200)
    assert rc == capi.E_ARG and n == 2 and off.tolist() == [0, 1200, 1500] and out == b"\xa5" * 1200
    # a chain that does not end on a member boundary: BRC_E_ARG, the whole member in front is inflated
    rc, out, off, st, n = inflater.inflate_raw(chain[:-3])
    assert rc == capi.E_ARG and n == 1 and st.tolist() == [0] and out == b"hello, world" * 100
    rc, out, off, st, n = inflater.inflate_raw(chain + b"\x1f")
    assert rc == capi.E_ARG and n == 2 and st.tolist() == [0, 0]
    # a status array too small for the chain
    rc, out, off, st, n = inflater.inflate_raw(chain, dst_cap=1500, capacity=1)
    assert rc == capi.E_ARG and n == 2
    # no members at all
    rc, out, off, st, n = inflater.inflate_raw(b"")
    assert rc == 0 and n == 0 and out == b"" and off.tolist() == [0]
    # two inflaters alive at once
    other = capi.Inflater(inflater.path)
    a = inflater.inflate(chain); b = other.inflate(chain)
    assert a[0] == b[0] == b"hello, world" * 100 + b"second" * 50
    other.close()
    assert inflater.inflate(good)[0] == b"hello, world" * 100
    t = inflater.last_timing()
    assert t["bytes_out"] == 1200 and t["call_s"] >= t["kernel_s"] >= 0
