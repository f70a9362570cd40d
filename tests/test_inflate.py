"""The BGZF inflater (include/brc_inflate.h): the decoder of bam_readcount_amd/csrc/brc_inflate_core.h behind its C-ABI, on the GPU
([hip]: libbrc_inflate_hip.so) and lane for lane on the CPU ([sim]: tests/sim_inflate).  The reference is zlib itself
(zlib.decompress(payload, -15), zlib.crc32); equality is byte for byte.

The malformed members are a fixed list, each with the status the FORMAT demands (RFC 1951 / RFC 1952 / SAMv1 4.1; the reasoning
stands next to each case).  They are error paths of a total decoder: the list first runs on the CPU build under the host sanitizers
(every step outside a member's payload or slot would be a report), then on the plain CPU build, then — the identical list, once — on
the GPU.  The random-corruption fuzz runs under the sanitizers only."""
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
    assert len(cases) >= 13
    for case, (rc, n, st, out) in zip(cases, _run_asan([c.chain for c in cases], tmp_path)):
        _check_case(case, rc, n, st, out)


def test_malformed_members(inflater):
    """The fixed list, each case with its expected status; the good members of the same call come out right; a failed member leaves its
    slot untouched.  ([hip] runs it once, after the sanitizer build and the CPU build have passed the same list.)"""
    for case in im.malformed_cases():
        rc, out, off, st, n = inflater.inflate_raw(case.chain)
        _check_case(case, rc, n, st, out)


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
