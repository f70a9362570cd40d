"""The host side the two codec libraries share (bam_readcount_amd/csrc/brc_codec_hip.h, tests/sim_codec.h), seen through
brc_inflate_bgzf and brc_deflate_bgzf: a caller's page-locked memory (brc_*_host_alloc) is copied from and to as it lies, pageable
memory goes through the handle's staging, and both must give the same bytes.  Every call here is made in all four combinations of
page-locked / pageable source x page-locked / pageable destination, on the GPU ([hip]) and on the CPU builds ([sim], where host_alloc
is malloc and the four are one path: the cases then check the test itself and the shared CPU handle).

The references: zlib (zlib.decompress(payload, -15) for the inflater, zlib's decoder over the deflater's members) and the CPU builds
(the statuses of a chain with broken members; the deflater's bytes).  Equality is byte for byte.  Destinations are pre-filled with 0xA5:
what a failed member's slot, and the bytes behind dst_len, must still hold afterwards.

What the test cannot see is whether a page-locked buffer was staged all the same: that costs time, not bytes."""
import ctypes as C
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools", "fuzz"))
import inflate_members as im  # noqa: E402

SIM_INFLATE_DIR = os.path.join(ROOT, "tests", "sim_inflate")
SIM_DEFLATE_DIR = os.path.join(ROOT, "tests", "sim_deflate")
M = 0xff00
FILL = 0xA5
# (source page-locked, destination page-locked)
MEMORY = [(False, False), (True, False), (False, True), (True, True)]


class Arena:
    """Buffers of one library for one test: page-locked ones from its host_alloc (freed by close()), pageable ones from numpy."""

    def __init__(self, handle, stem):
        self.alloc = getattr(handle.lib, stem + "_host_alloc"); self.free = getattr(handle.lib, stem + "_host_free")
        self.held = []

    def buf(self, n, pinned):
        if not pinned:
            return np.empty(max(n, 1), np.uint8)
        p = self.alloc(max(n, 1))
        assert p, "host_alloc(%d) failed" % n
        self.held.append(p)
        return np.frombuffer((C.c_uint8 * max(n, 1)).from_address(p), np.uint8)

    def close(self):
        while self.held:
            self.free(self.held.pop())


@pytest.fixture(scope="module", params=["sim", pytest.param("hip", marks=pytest.mark.gpu)])
def libs(request):
    """(the inflater class's path, the deflater class's path) under test and the CPU builds' paths: handles are made per test."""
    from bam_readcount_amd import capi
    subprocess.check_call(["make", "-s", "-C", SIM_INFLATE_DIR])
    subprocess.check_call(["make", "-s", "-C", SIM_DEFLATE_DIR])
    sim = dict(inflate=os.path.join(SIM_INFLATE_DIR, "libbrc_inflate_sim.so"), deflate=os.path.join(SIM_DEFLATE_DIR, "libbrc_deflate_sim.so"))
    under = sim if request.param == "sim" else dict(inflate=capi.INFLATE_LIB, deflate=capi.DEFLATE_LIB)
    kind = "sim" if request.param == "sim" else "hip-gfx950"
    return dict(under=under, sim=sim, kind=kind)


def _text(n, seed):
    """n bytes of lines over a skewed alphabet: compressible, but far from its member's bound"""
    rng = np.random.default_rng(seed)
    weight = np.array([8, 8, 8, 8, 2, 2, 2, 2, 2, 1] + [1] * 10 + [3, 1, 1, 1, 1, 1], float)
    return rng.choice(np.frombuffer(b"ACGTNacgtn0123456789\t\n:=+-", np.uint8), n, p=weight / weight.sum()).tobytes()


# ---------------------------------------------------------------- the inflater
def _inflate(inf, arena, chain, slots, src_pinned, dst_pinned, slack=64):
    """One brc_inflate_bgzf over `chain`, whose members inflate to `slots` bytes each: (rc, n, dst_off, statuses, all of dst)."""
    n, total = len(slots), sum(slots)
    src = arena.buf(len(chain), src_pinned); src[:len(chain)] = np.frombuffer(chain, np.uint8)
    dst = arena.buf(total + slack, dst_pinned); dst[:] = FILL
    off = np.zeros(n + 1, np.uint64); st = np.full(n, 0xEE, np.uint8); cnt = C.c_size_t(n)
    rc = inf.lib.brc_inflate_bgzf(inf.h, src.ctypes.data, len(chain), dst.ctypes.data, total + slack, off.ctypes.data, st.ctypes.data, C.byref(cnt))
    assert src[:len(chain)].tobytes() == chain, "the source was written to"
    return rc, cnt.value, off.tolist(), st.tolist(), dst.tobytes()


def _flip_crc(member):
    """one bit of the CRC32 of the trailer (CRC32, ISIZE)"""
    m = bytearray(member); m[-8] ^= 0x10
    return bytes(m)


def _four_members():
    payloads = [b"Q", _text(65280, 5), b"", _text(700, 6)]
    members = [im.member(payloads[0], 0), im.member(payloads[1], 6), im.EOF_MEMBER, im.member(payloads[3], 9)]
    assert im.payload_of(members[0])[0] & 7 == 1, "member 0 is not one final stored block"
    assert len(members[2]) == 28 and members[2][-4:] == bytes(4)
    assert im.payload_of(members[3])[0] & 7 == 5, "member 3 is not one final block of dynamic Huffman codes"
    # the reference: zlib on each payload
    assert [zlib.decompress(im.payload_of(m), -15) for m in members] == payloads
    return members, payloads


def _expect_slots(dst, off, payloads, failed):
    for i, p in enumerate(payloads):
        got = dst[off[i]:off[i + 1]]
        assert got == (bytes([FILL]) * len(p) if i in failed else p), "slot %d" % i
    assert dst[off[-1]:] == bytes([FILL]) * (len(dst) - off[-1]), "bytes behind the last slot"


@pytest.mark.parametrize("flipped", [(), (0,), (1,), (3,), (0, 1, 2, 3)], ids=lambda f: "flip" + "".join(map(str, f)) if f else "whole")
def test_inflate_from_and_to_either_memory(libs, flipped):
    """A stored 1-byte member, a full 65280-byte member, the end-of-file member and a small dynamic-Huffman member, whole and with the
    CRC32 of some of them broken: the same rc, offsets, statuses and bytes in all four kinds of memory; good members equal zlib's
    output; a failed member's slot keeps the caller's 0xA5 in a pageable and in a page-locked destination (the copy by runs)."""
    from bam_readcount_amd import capi
    members, payloads = _four_members()
    chain = b"".join(_flip_crc(m) if i in flipped else m for i, m in enumerate(members))
    slots = [len(p) for p in payloads]
    want_st = [capi.INF_CRC_MISMATCH if i in flipped else capi.INF_OK for i in range(4)]
    want_off = np.concatenate([[0], np.cumsum(slots)]).tolist()
    sim = capi.Inflater(libs["sim"]["inflate"])
    inf = capi.Inflater(libs["under"]["inflate"])
    assert inf.kind() == libs["kind"]
    arena, sim_arena = Arena(inf, "brc_inflate"), Arena(sim, "brc_inflate")
    try:
        ref = _inflate(sim, sim_arena, chain, slots, False, False)
        assert ref[:4] == (0, 4, want_off, want_st)
        _expect_slots(ref[4], want_off, payloads, flipped)
        for src_pinned, dst_pinned in MEMORY:
            got = _inflate(inf, arena, chain, slots, src_pinned, dst_pinned)
            assert got[:4] == ref[:4], (src_pinned, dst_pinned)
            _expect_slots(got[4], want_off, payloads, flipped)
            assert got[4] == ref[4], (src_pinned, dst_pinned)
    finally:
        arena.close(); sim_arena.close(); inf.close(); sim.close()


# ---------------------------------------------------------------- the deflater
def _deflate(d, arena, src_bytes, src_pinned, dst_pinned):
    """One brc_deflate_bgzf into a destination of exactly the bound: (rc, dst_len, members, all of dst)."""
    n = len(src_bytes)
    cap = d.bound(n)
    src = arena.buf(n, src_pinned); src[:n] = np.frombuffer(src_bytes, np.uint8)
    dst = arena.buf(cap, dst_pinned); dst[:] = FILL
    got = C.c_size_t(12345); nm = C.c_size_t(12345)
    rc = d.lib.brc_deflate_bgzf(d.h, src.ctypes.data, n, dst.ctypes.data, cap, C.byref(got), C.byref(nm))
    assert src[:n].tobytes() == src_bytes, "the source was written to"
    return rc, got.value, nm.value, dst.tobytes()


def _check_deflated(res, src_bytes, ref_bytes):
    rc, dst_len, members, dst = res
    assert rc == 0 and members == (len(src_bytes) + M - 1) // M
    assert dst[:dst_len] == ref_bytes
    assert dst[dst_len:] == bytes([FILL]) * (len(dst) - dst_len), "bytes behind dst_len"
    # the reference: zlib's decoder over every member
    parts, payloads = im.split_members(dst[:dst_len])
    assert len(parts) == members and b"".join(payloads) == src_bytes


@pytest.mark.parametrize("size", [0, 1, M, M + 1, 3 * M + 17])
def test_deflate_from_and_to_either_memory(libs, size):
    """No byte, one byte, a full member, a full member and one byte, three full members and a few: the same bytes, dst_len and member
    count in all four kinds of memory, equal to the CPU build's; zlib inflates them to the input; nothing behind dst_len is touched."""
    from bam_readcount_amd import capi
    src = _text(3 * M + 17, 7)[:size]
    sim = capi.Deflater(libs["sim"]["deflate"])
    d = capi.Deflater(libs["under"]["deflate"])
    assert d.kind() == libs["kind"]
    arena, sim_arena = Arena(d, "brc_deflate"), Arena(sim, "brc_deflate")
    try:
        ref = _deflate(sim, sim_arena, src, False, False)
        _check_deflated(ref, src, ref[3][:ref[1]])
        for src_pinned, dst_pinned in MEMORY:
            got = _deflate(d, arena, src, src_pinned, dst_pinned)
            _check_deflated(got, src, ref[3][:ref[1]])
            assert got == ref, (src_pinned, dst_pinned)
    finally:
        arena.close(); sim_arena.close(); d.close(); sim.close()


# ---------------------------------------------------------------- growth of one handle's buffers; two handles
def _small_and_large():
    """100 bytes, then three full members: far more than a buffer sized for the first (want + want / 4 + 4096) holds."""
    small, large = _text(100, 8), _text(3 * M, 9)
    chains = []
    for data in (small, large):
        members = [im.member(data[o:o + M], 6) for o in range(0, len(data), M)]
        chains.append((b"".join(members), [min(M, len(data) - o) for o in range(0, len(data), M)], data))
    assert len(chains[1][0]) > (len(chains[0][0]) + 16) * 5 // 4 + 4096 and len(large) > (100 + 16) * 5 // 4 + 4096
    return small, large, chains


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "page-locked"])
def test_buffers_grow_and_are_reused(libs, pinned):
    """small, large, small on ONE handle of each library: the second call outgrows every buffer of the first (device buffers, and with
    pageable memory the staging too), the third fits what the second left.  Each call is right; the third equals the first."""
    from bam_readcount_amd import capi
    small, large, chains = _small_and_large()
    inf = capi.Inflater(libs["under"]["inflate"]); d = capi.Deflater(libs["under"]["deflate"]); sim = capi.Deflater(libs["sim"]["deflate"])
    ia, da, sa = Arena(inf, "brc_inflate"), Arena(d, "brc_deflate"), Arena(sim, "brc_deflate")
    try:
        got = []
        for chain, slots, data in (chains[0], chains[1], chains[0]):
            rc, n, off, st, dst = _inflate(inf, ia, chain, slots, pinned, pinned)
            assert (rc, n, st) == (0, len(slots), [0] * len(slots)) and off == np.concatenate([[0], np.cumsum(slots)]).tolist()
            assert dst[:len(data)] == data and dst[len(data):] == bytes([FILL]) * 64
            got.append((off, dst))
        assert got[2] == got[0]
        got = []
        for data in (small, large, small):
            ref = _deflate(sim, sa, data, False, False)
            res = _deflate(d, da, data, pinned, pinned)
            _check_deflated(res, data, ref[3][:ref[1]])
            got.append(res)
        assert got[2] == got[0]
    finally:
        ia.close(); da.close(); sa.close(); inf.close(); d.close(); sim.close()


def test_two_handles_of_one_library(libs):
    """Two inflaters and two deflaters alive at once, used in turn on two inputs: every handle gives the bytes the other gives, and the
    bytes zlib / the first call gave."""
    from bam_readcount_amd import capi
    small, large, chains = _small_and_large()
    infs = [capi.Inflater(libs["under"]["inflate"]) for _ in range(2)]
    defs = [capi.Deflater(libs["under"]["deflate"]) for _ in range(2)]
    arenas = [Arena(infs[0], "brc_inflate"), Arena(defs[0], "brc_deflate")]
    try:
        first = {}
        for turn in range(4):
            h, which = infs[turn % 2], (turn // 2 + turn) % 2          # (handle 0: small, handle 1: large, then the other way round)
            chain, slots, data = chains[which]
            rc, n, off, st, dst = _inflate(h, arenas[0], chain, slots, turn % 2 == 0, turn % 2 == 1)
            assert (rc, n, st) == (0, len(slots), [0] * len(slots)) and dst[:len(data)] == data
            assert first.setdefault(("inf", which), (off, dst)) == (off, dst)
            res = _deflate(defs[turn % 2], arenas[1], data, turn % 2 == 1, turn % 2 == 0)
            assert res[0] == 0 and b"".join(im.split_members(res[3][:res[1]])[1]) == data
            assert first.setdefault(("def", which), res) == res
        assert len(first) == 4
    finally:
        for a in arenas:
            a.close()
        for h in infs + defs:
            h.close()
