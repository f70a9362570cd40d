"""Device-side window summaries (include/brc_bins.h): brc_bins_reduce and bam_readcount_amd.tensors.bins against the header's definitions
written in numpy over the ORACLE's dense brc_result (depth, ncol, istat[..][BRC_I_N], refbase) and its indel list — uint64 sums, every
output equal exactly, no tolerance.

Every body runs twice (the `route` fixture): [sim] = libbrc_sim.so + tests/sim_bins/libbrc_bins_sim.so, host memory, in the CPU suite;
[hip] = the product's libraries on the GPU (gpu-marked), edge lists, status word and destinations in device memory allocated through
torch.  Destinations are filled with 0xA5 bytes first and are PAD elements wider than n_bins: the padding, and every destination that
was not asked for, must keep them.  The host sanitizers run the CPU build over the hand-built and the window cases.

Where no engine can produce the shape — depths of 2^31, 254 libraries, reference characters of every kind — the two views are built by
hand (test_select.build_views) from dense counts, in the route's memory, and the reference is the same numpy over those dense counts.

Sizes that matter to the kernels (brc_bins.hip): a wave is 64 consecutive positions and reduces across its lanes when they share one bin,
a workgroup is 256 positions, the histogram lives in LDS per workgroup."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from bam_readcount_amd import capi
import abi_side as side
from route import Route, SENT
import test_dense as td
import test_select as ts

SENT64 = np.uint64(0xA5A5A5A5A5A5A5A5)
LIBS = ("dense", "select", "bins")
PAD = 3                                   # elements of every row behind n_bins
NSUM = capi.BINS_NSUM
PER_LIB = ts.PER_LIB
ALL = ("sums", "covered", "hist", "status")
THR = (0, 1, 4, 10, 20, 30)


@pytest.fixture(scope="module", params=["sim", pytest.param("hip", marks=pytest.mark.gpu)])
def route(request):
    return Route(request.param, LIBS, engine=True)


@pytest.fixture(scope="module")
def sim_route():
    return Route("sim", LIBS, engine=True)


# ------------------------------------------------------------------------------------------------ the reference

class Dense:
    """what the reference reads, from an oracle result or from hand-made arrays: depth, ncol [L, P], cnt [L, 6, P] (the read counts of
    "=ACGTN"), refbase: P characters, indels: (pos, lib, len, count)"""

    def __init__(self, depth, ncol, cnt, refbase, indels, pos0):
        self.depth, self.ncol, self.cnt, self.refbase, self.indels, self.pos0 = depth, ncol, cnt, bytes(refbase), list(indels), pos0
        self.n_lib, self.n_pos = depth.shape

    @classmethod
    def of(cls, res):
        return cls(res.depth, res.ncol, res.istat[:, :, 0, :], res.refbase, [(d["pos"], d["lib"], d["len"], int(d["i"][0])) for d in res.indels], res.pos0)

    @classmethod
    def of_hand(cls, h):
        """a test_select.Dense of build_views: cnt [L, 4, P], the ncol plane a copy of depth"""
        cnt = np.zeros((h.n_lib, 6, h.n_pos), np.uint32); cnt[:, 1:5] = h.cnt
        return cls(np.asarray(h.depth, np.uint32), np.asarray(h.depth, np.uint32), cnt, h.refbase, h.indels, h.pos0)


def bin_index(k0, n, width=0, edges=None):
    """(bin of every window position or -1, n_bins), by the header's words: the number of edges[1..n_bins] that are <= k"""
    k = np.arange(k0, k0 + n, dtype=np.int64)
    if edges is None:
        return (k - k0) // width, (n + width - 1) // width
    e = np.asarray(edges, np.int64)
    nb = e.size - 1
    if nb == 0:
        return np.full(n, -1, np.int64), 0
    b = (e[1:, None] <= k[None, :]).sum(axis=0) if nb * max(n, 1) <= 4_000_000 else np.searchsorted(e[1:], k, side="right")
    return np.where((e[0] <= k) & (k < e[nb]), b, -1), nb


def reference(D, k0, n, width=0, edges=None, thr=(), n_hist=0):
    """{"sums" [L, 12, n_bins], "covered" [L, n_thr, n_bins], "hist" [L, n_hist]} in uint64"""
    u = np.uint64
    b, nb = bin_index(k0, n, width, edges)
    ok = b >= 0
    bo = b[ok]
    L = D.n_lib
    depth = D.depth[:, k0:k0 + n].astype(u); cnt = D.cnt[:, :, k0:k0 + n].astype(u)
    rb = ts._REFCODE[np.frombuffer(D.refbase, np.uint8)[k0:k0 + n]]
    nonref = np.zeros((L, n), u)
    for c in range(4):
        nonref += cnt[:, 1 + c] * ((rb >= 0) & (rb != c)).astype(u)
    vals = np.concatenate([depth[:, None], D.ncol[:, None, k0:k0 + n].astype(u), cnt, nonref[:, None]], axis=1)          # [L, 9, n]
    sums = np.zeros((L, NSUM, nb), u)
    if nb:
        np.add.at(sums, (slice(None), slice(0, 9), bo), vals[:, :, ok])
        np.maximum.at(sums, (slice(None), 11, bo), depth[:, ok])
        for pos, lib, ln, count in D.indels:
            j = pos - D.pos0 - k0
            if ln != 0 and 0 <= j < n and b[j] >= 0:
                sums[lib, 9 if ln > 0 else 10, b[j]] += u(count)
    cov = np.zeros((L, len(thr), nb), u)
    for t, x in enumerate(thr):
        if nb:
            np.add.at(cov, (slice(None), t, bo), (depth[:, ok] >= u(x)).astype(u))
    hist = np.zeros((L, n_hist), u)
    for l in range(L):
        if n_hist:
            hist[l] = np.bincount(np.minimum(depth[l, ok], u(n_hist - 1)).astype(np.int64), minlength=n_hist).astype(u)
    return {"sums": sums, "covered": cov, "hist": hist}


# ------------------------------------------------------------------------------------------------ calling the library

def count_bins(n, width, edges):
    return len(edges) - 1 if edges is not None else ((n + width - 1) // width if width > 0 and n > 0 else 0)


def call(route, v, d, k0, n, width=0, edges=None, thr=(), n_hist=0, ds=None, want=ALL, handle=True, params=True, fields=None):
    """brc_bins_reduce into 0xA5-filled destinations of [.][n_bins + PAD] (or [.][ds]); edges go into the route's memory.
    fields: members of brc_bins_params set afterwards (for the refusals).  Returns (rc, status word, sums [L, 12, ds], covered
    [L, n_thr, ds], hist [L, n_hist])"""
    L = int(v.n_lib) if v is not None and v.n_lib > 0 else 1
    nb = count_bins(n, width, edges)
    ds = nb + PAD if ds is None else ds
    nt, nh, dd = min(len(thr), 8), min(max(n_hist, 0), 4096), max(ds, 0)
    bs, bc, bh, bt = route.sentinel_words(max(2 * (L + 1) * NSUM * dd, 2)), route.sentinel_words(max(2 * L * nt * dd, 2)), route.sentinel_words(max(2 * L * nh, 2)), route.sentinel_words(1)
    be = route.put(np.asarray(edges, np.int32)) if edges is not None else None
    par = capi.bins_params(width, route.ptr(be) if be is not None else None, nb if edges is not None else 0, list(thr), n_hist)
    for k, x in (fields or {}).items():
        setattr(par, k, x)
    rc = route.bins.lib.brc_bins_reduce(route.bins.h if handle else None, C.byref(v) if v is not None else None, C.byref(d) if d is not None else None,
                                        C.byref(par) if params else None, k0, n, route.ptr(bs) if "sums" in want else None,
                                        route.ptr(bc) if "covered" in want else None, route.ptr(bh) if "hist" in want else None, ds,
                                        route.ptr(bt) if "status" in want else None, None)
    assert (route.quads(bs)[L * NSUM * dd:] == SENT64).all(), "sums of a library behind the last one were written"      # (room for one library more)
    return (rc, int(route.words(bt)[0]), route.quads(bs)[:L * NSUM * dd].reshape(L, NSUM, dd).copy(), route.quads(bc)[:L * nt * dd].reshape(L, nt, dd).copy(),
            route.quads(bh)[:L * nh].reshape(L, nh).copy())


def untouched(*arrays):
    return all((a == SENT64).all() for a in arrays)


def check(route, v, d, D, k0=0, n=None, width=0, edges=None, thr=THR, n_hist=16, what="", status=0):
    n = D.n_pos - k0 if n is None else n
    w = reference(D, k0, n, width, edges, thr, n_hist)
    nb = w["sums"].shape[2]
    rc, st, gs, gc, gh = call(route, v, d, k0, n, width, edges, thr, n_hist)
    assert rc == 0, (what, route.bins.lib.brc_bins_last_error(route.bins.h))
    assert st == status, (what, st)
    assert np.array_equal(gs[:, :, :nb], w["sums"]), "%s: sums differ at %r" % (what, np.argwhere(gs[:, :, :nb] != w["sums"])[:6].tolist())
    assert np.array_equal(gc[:, :, :nb], w["covered"]), "%s: covered differs at %r" % (what, np.argwhere(gc[:, :, :nb] != w["covered"])[:6].tolist())
    assert np.array_equal(gh, w["hist"]), "%s: hist differs" % what
    assert untouched(gs[:, :, nb:], gc[:, :, nb:]), "%s: wrote into the padding" % what
    return w


def hand(route, *a, **kw):
    v, d, h, keep = ts.build_views(route, *a, **kw)
    return v, d, Dense.of_hand(h), keep


# ------------------------------------------------------------------------------------------------ 1. the golden fixtures

def test_golden_fixtures_at_five_widths(route, oracle_lib, test_bam, twolib):
    beg0, end = 10402736, 10405248
    res, _ = td.oracle_result(oracle_lib, test_bam, beg0, end, test_bam["ref"], tid=20)
    eng = td.computed(route.engine_lib, test_bam, beg0, end, test_bam["ref"], tid=20)
    v, d = ts.views_of(eng)
    D = Dense.of(res)
    for width in (1, 7, 64, 100, res.n_pos):
        w = check(route, v, d, D, width=width, n_hist=64, what="test_bam width %d" % width)
        s = w["sums"]
        assert s[:, 0].any() and s[:, 8].any() and (s[:, 9].any() or s[:, 10].any()), "the fixture leaves a sum of the table at zero"
    eng.close()
    names = [str(s) for s in twolib["lib_names"]]
    opts = dict(lib_names=names, per_lib=True, insertion_centric=True, ref_len_check=True)
    end = int(twolib["ref"].size)
    res, _ = td.oracle_result(oracle_lib, twolib, 0, end, twolib["ref"], **opts)
    assert res.n_lib == 2
    eng = td.computed(route.engine_lib, twolib, 0, end, twolib["ref"], **opts)
    v, d = ts.views_of(eng)
    for width in (1, 7, 64, 100, res.n_pos):
        check(route, v, d, Dense.of(res), width=width, thr=(0, 1, 2), n_hist=4, what="twolib width %d" % width)
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. windows off the grid

LOW_INDELS = [(0, 0, 2, 3), (63, 1, -1, 2), (64, 0, -3, 1), (255, 1, 4, 5), (256, 0, 1, 1), (700, 1, -2, 7), (1499, 0, 5, 2), (1499, 1, -1, 1)]


def low_views(route):
    depth, cnt, ref = ts.low_depth(1500, seed=4)
    return hand(route, depth, cnt, ref, indels=LOW_INDELS)


def window_calls(P):
    """(k0, n, width, edges): windows off the 64-grid and n of 1, 63 / 64 / 65 and 257, uniform bins and an edge list inside each"""
    out = []
    for i, (k0, n) in enumerate(ts.window_list(P)):
        for width in ((1, 7, 64, 100, n)[i % 5], (64, 100, n, 1, 7)[i % 5]):
            out.append((k0, n, width, None))
        cut = sorted({k0, k0 + n // 3, k0 + n // 3, k0 + (2 * n) // 3, k0 + n - (n > 2)})
        out.append((k0, n, 0, cut))
    return out


def test_windows_off_the_grid(route):
    v, d, D, keep = low_views(route)
    assert D.n_lib == 2 and (D.cnt.sum(axis=1) > 0).any()
    for k0, n, width, edges in window_calls(D.n_pos):
        check(route, v, d, D, k0, n, width, edges, what="window %r width %r edges %r" % ((k0, n), width, edges))


# ------------------------------------------------------------------------------------------------ 3. bin edges against the kernel's grain

def grain_lists(k0, n):
    e = k0 + n
    return {"64 bins of width 1 inside one wave": list(range(k0 + 64, k0 + 129)),
            "cuts at lanes 63 | 64 and 255 | 256": [k0, k0 + 64, k0 + 256, e],
            "a bin of 600 positions over workgroups": [k0 + 100, k0 + 700, k0 + 701],
            "empty bins at the front, in the middle and at the end": [k0, k0, k0, k0 + 300, k0 + 300, k0 + 300, k0 + 900, e, e, e],
            "edges equal to k0 and k0 + n": [k0, e],
            "n_bins 0": [k0 + 5],
            "n_bins 1": [k0 + 70, k0 + 71],
            "n_bins 257": [k0 + 3 * i for i in range(258)],
            "everything behind the last edge": [k0, k0 + 1]}


def test_bin_edges_against_the_grain(route):
    v, d, D, keep = low_views(route)
    for k0, n in ((0, D.n_pos), (37, 1301)):
        for what, edges in grain_lists(k0, n).items():
            w = check(route, v, d, D, k0, n, 0, edges, what="%s (window %r)" % (what, (k0, n)))
            if what.startswith("empty"):
                assert not w["sums"][:, :, [0, 1, 3, 4, 7, 8]].any() and w["sums"][:, 0, 2].all() and w["sums"][:, 0, 6].all()
    # uniform bins of 64 positions from a window that starts off the grid: every wave holds an edge
    check(route, v, d, D, 37, 1301, 64, what="width 64 from k0 = 37")
    check(route, v, d, D, 64, 1280, 64, what="width 64 from k0 = 64")
    check(route, v, d, D, 0, 1500, 10 ** 12, what="a width beyond the window")


# ------------------------------------------------------------------------------------------------ 4. third alleles

def test_third_allele_counts_sit_in_records_only(route, oracle_lib, monkeypatch):
    """The knob libraries under BRC_FORCE_DOM=3 + BRC_XEV_CAP=1 (as test_select sets them): bins whose bucket sums and non-reference
    sums are right only with the records applied — the slots alone, summed by the same reference, give another number"""
    monkeypatch.setenv("BRC_FORCE_DOM", "3"); monkeypatch.setenv("BRC_XEV_CAP", "1")
    ref, arrs = td.third_allele_inputs()
    opts = dict(PER_LIB, min_bq=10)
    res, _ = td.oracle_result(oracle_lib, arrs, 0, 2000, ref, **opts)
    eng = td.computed(route.knob_lib, arrs, 0, 2000, ref, **opts)
    v, d = ts.views_of(eng)
    assert v.n_xagg > 0
    D = Dense.of(res)
    bare = capi.DeviceView.from_buffer_copy(v); bare.n_xagg = 0
    rc, slots = td.expand(route, bare, 0, res.n_pos, res.n_pos, kinds=("istat",))
    assert rc == 0
    S = Dense(D.depth, D.ncol, slots["istat"].reshape(2, 6, 9, res.n_pos)[:, :, 0, :], D.refbase, D.indels, D.pos0)
    for width, edges in ((1, None), (64, None), (100, None), (res.n_pos, None), (0, [5, 130, 131, 900, 1990])):
        w = check(route, v, d, D, width=width, edges=edges, what="third alleles width %r" % width)
        s = reference(S, 0, res.n_pos, width, edges)
        assert (w["sums"][:, 2:8] != s["sums"][:, 2:8]).any() and (w["sums"][:, 8] != s["sums"][:, 8]).any(), "the slots alone give the same sums"
    check(route, v, d, D, 333, 1111, 64, what="third alleles, a window")
    eng.close()


# ------------------------------------------------------------------------------------------------ 5. hand-built views

def big_depth_views(route):
    """depths of 2^31 at three positions of one bin (their sum passes 2^32), depths around the thresholds 5 and 2^31"""
    P = 200
    depth = np.full((2, P), 4, np.uint32); depth[0, 1::2] = 5; depth[1, ::3] = 6
    depth[0, [70, 100, 127]] = 2 ** 31; depth[1, 71] = 2 ** 31 - 1; depth[1, 72] = 2 ** 32 - 1
    cnt = np.zeros((2, 4, P), np.uint32); cnt[:, 0] = depth
    return hand(route, depth, cnt, b"A" * P, indels=[(64, 0, 3, 2 ** 32 - 1), (64, 0, 2, 9), (127, 0, -1, 4), (127, 1, -2, 2 ** 31), (128, 1, 1, 1)])


BIG_THR = (0, 4, 5, 6, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1)
BIG_CALLS = [dict(width=64, n_hist=1), dict(width=64, n_hist=2), dict(width=64, n_hist=4096), dict(edges=[64, 128], n_hist=6), dict(width=200, n_hist=7)]


def test_sums_beyond_32_bits_thresholds_and_clamps(route):
    v, d, D, keep = big_depth_views(route)
    for kw in BIG_CALLS:
        w = check(route, v, d, D, thr=BIG_THR, what=repr(kw), **kw)
        if kw.get("width") == 64:
            assert w["sums"][0, 0, 1] > 2 ** 32 and w["sums"][0, 11, 1] == 2 ** 31 and w["sums"][0, 9, 1] == 2 ** 32 + 8
            # thresholds met exactly and missed by one, threshold 0
            assert w["covered"][0, :, 1].tolist() == [64, 64, 3 + 31, 3, 3, 3, 0] and w["covered"][1, 4:, 1].tolist() == [2, 1, 1]
    h = reference(D, 0, D.n_pos, 64, None, (), 6)["hist"]
    assert h[0, 4] and h[0, 5] > 3 and h[1, 5] > 0                     # a depth below, at and above the clamp of six bars


def test_reference_characters_and_no_reference(route):
    """acgt, N, IUPAC codes and NUL; no reference at all; slices that start late, end early or pass ref_len: sum 8 counts the other
    bases only where the reference character is one of ACGTacgt"""
    for what, (v, d, h, keep), _ in ts.refchar_views(route):
        D = Dense.of_hand(h)
        for width in (1, 4, 64, D.n_pos):
            w = check(route, v, d, D, width=width, what="%s width %d" % (what, width))
        if what == "characters":
            one = reference(D, 0, D.n_pos, 4)["sums"][0, 8]
            assert one[:8].tolist() == [12] * 8 and not one[8:].any()          # four positions per character, three of them not its base
        if what == "no reference":
            assert not d.ref and not w["sums"][:, 8].any() and w["sums"][0, 9].any()


def test_indel_records_at_bin_borders_and_in_libraries_without_reads(route):
    P = 300
    depth = np.zeros((3, P), np.uint32); depth[0] = 7
    cnt = np.zeros((3, 4, P), np.uint32); cnt[0, 2] = 7
    ind = [(100, 0, 2, 3), (199, 0, -2, 4), (200, 0, 1, 5), (99, 0, -1, 6),       # the first and the last position of bin [100, 200)
           (100, 2, 5, 1), (199, 2, -7, 2), (150, 1, 1, 9), (299, 2, 3, 1), (0, 1, -1, 1)]     # libraries 1 and 2 have no reads
    v, d, D, keep = hand(route, depth, cnt, b"G" * P, indels=ind)
    w = check(route, v, d, D, edges=[100, 200], what="one bin")
    assert w["sums"][:, 9, 0].tolist() == [3, 9, 1] and w["sums"][:, 10, 0].tolist() == [4, 0, 2]
    check(route, v, d, D, width=100, what="width 100")
    check(route, v, d, D, 1, 298, width=1, what="width 1")
    # a view without indel records and without third-allele records
    v, d, D, keep = hand(route, depth, cnt, b"G" * P)
    assert d.n_slots == 0 and v.n_xagg == 0
    check(route, v, d, D, width=100, what="no records")


def lib254_views(route):
    depth, cnt, ref = ts.low_depth(70, L=254, seed=3, alt=0.02)
    return hand(route, depth, cnt, ref, indels=[(7, 253, -2, 3), (7, 1, -1, 1), (9, 252, 4, 2)])


def test_254_libraries(route):
    v, d, D, keep = lib254_views(route)
    assert v.n_lib == 254 and v.n_xagg > 0
    check(route, v, d, D, width=7, what="254 libraries, width 7")
    check(route, v, d, D, 3, 65, edges=[3, 10, 10, 67, 68], what="254 libraries, edges")


def test_an_edge_one_behind_a_window_of_more_than_100000_positions(route):
    """BRC_BINS_OUTSIDE for an edge at k0 + n + 1, and none for an edge at k0 + n, when the window has 100 001 positions"""
    Pn = 100002
    depth = (np.arange(Pn) % 11).astype(np.uint32)[None, :]
    cnt = np.zeros((1, 4, Pn), np.uint32); cnt[0, 0] = depth[0]
    v, d, D, keep = hand(route, depth, cnt, b"A" * Pn)
    n = Pn - 1
    check(route, v, d, D, 0, n, edges=[0, 50000, n], what="edges up to k0 + n", n_hist=4)
    check(route, v, d, D, 0, n, edges=[0, 50000, n + 1], what="an edge at k0 + n + 1", n_hist=4, status=capi.BINS_OUTSIDE)
    check(route, v, d, D, 1, n, edges=[0, 50000, n + 1], what="an edge at k0 - 1", n_hist=4, status=capi.BINS_OUTSIDE)


def test_uniform_bins_behind_window_element_2_to_the_24(route):
    """a window of 2^24 + 5 positions in bins of 2^23: the last five positions are bin 2 (an element index that passes 2^24 has no
    exact fp32 form).  covered and hist alone read the depth plane alone, so the view's other planes are the depth plane again: 64 MiB."""
    Pn = 2 ** 24 + 5
    PS = Pn + 59
    depth = (np.arange(PS, dtype=np.uint32) % 7).astype(np.uint32)
    buf = route.put(depth)
    p = route.ptr(buf)
    v = capi.DeviceView(route.mem, 0, 1, 0, Pn, PS, p, p, p, p, None, p, None, 0)
    d = capi.DeviceIndels(route.mem, 0, 1, 0, Pn, None, 0)
    rc, st, gs, gc, gh = call(route, v, d, 0, Pn, 2 ** 23, thr=(0, 3), n_hist=5, want=("covered", "hist", "status"))
    assert rc == 0 and st == 0 and untouched(gs)
    dd = depth[:Pn]
    cuts = [0, 2 ** 23, 2 ** 24, Pn]
    want = np.array([[int((dd[a:b] >= t).sum()) for a, b in zip(cuts, cuts[1:])] for t in (0, 3)], np.uint64)
    assert want[0].tolist() == [2 ** 23, 2 ** 23, 5]
    assert np.array_equal(gc[0, :, :3], want) and untouched(gc[:, :, 3:])
    assert np.array_equal(gh[0], np.bincount(np.minimum(dd, 4), minlength=5).astype(np.uint64))


def test_reads_in_the_buckets_that_are_no_base(route):
    """reads in bucket 0 ('=') and bucket 5 (N), in slots and in third-allele records, at positions whose reference is A, C, G or T and
    at positions whose reference is N (test_select.raw_views: the compact form written down).  S_NONREF counts buckets 1 .. 4 only —
    shown on the reference's side against a sum that takes bucket 5, or bucket 0, along — and the buckets' own sums count them all.
    Records of libraries n_lib, n_lib + 1 and -1 lie beside valid ones of the same position and add nothing."""
    import handmade_views as hv
    L, Pn = 2, 140
    k = np.arange(Pn)
    ref = bytes(b"ACGTN"[x] for x in k % 5)
    kind = (k // 5) % 4                                     # slots name (ref's, 5), (5, an alternate), (0, ref's), (an alternate, 0)
    rb = np.where(k % 5 < 4, k % 5 + 1, 1); other = rb % 4 + 1
    b0 = np.choose(kind, [rb, 5, 0, other]); b1 = np.choose(kind, [5, other, rb, 0])
    b0[120:130] |= 0x80; b1[130:] |= 0x80                     # bytes 0x80 .. 0x85 name no bucket: those slots' reads count nowhere
    slotid = np.broadcast_to((b0 | (b1 << 8)).astype(np.uint32), (L, Pn)).copy()
    si = np.zeros((L, 2, 9, Pn), np.uint32)
    si[0, 0, 0] = 10 + k % 7; si[0, 1, 0] = 3 + k % 4; si[1, 0, 0] = 2 + k % 3; si[1, 1, 0] = 20 + k % 5
    recs = []
    for x in range(0, Pn, 3):                                # a third-allele record of bucket 5 or 0 where no slot names it, every third position
        b = 0 if b0[x] == 5 or b1[x] == 5 else 5
        recs.append(hv.record(x, x % L, b, [40 + x % 9] * 9, [0] * 4))
        if x % 2:
            recs.append(hv.record(x, x % L, 5 - b, [60 + x % 4] * 9, [0] * 4))      # ... and one that takes a slot's place
    for x in (7, 63, 64):
        for bad in (L, L + 1, -1):
            recs += [hv.record(x, bad, 5, [1000] * 9, [0] * 4), hv.record(x, bad, 2, [1000] * 9, [0] * 4)]
        recs += [hv.record(x, 0, 6, [1000] * 9, [0] * 4), hv.record(x, 1, 0xFF, [1000] * 9, [0] * 4)]      # buckets that do not exist
        recs += [hv.record(x, 0, 0x83, [1000] * 9, [0] * 4), hv.record(x, 1, 0x80, [1000] * 9, [0] * 4)]
    good = [(7, 0, 2, 3), (63, 1, -1, 4), (64, 0, -2, 5)]
    ind = good + [(x, bad, ln, 1000) for x in (7, 63, 64) for bad in (L, L + 1, -1) for ln in (3, -3)]
    depth = np.full((L, Pn), 90, np.uint32)
    v, d, istat, _, refbase, keep = ts.raw_views(route, depth, slotid, si, records=recs[::-1], indels=ind[::-1], ref=ref)
    D = Dense(depth, depth, istat[:, :, 0, :], refbase, good, 0)
    assert D.cnt[:, 0].any() and D.cnt[:, 5].any() and D.cnt[:, 5, k % 5 < 4].any() and D.cnt[:, 5, k % 5 == 4].any() and D.cnt.max() < 1000
    for kw in (dict(width=1), dict(width=5), dict(width=64), dict(k0=3, n=130, edges=[3, 60, 64, 65, 133])):
        w = check(route, v, d, D, what="buckets 0 and 5, %r" % (kw,), **kw)
    w = reference(D, 0, Pn, width=Pn)["sums"][:, :, 0]
    acgt = (k % 5 < 4)
    for l in range(L):
        own = D.cnt[l, 1:5][ts._REFCODE[np.frombuffer(refbase, np.uint8)], k].astype(np.uint64)[acgt].sum()
        assert w[l, 8] == D.cnt[l, 1:5, acgt.nonzero()[0]].sum() - own
        assert w[l, 8] + D.cnt[l, 5, acgt].sum() != w[l, 8] != w[l, 8] + D.cnt[l, 0, acgt].sum()
        assert w[l, 2] == D.cnt[l, 0].sum() and w[l, 7] == D.cnt[l, 5].sum()


# ------------------------------------------------------------------------------------------------ 6. a site-list axis

def test_site_list_axis_counts_empty_positions_as_depth_zero(route, oracle_lib, low_region):
    ref, arrs, res = low_region
    wins = [(300, 301), (640, 710), (1500, 1501), (2000, 2064)]
    b = np.array([w[0] for w in wins], np.int32); e = np.array([w[1] for w in wins], np.int32)
    eng = capi.Engine(route.engine_lib, **PER_LIB)
    eng.begin_region(0, 50, 2950, ref)
    eng.push_reads(capi.select_reads(arrs, capi.fetch_overlapping(arrs, capi.read_ends(arrs), 49, 2950)))
    eng.region_windows(b, e)
    eng.upload(); eng.compute()
    v, d = ts.views_of(eng)
    full = Dense.of(res)
    # include/brc.h, brc_region_windows: per 64-position tile the engine piles up from the first to the last position that a window
    # [vbeg0 - 1, vend) asks for; everything else is EMPTY
    asked = np.zeros(res.n_pos, bool)
    for x, y in wins:
        asked[x - 1 - res.pos0:y - res.pos0] = True
    announced = np.zeros(res.n_pos, bool)
    for t in range(0, res.n_pos, 64):
        k = np.nonzero(asked[t:t + 64])[0]
        if k.size:
            announced[t + k[0]:t + k[-1] + 1] = True
    assert asked.sum() <= announced.sum() < res.n_pos // 2
    D = Dense(full.depth * announced, full.ncol * announced, full.cnt * announced, full.refbase,
              [r for r in full.indels if announced[r[0] - res.pos0]], full.pos0)
    assert D.depth[:, asked].any()
    edges = [p - res.pos0 for w in wins for p in w]                                    # one bin per line, the gaps between them as bins too
    w = check(route, v, d, D, edges=edges, thr=(0, 1), n_hist=8, what="one bin per line")
    assert w["covered"][0, 0].tolist() == [1, 339, 70, 790, 1, 499, 64]               # threshold 0 counts the EMPTY positions too
    assert w["hist"][0, 0] >= 1764 - announced.sum() and w["covered"][0, 1, 3] < 64
    check(route, v, d, D, width=64, thr=(0, 1), n_hist=8, what="uniform bins over a site list")
    eng.close()


@pytest.fixture(scope="module")
def low_region(oracle_lib):
    import synth
    rng = np.random.default_rng(11)
    ref = synth.make_ref(rng, 3000, weird=0.01)
    arrs = synth.make_batch(77, ref, 260, read_len=(60, 120), style="indel", n_libs=2, mismatch=0.06)
    res, _ = td.oracle_result(oracle_lib, arrs, 50, 2950, ref, **PER_LIB)
    return ref, arrs, res


# ------------------------------------------------------------------------------------------------ 7. the status word

def test_status_word_and_stores_stay_inside(route):
    v, d, D, keep = low_views(route)
    k0, n = 100, 1000
    cases = [("descends", [100, 400, 300, 900, 1100], capi.BINS_DESCENDS), ("descends at the end", [100, 500, 499], capi.BINS_DESCENDS),
             ("descends all the way", list(range(1100, 99, -10)), capi.BINS_DESCENDS),
             ("below k0", [50, 400, 1100], capi.BINS_OUTSIDE), ("above k0 + n", [100, 400, 1101], capi.BINS_OUTSIDE),
             ("both ends outside", [0, 400, 1500], capi.BINS_OUTSIDE), ("negative and huge", [-5, 400, 2 ** 31 - 1], capi.BINS_OUTSIDE),
             ("outside and descending", [1400, 700, 20], capi.BINS_OUTSIDE | capi.BINS_DESCENDS)]
    for what, edges, bits in cases:
        nb = len(edges) - 1
        rc, st, gs, gc, gh = call(route, v, d, k0, n, 0, edges, THR, 16)
        assert rc == 0 and st == bits, (what, rc, st)
        assert untouched(gs[:, :, nb:], gc[:, :, nb:]), "%s: wrote into the padding" % what
        assert (gs[:, :, :nb] != SENT64).all() and (gh.sum(axis=1) <= n).all(), what
        if not bits & capi.BINS_DESCENDS:                     # edges outside count as the window's ends: the values are defined
            clipped = [min(max(x, k0), k0 + n) for x in edges]
            w = reference(D, k0, n, 0, clipped, THR, 16)
            assert np.array_equal(gs[:, :, :nb], w["sums"]) and np.array_equal(gc[:, :, :nb], w["covered"]) and np.array_equal(gh, w["hist"]), what
    # without a status word the call is as good
    rc, st, gs, gc, gh = call(route, v, d, k0, n, 0, [100, 400, 300, 1100], THR, 16, want=("sums",))
    assert rc == 0 and st == SENT and untouched(gs[:, :, 3:], gc, gh)


# ------------------------------------------------------------------------------------------------ 8. outputs, determinism, refusals

def test_each_output_alone_and_two_calls_give_identical_bytes(route):
    v, d, D, keep = low_views(route)
    kw = dict(width=100, thr=THR, n_hist=16)
    w = reference(D, 5, 1400, 100, None, THR, 16)
    nb = 14
    a = call(route, v, d, 5, 1400, **kw)
    b = call(route, v, d, 5, 1400, **kw)
    assert a[0] == b[0] == 0 and all(x.tobytes() == y.tobytes() for x, y in zip(a[2:], b[2:]))
    for one in ("sums", "covered", "hist", "status"):
        rc, st, gs, gc, gh = call(route, v, d, 5, 1400, want=(one,), **kw)
        assert rc == 0, one
        assert st == (0 if one == "status" else SENT), one
        assert np.array_equal(gs[:, :, :nb], w["sums"]) and untouched(gs[:, :, nb:]) if one == "sums" else untouched(gs), one
        assert np.array_equal(gc[:, :, :nb], w["covered"]) and untouched(gc[:, :, nb:]) if one == "covered" else untouched(gc), one
        assert np.array_equal(gh, w["hist"]) if one == "hist" else untouched(gh), one
    assert call(route, v, d, 5, 1400, want=(), **kw)[0] == 0
    # hist wanted with n_hist == 0, covered wanted without thresholds: nothing to write
    rc, st, gs, gc, gh = call(route, v, d, 5, 1400, width=100)
    assert rc == 0 and st == 0 and np.array_equal(gs[:, :, :nb], w["sums"])
    # n == 0 and n_bins == 0: every bin there is is empty, the histogram is zero
    rc, st, gs, gc, gh = call(route, v, d, 7, 0, 0, [7, 7, 7], THR, 4)
    assert rc == 0 and st == 0 and not gs[:, :, :2].any() and not gc[:, :, :2].any() and not gh.any() and untouched(gs[:, :, 2:], gc[:, :, 2:])
    rc, st, gs, gc, gh = call(route, v, d, 7, 0, 64, None, THR, 4)
    assert rc == 0 and st == 0 and not gh.any() and untouched(gs, gc)
    rc, st, gs, gc, gh = call(route, v, d, 7, 100, 0, [50], THR, 4)
    assert rc == 0 and st == 0 and not gh.any() and untouched(gs, gc)
    t = route.bins.last_timing()
    assert t["bytes_written"] > 0
    call(route, v, d, 5, 1400, **kw)
    t = route.bins.last_timing()
    assert t["kernel_s"] > 0 and t["bytes_read"] >= 5 * 4 * 2 * 1400


def test_refused_calls_write_nothing(route, low_region):
    ref, arrs, res = low_region
    eng = td.computed(route.engine_lib, arrs, 50, 2950, ref, **PER_LIB)
    v, d = ts.views_of(eng)
    P = int(v.n_pos)

    def av(**kw):
        w = capi.DeviceView.from_buffer_copy(v)
        for k, x in kw.items():
            setattr(w, k, x)
        return w

    def ad(**kw):
        w = capi.DeviceIndels.from_buffer_copy(d)
        for k, x in kw.items():
            setattr(w, k, x)
        return w
    assert d.n_slots > 0
    other = capi.MEM_HOST if route.mem == capi.MEM_DEVICE else capi.MEM_DEVICE
    ok = dict(v=v, d=d, k0=0, n=100, width=10, thr=(1, 2), n_hist=4)
    cases = [("no handle", dict(handle=False)), ("no view", dict(v=None)), ("no indel view", dict(d=None)), ("no parameters", dict(params=False)),
             ("k0 < 0", dict(k0=-1)), ("n < 0", dict(n=-1)), ("k0 + n > n_pos", dict(k0=P - 5, n=6)), ("k0 beyond the planes", dict(k0=P + 1, n=0)),
             ("memory of the other kind", dict(v=av(memory=other), d=ad(memory=other))), ("memory 0", dict(v=av(memory=0), d=ad(memory=0))),
             ("views of two kinds", dict(d=ad(memory=other))), ("another device", dict(v=av(device=int(v.device) + 1), d=ad(device=int(v.device) + 1))),
             ("views of two devices", dict(v=av(device=int(v.device) + 1))), ("a view without planes", dict(v=av(si=None))),
             ("a view without planes (depth)", dict(v=av(depth=None))), ("not a view", dict(v=capi.DeviceView())),
             ("records without their arrays", dict(d=ad(slots=None))), ("records without the third-allele array", dict(v=av(xagg=None, n_xagg=5))),
             ("n_lib differs", dict(d=ad(n_lib=1))), ("pos0 differs", dict(d=ad(pos0=int(d.pos0) + 1))), ("n_pos differs", dict(d=ad(n_pos=P - 1))),
             ("a window that ends behind index 2^31 - 1", dict(v=av(n_pos=2 ** 31 + 64, stride=2 ** 31 + 64), d=ad(n_pos=2 ** 31 + 64), k0=2 ** 31 - 50, n=100)),
             ("width < 0", dict(width=0, ds=4, fields=dict(width=-1))), ("width 0 without edges", dict(width=0, ds=4)),
             ("both width and edges", dict(width=0, edges=[0, 50, 100], fields=dict(width=10))),
             ("n_thr > 8", dict(thr=tuple(range(9)))), ("n_thr < 0", dict(fields=dict(n_thr=-1))),
             ("n_hist > 4096", dict(n_hist=4097)), ("n_hist < 0", dict(n_hist=-1)),
             ("dst_stride < n_bins", dict(ds=9)), ("dst_stride < n_bins of a list", dict(width=0, edges=[0, 50, 100], ds=1)),
             ("n_bins < 0", dict(width=0, edges=[0, 50, 100], fields=dict(n_bins=-1))), ("n_bins < 0 with a width", dict(fields=dict(n_bins=-1)))]
    for what, kw in cases:
        a = dict(ok, **kw)
        rc, st, gs, gc, gh = call(route, a.pop("v"), a.pop("d"), a.pop("k0"), a.pop("n"), **a)
        assert rc == capi.E_ARG, what
        assert st == SENT and untouched(gs, gc, gh), "%s: something was written" % what
        if kw.get("handle", True):
            assert route.bins.lib.brc_bins_last_error(route.bins.h), what
    rc, st, gs, gc, gh = call(route, v, d, 0, 100, 10, ds=10)
    assert rc == 0 and route.bins.lib.brc_bins_last_error(route.bins.h) == b""
    eng.close()


# ------------------------------------------------------------------------------------------------ 9. tensors.bins

def check_bins(route, r, D, k0, n, width=0, edges=None, thr=(), n_hist=0, what=""):
    w = reference(D, k0, n, width, edges, thr, n_hist)
    assert r["n_bins"] == w["sums"].shape[2] and r["first"] == D.pos0 + k0 and r["n"] == n and r["n_lib"] == D.n_lib and r["pos0"] == D.pos0, what
    for k in ("sums", "covered", "hist"):
        a = r[k]
        assert isinstance(a, np.ndarray) if route.name == "sim" else a.is_cuda, (what, k)
        a = a if route.name == "sim" else a.view(route.torch.int64).cpu().numpy().view(np.uint64)
        assert a.dtype == np.uint64 and a.shape == w[k].shape and np.array_equal(a, w[k]), (what, k)
    st = r["status"] if route.name == "sim" else r["status"].view(route.torch.int32).cpu().numpy().view(np.uint32)
    assert st.shape == (1,) and st[0] == 0, what
    if width:
        start = r["start"] if route.name == "sim" else r["start"].cpu().numpy()
        assert start.dtype == np.int64 and np.array_equal(start, D.pos0 + k0 + np.arange(r["n_bins"]) * width), what
    else:
        assert "start" not in r, what


def test_tensors_bins_on_text_only_engines_and_after_a_fetch(route, oracle_lib, test_bam):
    from bam_readcount_amd import tensors
    beg0, end = 10403000, 10403700
    res, text = td.oracle_result(oracle_lib, test_bam, beg0, end, test_bam["ref"], tid=20, chrom="21")
    D = Dense.of(res)
    P, p0 = res.n_pos, res.pos0
    for opts in (dict(text_only=True), dict(device_text="21")):
        eng = td.computed(route.engine_lib, test_bam, beg0, end, test_bam["ref"], tid=20, **opts)
        check_bins(route, tensors.bins(eng, route.bins, width=100, thresholds=(10, 20), hist=32), D, 0, P, 100, None, (10, 20), 32, "before fetch %r" % opts)
        eng.fetch_result()
        assert eng.format_region("21") == text
        check_bins(route, tensors.bins(eng, route.bins, width=100, thresholds=(10, 20), hist=32), D, 0, P, 100, None, (10, 20), 32, "after fetch %r" % opts)
        # a window in reference coordinates, clipped to the planes, with a host edge list in reference positions
        assert P > 200
        e = [p0 + 70, p0 + 71, p0 + 150, p0 + 150, p0 + P]
        r = tensors.bins(eng, route.bins, edges=e, beg0=p0 + 70, end=10 ** 9, thresholds=(1,), hist=3)
        check_bins(route, r, D, 70, P - 70, 0, [x - p0 for x in e], (1,), 3, "edges")
        if route.name == "hip":
            t = route.torch.tensor(e, dtype=route.torch.int32, device="cuda")
            check_bins(route, tensors.bins(eng, route.bins, edges=t, beg0=p0 + 70, thresholds=(1,), hist=3), D, 70, P - 70, 0, [x - p0 for x in e], (1,), 3, "device edges")
        r = tensors.bins(eng, route.bins, width=64, want=("hist",), hist=5)
        assert sorted(r) == ["first", "hist", "n", "n_bins", "n_lib", "pos0", "start", "status"]
        r = tensors.bins(eng, route.bins, width=7, beg0=p0 + P + 5)
        assert r["n"] == 0 and r["n_bins"] == 0 and tuple(r["sums"].shape) == (1, NSUM, 0) and tuple(r["covered"].shape) == (1, 0, 0)
        bad = [dict(), dict(width=10, edges=[p0, p0 + 5]), dict(width=0), dict(width=-3), dict(width=2.5), dict(edges=[]), dict(edges=[p0 + 5, p0 + 4]),
               dict(edges=[p0 - 1, p0 + 4]), dict(edges=[p0, p0 + P + 1]), dict(edges=[[p0, p0 + 1]]), dict(edges=[p0, p0 + 1.5]),
               dict(edges=[p0 + 10, p0 + 20], beg0=p0 + 11), dict(width=5, thresholds=range(9)), dict(width=5, thresholds=(-1,)), dict(width=5, hist=4097),
               dict(width=5, hist=-1), dict(width=5, want=("sums", "depth"))]
        for b in bad:
            with pytest.raises(ValueError):
                tensors.bins(eng, route.bins, **b)
        eng.close()


# ------------------------------------------------------------------------------------------------ 10. the host sanitizers

def _serialize(v, d, calls):
    b = ts._serialize(v, d, [])
    b = b[:36] + struct.pack("<i", len(calls)) + b[40:]
    for k0, n, width, edges, thr, n_hist, want in calls:
        nb = count_bins(n, width, edges)
        b += struct.pack("<qqqqqii8Iii", k0, n, width, nb if edges is not None else 0, nb + PAD, len(thr), n_hist, *(list(thr) + [0] * (8 - len(thr))),
                         want, 1 if edges is not None else 0)
        if edges is not None:
            b += np.asarray(edges, np.int32).tobytes()
    return b


def _sanitized(tmp_path, name, v, d, D, calls):
    """bins_check_asan over one pair of host views: every call must return 0 without a report and give the reference's values, with the
    padding and every destination that was not wanted as they were filled; returns the number of bins compared"""
    assert v.memory == capi.MEM_HOST and d.memory == capi.MEM_HOST
    case, out = str(tmp_path / (name + ".bin")), str(tmp_path / (name + ".res"))
    open(case, "wb").write(_serialize(v, d, calls))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    pr = subprocess.run([side.sim_checker(side.SIDE["bins"]), case, out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert pr.returncode == 0, (name, pr.stderr.decode()[-3000:])
    assert pr.stdout.decode().strip() == "%d calls" % len(calls), name
    raw = open(out, "rb").read(); o = 0
    L, some = D.n_lib, 0
    for k0, n, width, edges, thr, n_hist, want in calls:
        w = reference(D, k0, n, width, edges, thr, n_hist)
        nb = w["sums"].shape[2]; ds = nb + PAD
        rc, st = struct.unpack_from("<iI", raw, o); o += 8
        assert rc == 0 and st == (0 if want & 8 else SENT), (name, k0, n, width, edges, rc, st)
        gs = np.frombuffer(raw, np.uint64, L * NSUM * ds, o).reshape(L, NSUM, ds); o += gs.nbytes
        gc = np.frombuffer(raw, np.uint64, L * len(thr) * ds, o).reshape(L, len(thr), ds); o += gc.nbytes
        gh = np.frombuffer(raw, np.uint64, L * n_hist, o).reshape(L, n_hist); o += gh.nbytes
        what = (name, k0, n, width, edges, want)
        assert (np.array_equal(gs[:, :, :nb], w["sums"]) and untouched(gs[:, :, nb:])) if want & 1 else untouched(gs), what
        assert (np.array_equal(gc[:, :, :nb], w["covered"]) and untouched(gc[:, :, nb:])) if want & 2 else untouched(gc), what
        assert np.array_equal(gh, w["hist"]) if want & 4 else untouched(gh), what
        some += nb
    assert o == len(raw), name
    return some


def test_calls_under_the_host_sanitizers(oracle_lib, sim_route, tmp_path, monkeypatch):
    """The hand-built views and the window and edge cases of the tests above on the CPU build with -fsanitize=address,undefined: sources
    of exactly the views' sizes, an edge list of exactly n_bins + 1 elements, destinations of exactly [.][n_bins + PAD] — a load or
    store outside them is a report — and the results are the reference's.  One engine-made region carries third-allele records."""
    route = sim_route
    v, d, D, keep = low_views(route)
    calls = [(k0, n, width, edges, THR, 16, 15) for k0, n, width, edges in window_calls(D.n_pos)]
    for k0, n in ((0, D.n_pos), (37, 1301)):
        calls += [(k0, n, 0, edges, THR, 16, (15, 1, 2, 4, 8, 7)[i % 6]) for i, edges in enumerate(grain_lists(k0, n).values())]
    calls += [(7, 0, 0, [7, 7, 7], THR, 4, 15), (7, 0, 64, None, THR, 4, 15), (0, 1500, 10 ** 12, None, (), 0, 15)]
    assert _sanitized(tmp_path, "low", v, d, D, calls) > 1000
    v, d, D, keep = big_depth_views(route)
    _sanitized(tmp_path, "big", v, d, D, [(0, D.n_pos, kw.get("width", 0), kw.get("edges"), BIG_THR, kw["n_hist"], 15) for kw in BIG_CALLS])
    for what, (v, d, h, keep), _ in ts.refchar_views(route):
        D = Dense.of_hand(h)
        _sanitized(tmp_path, "ref", v, d, D, [(0, D.n_pos, w, None, (1,), 2, 15) for w in (1, 4, 64)] + [(3, D.n_pos - 5, 0, [3, 9, D.n_pos - 2], (), 0, 1)])
    v, d, D, keep = lib254_views(route)
    _sanitized(tmp_path, "lib254", v, d, D, [(0, D.n_pos, 7, None, (1, 3), 4, 15), (3, 65, 0, [3, 10, 10, 67, 68], (1,), 0, 15)])
    monkeypatch.setenv("BRC_FORCE_DOM", "3"); monkeypatch.setenv("BRC_XEV_CAP", "1")
    ref, arrs = td.third_allele_inputs()
    res, _ = td.oracle_result(oracle_lib, arrs, 100, 1900, ref, **PER_LIB)
    eng = td.computed(route.knob_lib, arrs, 100, 1900, ref, **PER_LIB)
    monkeypatch.delenv("BRC_FORCE_DOM"); monkeypatch.delenv("BRC_XEV_CAP")
    v, d = ts.views_of(eng)
    assert v.n_xagg > 0 and d.n_slots > 0
    D = Dense.of(res)
    _sanitized(tmp_path, "third", v, d, D, [(k0, n, width, edges, (1, 8), 8, 15) for k0, n, width, edges in window_calls(res.n_pos)[::3]])
    eng.close()
