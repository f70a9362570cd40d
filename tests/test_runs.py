"""Device-side depth-class intervals (include/brc_runs.h): brc_runs_find and bam_readcount_amd.tensors.runs against the header's definition
written in numpy over the ORACLE's dense brc_result (depth, refbase) — searchsorted(cuts, V, "right"), boundaries from diff — start, end,
cls, counts and per_class equal exactly, no tolerance.

Every body runs twice (the `route` fixture): [sim] = libbrc_sim.so + tests/sim_runs/libbrc_runs_sim.so, host memory, in the CPU suite;
[hip] = the product's libraries on the GPU (gpu-marked), lists, counts, per_class and scratch in device memory allocated through torch.
Destinations are filled with 0xA5 bytes first and are PAD elements wider than needed: everything at or behind min(total, cap), the
padding behind per_class and every destination that was not asked for must keep them.  The scratch has exactly brc_runs_workspace
bytes.  The host sanitizers run the CPU build over the hand-built views, the window and the cap cases.

Where no engine can produce the shape — a class change at a given lane, depths of 2^31, 254 libraries, reference characters and slices of
every kind — the views are built by hand (test_select.build_views) in the route's memory, and the reference is the same numpy over the
dense depths given.

Sizes that matter to the kernels (brc_runs.hip): a wave is 64 consecutive positions, a workgroup and a scan tile 256 with one halo
position on either side, the scan of the workgroups' counts takes 256 of them per pass — a window of more than 65536 positions makes it
carry."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from bam_readcount_amd import capi
import abi_side as side
from route import Route, SENT
import synth
import test_dense as td
import test_select as ts

LIBS = ("dense", "select", "runs")
SENT64 = np.uint64(0xA5A5A5A5A5A5A5A5)
PAD = 3                                   # elements of every destination behind what the contract writes
MAXC = capi.RUNS_MAX_CUT + 2              # the most classes a call can have
MIN, MAX, SUM = capi.RUNS_MIN, capi.RUNS_MAX, capi.RUNS_SUM
ALL = ("start", "end", "cls", "counts", "per_class")
PER_LIB = ts.PER_LIB


@pytest.fixture(scope="module", params=["sim", pytest.param("hip", marks=pytest.mark.gpu)])
def route(request):
    return Route(request.param, LIBS, engine=True)


@pytest.fixture(scope="module")
def sim_route():
    return Route("sim", LIBS, engine=True)


# ------------------------------------------------------------------------------------------------ the reference

def all_classes(cuts, ref_n=False):
    return (1 << (len(cuts) + (2 if ref_n else 1))) - 1


def classes_of(D, k0, n, cuts, combine=MIN, role=None, ref_n=False):
    """class(k) of the header for the window, int64 [n]; D has .depth [L, P] and .refbase (P characters)"""
    role = np.ones(D.depth.shape[0], np.int64) if role is None else np.asarray(role, np.int64)
    d = D.depth[role == 1][:, k0:k0 + n].astype(np.uint64)
    V = d.min(axis=0) if combine == MIN else d.max(axis=0) if combine == MAX else d.sum(axis=0, dtype=np.uint64)
    c = np.searchsorted(np.asarray(cuts, np.uint64), V, "right").astype(np.int64)
    if ref_n:
        rb = ts._REFCODE[np.frombuffer(bytes(D.refbase), np.uint8)[k0:k0 + n]]
        c = np.where(rb < 0, len(cuts) + 1, c)
    return c


def reference(D, k0, n, cuts, combine=MIN, role=None, keep=None, ref_n=False):
    """(start, end, cls: int64 [m] of the emitted runs, per_class uint64 [n_cut + 2])"""
    keep = all_classes(cuts, ref_n) if keep is None else keep
    c = classes_of(D, k0, n, cuts, combine, role, ref_n)
    per = np.bincount(c, minlength=len(cuts) + 2).astype(np.uint64)
    if n == 0:
        z = np.zeros(0, np.int64)
        return z, z, z, per
    b = np.flatnonzero(np.diff(c)) + 1
    s = np.concatenate([[0], b]); e = np.concatenate([b, [n]]); cl = c[s]
    ok = ((keep >> cl) & 1).astype(bool)
    return s[ok] + k0, e[ok] + k0, cl[ok], per


# ------------------------------------------------------------------------------------------------ calling the library

def call(route, v, d, k0, n, cap, cuts=(1,), combine=MIN, role=None, keep=None, flags=0, want=ALL, handle=True, params=True, ws=True, fields=None):
    """brc_runs_find into sentinel-filled buffers of cap + PAD elements (per_class: MAXC + PAD) and a scratch of exactly
    brc_runs_workspace bytes.  fields: members of brc_runs_params set afterwards (for the refusals).
    Returns (rc, counts word, start words, end words, cls words, per_class quads)"""
    par, keepalive = capi.runs_params(cuts, combine, role, keep, flags)
    for k, x in (fields or {}).items():
        setattr(par, k, x)
    c = max(cap, 0)
    bs, be, bc, bn, bp = route.sentinel_words(c + PAD), route.sentinel_words(c + PAD), route.sentinel_words(c + PAD), route.sentinel_words(1), route.sentinel_words(2 * (MAXC + PAD))
    wsb = route.runs.workspace(n)
    assert wsb % 4 == 0 and wsb == (4 * n + 8 * ((n + 255) // 256) if n > 0 else 0)
    bw = route.sentinel_words(wsb // 4)
    rc = route.runs.lib.brc_runs_find(route.runs.h if handle else None, C.byref(v) if v is not None else None, C.byref(d) if d is not None else None,
                                      C.byref(par) if params else None, k0, n, cap, route.ptr(bs) if "start" in want else None,
                                      route.ptr(be) if "end" in want else None, route.ptr(bc) if "cls" in want else None,
                                      route.ptr(bn) if "counts" in want else None, route.ptr(bp) if "per_class" in want else None,
                                      route.ptr(bw) if ws and wsb else None, None)
    del keepalive
    return (rc, int(route.words(bn)[0]), route.words(bs)[:c + PAD].copy(), route.words(be)[:c + PAD].copy(), route.words(bc)[:c + PAD].copy(),
            route.words(bp)[:2 * (MAXC + PAD)].view(np.uint64).copy())


def untouched(*arrays):
    return all((a == (SENT64 if a.dtype == np.uint64 else SENT)).all() for a in arrays)


def check(route, v, d, D, k0=0, n=None, cuts=(1,), combine=MIN, role=None, keep=None, ref_n=False, what="", caps=(), min_runs=0, min_classes=0, with_d=None):
    """counts and per_class alone, then the list at cap = total (and at `caps`), against the reference; returns the wanted
    (start, end, cls, per_class).  The indels view is passed only with ref_n (or with_d): the flag off works with NULL."""
    n = D.n_pos - k0 if n is None else n
    w0, w1, wc, wp = reference(D, k0, n, cuts, combine, role, keep, ref_n)
    m, nc = len(w0), len(cuts) + 2
    assert m >= min_runs and len(set(wc.tolist())) >= min_classes, "%s: the reference gives %d runs of %d classes: choose other cuts" % (what, m, len(set(wc.tolist())))
    assert int(wp.sum()) == n
    dd = d if (ref_n if with_d is None else with_d) else None
    kw = dict(cuts=cuts, combine=combine, role=role, keep=keep, flags=capi.RUNS_REF_N if ref_n else 0)
    rc, total, gs, ge, gc, gp = call(route, v, dd, k0, n, 0, want=("counts", "per_class"), **kw)
    assert rc == 0, (what, route.runs.lib.brc_runs_last_error(route.runs.h))
    assert total == m, (what, total, m)
    assert np.array_equal(gp[:nc], wp) and untouched(gp[nc:], gs, ge, gc), (what, gp[:nc], wp)
    for cap in [m] + list(caps):
        rc, total, gs, ge, gc, gp = call(route, v, dd, k0, n, cap, **kw)
        t = min(m, cap)
        assert rc == 0 and total == m, (what, cap, rc, total)
        assert np.array_equal(gs[:t].view(np.int32), w0[:t].astype(np.int32)), (what, cap, gs[:8].view(np.int32), w0[:8])
        assert np.array_equal(ge[:t].view(np.int32), w1[:t].astype(np.int32)), (what, cap, ge[:8].view(np.int32), w1[:8])
        assert np.array_equal(gc[:t], wc[:t].astype(np.uint32)), (what, cap, gc[:8], wc[:8])
        assert untouched(gs[t:], ge[t:], gc[t:]), "%s: wrote behind the list (cap %d)" % (what, cap)
        assert np.array_equal(gp[:nc], wp) and untouched(gp[nc:]), (what, cap)
    return w0, w1, wc, wp


def hand(route, depth, ref=None, **kw):
    """hand-built views that expand to the depths given (no base counts: the intervals read depth alone)"""
    depth = np.asarray(depth, np.uint32)
    depth = depth[None, :] if depth.ndim == 1 else depth
    return ts.build_views(route, depth, np.zeros((depth.shape[0], 4, depth.shape[1]), np.uint32), ref, **kw)


# ------------------------------------------------------------------------------------------------ 1. the golden fixtures

def test_golden_fixtures(route, oracle_lib, test_bam, twolib, low_region):
    """test_bam.npz all-lib; twolib.npz per library and with both libraries counted, under MIN / MAX / SUM.  On test_bam.npz the
    oracle-side reference gives at least three runs of at least two classes.  twolib.npz CANNOT, under any cuts: it holds four reads,
    library 0 has depth 1 on the first 120 positions and 0 behind, library 1 the reverse, and the reference is ACGT throughout — per
    library that is two runs of two classes, and with both counted MIN is 0 everywhere, MAX and SUM are 1 everywhere: one run.  It runs
    all the same and the test asserts exactly that structure; the two-library synthetic batch `low_region` (test_select's stand-in for
    the same fixture) carries the "at least three runs, at least two classes" condition per library and with both counted."""
    beg0, end = 10402736, 10405248
    res, _ = td.oracle_result(oracle_lib, test_bam, beg0, end, test_bam["ref"], tid=20)
    eng = td.computed(route.engine_lib, test_bam, beg0, end, test_bam["ref"], tid=20)
    v, d = ts.views_of(eng)
    D = ts.Dense.of(res)
    for combine in (MIN, MAX, SUM):
        check(route, v, d, D, cuts=(1, 10, 30, 60), combine=combine, what="test_bam %d" % combine, min_runs=3, min_classes=2)
    check(route, v, d, D, cuts=(10, 30), keep=0b1010, ref_n=True, what="test_bam callable", min_runs=3, min_classes=1)
    eng.close()
    names = [str(s) for s in twolib["lib_names"]]
    opts = dict(lib_names=names, per_lib=True, insertion_centric=True, ref_len_check=True)
    end = int(twolib["ref"].size)
    res, _ = td.oracle_result(oracle_lib, twolib, 0, end, twolib["ref"], **opts)
    assert res.n_lib == 2 and res.depth.max() == 1
    eng = td.computed(route.engine_lib, twolib, 0, end, twolib["ref"], **opts)
    v, d = ts.views_of(eng)
    D = ts.Dense.of(res)
    for combine in (MIN, MAX, SUM):
        for role in ([1, 0], [0, 1]):
            w0, w1, wc, wp = check(route, v, d, D, cuts=(1, 2), combine=combine, role=role, ref_n=True, what="twolib %r %d" % (role, combine), min_runs=2, min_classes=2)
            assert len(w0) == 2
        w0, w1, wc, wp = check(route, v, d, D, cuts=(1, 2), combine=combine, what="twolib both %d" % combine, min_runs=1)
        assert len(w0) == 1 and wc[0] == (0 if combine == MIN else 1)
    eng.close()
    ref, arrs, res = low_region
    eng = td.computed(route.engine_lib, arrs, 50, 2950, ref, **PER_LIB)
    v, d = ts.views_of(eng)
    D = ts.Dense.of(res)
    for combine in (MIN, MAX, SUM):
        for role in ([1, 0], [0, 1], None):
            check(route, v, d, D, cuts=(1, 3, 6), combine=combine, role=role, ref_n=True, what="two synthetic libraries %r %d" % (role, combine), min_runs=3, min_classes=2)
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. shapes the kernels can get wrong

SHAPE_P = 700
SHAPE_CUTS = (3, 8)


def shape_depths():
    """name -> (depth [P] of one library, keep): classes under SHAPE_CUTS are 0 (depth 0), 1 (depth 5), 2 (depth 10)"""
    P = SHAPE_P
    k = np.arange(P)
    out = {}
    out["one run over everything"] = (np.full(P, 5), None)
    out["alternating every position"] = (np.where(k % 2, 5, 0), None)
    out["alternating, one class kept"] = (np.where(k % 2, 5, 0), 0b010)
    x = np.zeros(P, np.int64); x[64:256] = 5; x[320:512] = 10
    out["changes at lanes 63 | 64 and 255 | 256"] = (x, None)
    out["a kept run between dropped ones"] = (x, 0b010)
    out["dropped runs between kept ones"] = (x, 0b101)
    x = np.zeros(P, np.int64); x[[0, 5, 7, 63, 64, 65, 129, 255, 256, 263, 320, P - 78, P - 77, P - 1]] = 5
    out["single positions at the windows' ends"] = (x, None)
    out["single positions, kept alone"] = (x, 0b010)
    x = np.zeros(P, np.int64); x[64:128] = np.where(k[64:128] % 2, 5, 10); x[320:384] = np.where(k[320:384] % 2, 10, 5)
    out["a full wave of kept single-position runs between dropped stretches"] = (x, 0b110)
    return out


def test_shapes_and_windows_off_the_grid(route):
    """n of 1, 63 / 64 / 65, 257; windows off the 64-grid; a change at lanes 63 | 64 and 255 | 256; runs of one position at k0 and at
    k0 + n - 1; one run over several workgroups (no start in most of them); classes alternating every position (256 starts and ends
    per workgroup); kept between dropped and the reverse; a full wave of kept single-position runs"""
    wins = ts.window_list(SHAPE_P) + [(64, 192), (256, 256), (7, 257), (263, 1), (63, 2)]
    for name, (depth, keep) in shape_depths().items():
        v, d, D, keepalive = hand(route, depth)
        for k0, n in wins:
            w0, w1, wc, wp = check(route, v, d, D, k0, n, cuts=SHAPE_CUTS, keep=keep, what="%s, window %r" % (name, (k0, n)), caps=(1,))
            if keep is None:                            # every class kept: the runs tile the window
                assert w0[0] == k0 and w1[-1] == k0 + n and np.array_equal(w0[1:], w1[:-1]), name
        w0, w1, wc, wp = reference(D, 0, SHAPE_P, SHAPE_CUTS, keep=keep)
        if name.startswith("one run"):
            assert len(w0) == 1
        if name == "alternating every position":
            assert len(w0) == SHAPE_P
        if name.startswith("a full wave"):
            assert len(w0) == 128 and (w1 - w0 == 1).all()
        if name.startswith("single positions, kept"):
            r = reference(D, 7, 257, SHAPE_CUTS, keep=keep)
            assert r[0][0] == 7 and r[1][0] == 8 and r[0][-1] == 263 and r[1][-1] == 264      # a run of one position at k0 and at k0 + n - 1


def test_scan_carry_over_more_than_256_workgroups(route):
    """70 000 positions of alternating short runs = 274 workgroups: the scan of their counts takes two passes and carries (the only larger
    case)"""
    P = 70000
    rng = np.random.default_rng(9)
    lens = rng.integers(1, 6, P)
    depth = np.repeat(np.arange(P) % 3 * 5, lens)[:P]
    v, d, D, keepalive = hand(route, depth)
    w0, w1, wc, wp = check(route, v, d, D, cuts=SHAPE_CUTS, keep=0b101, what="70000 positions", min_runs=10000, min_classes=2)
    assert (w0 > 256 * 256).sum() > 64 and (w0 < 256 * 256).sum() > 64


# ------------------------------------------------------------------------------------------------ 3. values

def test_cuts_met_exactly_and_the_number_of_cuts(route):
    P = 300
    depth = np.arange(P) % 20
    v, d, D, keepalive = hand(route, depth)
    c = classes_of(D, 0, P, (3, 7))
    assert c[2] == 0 and c[3] == 1 and c[6] == 1 and c[7] == 2                              # met exactly, missed by one
    check(route, v, d, D, cuts=(3, 7), what="cuts 3, 7", min_runs=3, min_classes=3)
    check(route, v, d, D, cuts=(7,), what="one cut", min_runs=3, min_classes=2)
    cuts15 = tuple(range(15))                                                               # cut[0] == 0: no position has class 0
    w0, w1, wc, wp = check(route, v, d, D, cuts=cuts15, what="15 cuts from 0", min_runs=3, min_classes=15)
    assert wp[0] == 0 and wc.min() == 1 and wc.max() == 15
    check(route, v, d, D, 5, 290, cuts=cuts15, keep=1 << 15, what="15 cuts, the last class alone", min_runs=3)
    check(route, v, d, D, cuts=(0, 2 ** 32 - 1), what="cuts 0 and 2^32 - 1")


def big_views(route):
    """depths of 2^31 in four libraries at some positions: their sum is 2^33, a 32-bit sum would be 0"""
    P = 130
    depth = np.ones((4, P), np.uint32)
    depth[:, 10:20] = 2 ** 31; depth[:, 64] = 2 ** 31; depth[:3, 100:110] = 2 ** 31; depth[:, 129] = 2 ** 32 - 1
    return hand(route, depth)


BIG_CUTS = (5, 2 ** 32 - 1)


def test_sums_beyond_32_bits(route):
    v, d, D, keepalive = big_views(route)
    c = classes_of(D, 0, D.n_pos, BIG_CUTS, SUM)
    assert c[10] == 2 and c[64] == 2 and c[0] == 0 and c[100] == 2 and c[129] == 2
    wrapped = np.searchsorted(np.asarray(BIG_CUTS, np.uint64), D.depth.astype(np.uint64).sum(axis=0) & np.uint64(2 ** 32 - 1), "right")
    assert wrapped[10] == 0 and wrapped[64] == 0                                            # a 32-bit sum picks another class
    check(route, v, d, D, cuts=BIG_CUTS, combine=SUM, what="sum of 2^31 x 4", min_runs=3, min_classes=2)
    check(route, v, d, D, cuts=BIG_CUTS, combine=MAX, what="max of 2^31")
    check(route, v, d, D, cuts=(2 ** 31, 2 ** 31 + 1), combine=MIN, what="min of 2^31", min_runs=3)


def two_lib_views(route):
    P = 400
    k = np.arange(P)
    depth = np.stack([np.where((k // 37) % 2, 12, 2), np.where((k // 53) % 2, 30, 0)])
    return hand(route, depth)


def test_combine_and_roles(route):
    """MIN and MAX differ; a role that ignores the deciding library changes the list"""
    v, d, D, keepalive = two_lib_views(route)
    got = {}
    for combine in (MIN, MAX, SUM):
        for role in (None, [1, 0], [0, 1]):
            r = check(route, v, d, D, cuts=(1, 10, 20), combine=combine, role=role, what="combine %d role %r" % (combine, role), min_runs=3, min_classes=2)
            got[combine, str(role)] = (r[0].tolist(), r[2].tolist())
    assert got[MIN, "None"] != got[MAX, "None"] and got[MIN, "None"] != got[MIN, "[1, 0]"] and got[MAX, "None"] != got[MAX, "[1, 0]"]
    assert got[MIN, "[1, 0]"] == got[MAX, "[1, 0]"] == got[SUM, "[1, 0]"]                   # one library: the three are one
    check(route, v, d, D, 3, 390, cuts=(1, 10, 20), combine=MIN, role=[1, 1], what="roles given, all counted", with_d=True)


def lib254_views(route):
    depth, cnt, ref = ts.low_depth(70, L=254, seed=3, alt=0.02)
    depth = depth + (np.arange(70) // 5 % 3).astype(np.uint32)[None, :]                     # (the minimum over 127 libraries varies too)
    return hand(route, depth, ref)


LIB254_ROLE = [l % 2 for l in range(254)]


def test_254_libraries_with_alternating_roles(route):
    v, d, D, keepalive = lib254_views(route)
    assert v.n_lib == 254
    for combine, cuts in ((MIN, (1, 2)), (MAX, (11, 13)), (SUM, (600, 700, 800))):
        check(route, v, d, D, cuts=cuts, combine=combine, role=LIB254_ROLE, ref_n=True, what="254 libraries %d" % combine, min_runs=3, min_classes=2)
    # one library more is refused
    v2 = capi.DeviceView.from_buffer_copy(v); d2 = capi.DeviceIndels.from_buffer_copy(d); v2.n_lib = d2.n_lib = 255
    assert call(route, v2, d2, 0, 1, 0)[0] == capi.E_ARG and call(route, v2, None, 0, 1, 0)[0] == capi.E_ARG


# ------------------------------------------------------------------------------------------------ 4. the reference

def test_reference_characters_slices_and_no_reference(route):
    """acgt, N, IUPAC codes, NUL and bytes above 127; slices that start late, end early or pass ref_len; no reference: with
    BRC_RUNS_REF_N such positions have class n_cut + 1; with the flag off and a NULL indels view the reference is nobody's business"""
    kinds = set()
    for what, (v, d, D, keepalive), _ in ts.refchar_views(route):
        kinds.add((bool(d.ref), d.ref_lo > d.pos0, d.ref_hi < d.pos0 + d.n_pos, d.ref_len < d.ref_hi))
        w0, w1, wc, wp = check(route, v, d, D, cuts=(5, 7), ref_n=True, what=what + ", ref_n")
        check(route, v, d, D, 3, D.n_pos - 5, cuts=(5, 7), ref_n=True, keep=1 << 3, what=what + ", the no-reference class alone")
        if what == "characters":
            assert wp[3] == D.n_pos - 8 * 4 and wp[1] == 8 * 4 and len(w0) == 2                # ACGTacgt, four positions each, depth 6
        if what == "no reference":
            assert not d.ref and wp[3] == D.n_pos and len(w0) == 1
        w = check(route, v, d, D, cuts=(5, 7), what=what + ", flag off, NULL indels view")
        assert w[3][3] == 0 and len(w[0]) == 1
        check(route, v, d, D, cuts=(5, 7), what=what + ", flag off, indels view given", with_d=True)
    assert len(kinds) >= 5                              # whole, none, late, early, cut by ref_len


@pytest.fixture(scope="module")
def low_region(oracle_lib):
    """a synthetic low-depth region of two libraries and the oracle's result of it (test_select's)"""
    rng = np.random.default_rng(11)
    ref = synth.make_ref(rng, 3000, weird=0.01)
    arrs = synth.make_batch(77, ref, 260, read_len=(60, 120), style="indel", n_libs=2, mismatch=0.06)
    res, _ = td.oracle_result(oracle_lib, arrs, 50, 2950, ref, **PER_LIB)
    return ref, arrs, res


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
    full = ts.Dense.of(res)
    D = ts.Dense(full.depth * announced, full.cnt, full.refbase, [], full.pos0)
    assert D.depth[:, asked].any() and announced.sum() < res.n_pos // 2
    for combine in (MIN, MAX, SUM):
        w0, w1, wc, wp = check(route, v, d, D, cuts=(1, 4), combine=combine, ref_n=True, what="site list %d" % combine, min_runs=3, min_classes=2)
        assert wp[0] >= res.n_pos - announced.sum() - 40
    eng.close()


# ------------------------------------------------------------------------------------------------ 5. the contract

def low_views(route):
    depth, cnt, ref = ts.low_depth(1500, seed=4)
    return ts.build_views(route, depth, cnt, ref)


LOW_CUTS = (1, 4, 8)


def test_capacity_outputs_and_determinism(route):
    v, d, D, keepalive = low_views(route)
    P = D.n_pos
    w0, w1, wc, wp = check(route, v, d, D, cuts=LOW_CUTS, what="capacity", min_runs=65, min_classes=3, caps=[0, 1, 63, 64, 65])
    m = len(w0)
    check(route, v, d, D, cuts=LOW_CUTS, what="total - 1 and beyond", caps=[m - 1, m + 5])
    # ascending, disjoint, tiling; one class, all classes, sum(per_class) == n
    assert w0[0] == 0 and w1[-1] == P and np.array_equal(w0[1:], w1[:-1]) and int(wp.sum()) == P
    for c in range(4):
        x0, x1, xc, xp = check(route, v, d, D, 5, P - 9, cuts=LOW_CUTS, keep=1 << c, what="class %d alone" % c, min_runs=3)
        assert (xc == c).all() and (x0 < x1).all() and (x1[:-1] < x0[1:]).all() and int((x1 - x0).sum()) == int(xp[c])
    kw = dict(cuts=LOW_CUTS, combine=SUM, keep=0b0110)
    a = call(route, v, d, 3, P - 3, m, **kw)
    b = call(route, v, d, 3, P - 3, m, **kw)
    assert a[0] == b[0] == 0 and a[1] == b[1] and all(x.tobytes() == y.tobytes() for x, y in zip(a[2:], b[2:]))
    # each output alone
    w0, w1, wc, wp = reference(D, 0, P, LOW_CUTS)
    for one in ALL:
        rc, total, gs, ge, gc, gp = call(route, v, None, 0, P, m, cuts=LOW_CUTS, want=(one,))
        assert rc == 0, one
        assert total == (m if one == "counts" else SENT), one
        assert (np.array_equal(gs[:m].view(np.int32), w0) and untouched(gs[m:])) if one == "start" else untouched(gs), one
        assert (np.array_equal(ge[:m].view(np.int32), w1) and untouched(ge[m:])) if one == "end" else untouched(ge), one
        assert (np.array_equal(gc[:m], wc) and untouched(gc[m:])) if one == "cls" else untouched(gc), one
        assert (np.array_equal(gp[:5], wp) and untouched(gp[5:])) if one == "per_class" else untouched(gp), one
    rc, total, gs, ge, gc, gp = call(route, v, None, 0, P, m, cuts=LOW_CUTS, want=())
    assert rc == 0 and total == SENT and untouched(gs, ge, gc, gp)
    assert route.runs.last_timing()["bytes_read"] == 0
    call(route, v, None, 0, P, m, cuts=LOW_CUTS)
    t = route.runs.last_timing()
    assert t["kernel_s"] > 0 and t["bytes_read"] >= 4 * 2 * P and t["bytes_written"] >= 4 * P
    assert route.runs.workspace(0) == 0 and route.runs.workspace(-5) == 0 and route.runs.workspace(257) == 4 * 257 + 16


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
    ok = dict(v=v, d=d, k0=0, n=100, cap=8, cuts=(2, 5), role=[1, 1])
    cases = [("no handle", dict(handle=False)), ("no view", dict(v=None)), ("no parameters", dict(params=False)),
             ("k0 < 0", dict(k0=-1)), ("n < 0", dict(n=-1)), ("k0 + n > n_pos", dict(k0=P - 5, n=6)), ("k0 beyond the planes", dict(k0=P + 1, n=0)),
             ("memory of the other kind", dict(v=av(memory=other), d=ad(memory=other))), ("memory 0", dict(v=av(memory=0), d=ad(memory=0))),
             ("memory of the other kind, no indels view", dict(v=av(memory=other), d=None)),
             ("views of two kinds", dict(d=ad(memory=other))), ("another device", dict(v=av(device=int(v.device) + 1), d=ad(device=int(v.device) + 1))),
             ("another device, no indels view", dict(v=av(device=int(v.device) + 1), d=None)),
             ("views of two devices", dict(v=av(device=int(v.device) + 1))), ("a view without planes", dict(v=av(si=None))),
             ("a view without planes (depth)", dict(v=av(depth=None))), ("not a view", dict(v=capi.DeviceView())), ("not a view, alone", dict(v=capi.DeviceView(), d=None)),
             ("records without their arrays", dict(d=ad(slots=None))), ("records without the third-allele array", dict(v=av(xagg=None, n_xagg=5))),
             ("n_lib differs", dict(d=ad(n_lib=1))), ("pos0 differs", dict(d=ad(pos0=int(d.pos0) + 1))), ("n_pos differs", dict(d=ad(n_pos=P - 1))),
             ("a window that ends behind index 2^31 - 1", dict(v=av(n_pos=2 ** 31 + 64, stride=2 ** 31 + 64), d=ad(n_pos=2 ** 31 + 64), k0=2 ** 31 - 50, n=100)),
             ("a role above 1", dict(role=[1, 2])), ("no counted library", dict(role=[0, 0])),
             ("an unknown combine", dict(combine=3)), ("unknown flags", dict(flags=2)), ("unknown flags beside the known one", dict(flags=5)),
             ("n_cut 0", dict(cuts=(), keep=1)), ("n_cut 16", dict(fields=dict(n_cut=16))), ("n_cut huge", dict(fields=dict(n_cut=2 ** 32 - 1))),
             ("cuts equal", dict(cuts=(2, 2))), ("cuts descending", dict(cuts=(1, 5, 4))), ("keep 0", dict(keep=0)),
             ("keep with a bit above n_cut + 1", dict(keep=1 << 4)), ("keep with a high bit beside low ones", dict(keep=0b111 | 1 << 31)),
             ("BRC_RUNS_REF_N without an indels view", dict(d=None, flags=capi.RUNS_REF_N)),
             ("cap < 0", dict(cap=-1)), ("no workspace", dict(ws=False))]
    for what, kw in cases:
        a = dict(ok, **kw)
        rc, total, gs, ge, gc, gp = call(route, a.pop("v"), a.pop("d"), a.pop("k0"), a.pop("n"), a.pop("cap"), **a)
        assert rc == capi.E_ARG, what
        assert total == SENT and untouched(gs, ge, gc, gp), "%s: something was written" % what
        if kw.get("handle", True):
            assert route.runs.lib.brc_runs_last_error(route.runs.h), what
    # n == 0 is fine: the count is 0, per_class is zero, nothing else is written
    for dd in (d, None):
        rc, total, gs, ge, gc, gp = call(route, v, dd, 7, 0, 8, cuts=(2, 5))
        assert (rc, total) == (0, 0) and not gp[:4].any() and untouched(gs, ge, gc, gp[4:])
    assert call(route, v, None, P, 0, 0, want=())[0] == 0
    assert route.runs.lib.brc_runs_last_error(route.runs.h) == b""
    # keep with the no-reference class although the flag is off: allowed, and never emitted
    rc, total, gs, ge, gc, gp = call(route, v, None, 0, 100, 4, cuts=(2, 5), keep=1 << 3)
    assert (rc, total) == (0, 0) and untouched(gs, ge, gc) and gp[3] == 0 and int(gp[:4].sum()) == 100
    eng.close()


# ------------------------------------------------------------------------------------------------ 6. tensors.runs

def check_runs(route, r, D, k0, n, cuts, what, **kw):
    w0, w1, wc, wp = reference(D, k0, n, cuts, **kw)
    assert sorted(r) == ["cls", "end", "k0", "k1", "n", "n_class", "per_class", "start"], what
    assert r["n"] == len(w0) > 0 and r["n_class"] == len(cuts) + 2, (what, r["n"], len(w0))
    for k, w in (("k0", w0), ("k1", w1), ("start", w0 + D.pos0), ("end", w1 + D.pos0), ("cls", wc)):
        a = route.host(r[k])
        assert a.dtype == np.int32 and np.array_equal(a, w.astype(np.int32)), (what, k)
        assert isinstance(r[k], np.ndarray) if route.name == "sim" else r[k].is_cuda, (what, k)
    p = r["per_class"] if route.name == "sim" else r["per_class"].view(route.torch.int64).cpu().numpy().view(np.uint64)
    assert p.dtype == np.uint64 and np.array_equal(p, wp), what


def test_tensors_runs_on_text_only_engines_and_after_a_fetch(route, oracle_lib, test_bam):
    from bam_readcount_amd import tensors
    beg0, end = 10403000, 10403700
    res, text = td.oracle_result(oracle_lib, test_bam, beg0, end, test_bam["ref"], tid=20, chrom="21")
    D = ts.Dense.of(res)
    P, p0 = res.n_pos, res.pos0
    cuts = (10, 30, 50)
    for opts in (dict(text_only=True), dict(device_text="21")):
        eng = td.computed(route.engine_lib, test_bam, beg0, end, test_bam["ref"], tid=20, **opts)
        check_runs(route, tensors.runs(eng, route.runs, cuts=cuts), D, 0, P, cuts, "before fetch %r" % opts)
        eng.fetch_result()
        assert eng.format_region("21") == text
        check_runs(route, tensors.runs(eng, route.runs, cuts=cuts, combine="sum", ref_n=True), D, 0, P, cuts, "after fetch %r" % opts, combine=SUM, ref_n=True)
        # a window in reference coordinates, clipped to the planes; one class kept; a library by number
        r = tensors.runs(eng, route.runs, cuts=cuts, combine="max", libs=[0], keep=(1, 2), beg0=p0 + 70, end=10 ** 9)
        check_runs(route, r, D, 70, P - 70, cuts, "window", combine=MAX, keep=0b0110)
        e = tensors.runs(eng, route.runs, cuts=cuts, beg0=p0 + P + 5)
        assert e["n"] == 0 and tuple(e["k0"].shape) == (0,) and tuple(e["start"].shape) == (0,) and tuple(e["per_class"].shape) == (5,)
        bad = [dict(cuts=()), dict(cuts=range(16)), dict(cuts=(5, 5)), dict(cuts=(5, 4)), dict(cuts=(-1,)), dict(cuts=(2 ** 32,)), dict(cuts=(1.5,)),
               dict(cuts=cuts, combine="mean"), dict(cuts=cuts, combine=0), dict(cuts=cuts, keep=()), dict(cuts=cuts, keep=(5,)), dict(cuts=cuts, keep=(-1,)),
               dict(cuts=cuts, libs=[]), dict(cuts=cuts, libs=[1]), dict(cuts=cuts, libs=[0, 0]), dict(cuts=cuts, libs=["nobody"])]
        for b in bad:
            with pytest.raises(ValueError):
                tensors.runs(eng, route.runs, **b)
        with pytest.raises(TypeError):
            tensors.runs(eng, route.runs)                   # (cuts has no default)
        eng.close()


def test_tensors_runs_names_and_the_chain_into_bins(route, oracle_lib, low_region):
    """libs= by name on a per-library engine; ref_n without an indels view; runs["k0"] / ["k1"] of a kept class as the edges of
    tensors.bins: the bins' depth sums equal the reference's over those intervals"""
    from bam_readcount_amd import tensors
    import test_bins as tb
    bins = route.another("bins")
    ref, arrs, res = low_region
    names = PER_LIB["lib_names"]
    D = ts.Dense.of(res)
    P, p0 = res.n_pos, res.pos0
    eng = td.computed(route.engine_lib, arrs, 50, 2950, ref, **PER_LIB)
    cuts = (2, 5)
    check_runs(route, tensors.runs(eng, route.runs, cuts=cuts, libs=[names[1]]), D, 0, P, cuts, "one library by name", role=[0, 1])
    check_runs(route, tensors.runs(eng, route.runs, cuts=cuts, libs=names[0].encode(), combine="max"), D, 0, P, cuts, "bytes", role=[1, 0], combine=MAX)
    check_runs(route, tensors.runs(eng, route.runs, cuts=cuts, libs=names), D, 0, P, cuts, "both by name")
    r = tensors.runs(eng, route.runs, cuts=cuts, keep=2, ref_n=True)                        # callable: at least 5 in both libraries, reference known
    check_runs(route, r, D, 0, P, cuts, "callable", keep=1 << 2, ref_n=True)
    w0, w1, wc, wp = reference(D, 0, P, cuts, keep=1 << 2, ref_n=True)
    assert len(w0) >= 3
    # the intervals and the gaps between them as bins: even bins are the runs
    k0, k1 = route.host(r["k0"]).astype(np.int64), route.host(r["k1"]).astype(np.int64)
    assert np.array_equal(route.host(r["start"]), k0 + p0) and np.array_equal(route.host(r["end"]), k1 + p0)
    edges = np.stack([k0, k1], axis=1).reshape(-1) + p0
    b = tensors.bins(eng, bins, edges=edges, want=("sums",))
    s = b["sums"] if route.name == "sim" else b["sums"].view(route.torch.int64).cpu().numpy().view(np.uint64)
    want = np.array([[int(D.depth[l, x:y].sum()) for x, y in zip(w0, w1)] for l in range(2)], np.uint64)
    assert b["n_bins"] == 2 * len(w0) - 1 and np.array_equal(s[:, capi.BINS_S_DEPTH, ::2], want) and want.all()
    if route.name == "hip":                                 # the device route of the chain: the edge list never leaves the GPU
        t = route.torch.stack([r["start"], r["end"]], dim=1).reshape(-1).contiguous()
        b = tensors.bins(eng, bins, edges=t, want=("sums",))
        assert np.array_equal(b["sums"].view(route.torch.int64).cpu().numpy().view(np.uint64)[:, capi.BINS_S_DEPTH, ::2], want)
        assert int(b["status"].view(route.torch.int32)[0]) == 0

    class NoIndels:
        """an engine that has no indels view to give"""
        _names = eng._names

        def device_view(self):
            return eng.device_view()

        def device_indels(self):
            raise capi.BrcError("no indels view")
    with pytest.raises(ValueError):
        tensors.runs(NoIndels(), route.runs, cuts=cuts, ref_n=True)
    check_runs(route, tensors.runs(NoIndels(), route.runs, cuts=cuts), D, 0, P, cuts, "no indels view, flag off")
    eng.close()
    # names need an engine that keeps libraries apart
    eng = td.computed(route.engine_lib, arrs, 50, 2950, ref)
    with pytest.raises(ValueError, match="^libs names libraries: the engine reports one set of counts for all of them$"):
        tensors.runs(eng, route.runs, cuts=cuts, libs=[names[0]])
    eng.close()


# ------------------------------------------------------------------------------------------------ 7. the host sanitizers

WANT_ALL = 31


def _serialize(v, d, calls):
    b = ts._serialize(v, d, [])
    b = b[:36] + struct.pack("<i", len(calls)) + b[40:]
    for k0, n, cap, cuts, combine, role, keep, ref_n, want, with_d in calls:
        keep = all_classes(cuts, ref_n) if keep is None else keep
        b += struct.pack("<qqq4I15Iiii", k0, n, cap, combine, len(cuts), keep, capi.RUNS_REF_N if ref_n else 0, *(list(cuts) + [0] * (15 - len(cuts))),
                         0 if role is None else 1, want, 1 if with_d else 0)
        b += bytes(role or [])
    return b


def _sanitized(tmp_path, name, v, d, D, calls):
    """runs_check_asan over one pair of host views: every call must return 0 without a report and give the reference's values, with
    everything behind the list and every destination that was not wanted as it was filled; returns the number of runs compared"""
    assert v.memory == capi.MEM_HOST and d.memory == capi.MEM_HOST
    case, out = str(tmp_path / (name + ".bin")), str(tmp_path / (name + ".res"))
    open(case, "wb").write(_serialize(v, d, calls))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    pr = subprocess.run([side.sim_checker(side.SIDE["runs"]), case, out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert pr.returncode == 0, (name, pr.stderr.decode()[-3000:])
    assert pr.stdout.decode().strip() == "%d calls" % len(calls), name
    raw = open(out, "rb").read(); o = 0
    some = 0
    for k0, n, cap, cuts, combine, role, keep, ref_n, want, with_d in calls:
        w0, w1, wc, wp = reference(D, k0, n, cuts, combine, role, keep, ref_n)
        m, t, nc = len(w0), min(len(w0), cap), len(cuts) + 2
        what = (name, k0, n, cap, cuts, combine, keep, want)
        rc, total = struct.unpack_from("<iI", raw, o); o += 8
        assert rc == 0 and total == (m if want & 8 else SENT), what + (rc, total, m)
        gs = np.frombuffer(raw, np.int32, cap, o); o += 4 * cap
        ge = np.frombuffer(raw, np.int32, cap, o); o += 4 * cap
        gc = np.frombuffer(raw, np.uint32, cap, o); o += 4 * cap
        gp = np.frombuffer(raw, np.uint64, nc, o); o += 8 * nc
        ts_, te, tc = (t if want & 1 else 0), (t if want & 2 else 0), (t if want & 4 else 0)
        assert np.array_equal(gs[:ts_], w0[:ts_]) and untouched(gs[ts_:].view(np.uint32)), what
        assert np.array_equal(ge[:te], w1[:te]) and untouched(ge[te:].view(np.uint32)), what
        assert np.array_equal(gc[:tc], wc[:tc]) and untouched(gc[tc:]), what
        assert np.array_equal(gp, wp) if want & 16 else untouched(gp), what
        some += t
    assert o == len(raw), name
    return some


def _calls_of(D, k0, n, cuts, combine=MIN, role=None, keep=None, ref_n=False, every=True):
    """the forms of one call: the list at cap = total; with `every` also total - 1, counts and per_class alone, each list alone, and a
    capacity beyond the total without the count"""
    m = len(reference(D, k0, n, cuts, combine, role, keep, ref_n)[0])
    a = (cuts, combine, role, keep, ref_n)
    c = [(k0, n, m) + a + (WANT_ALL, ref_n)]
    if every:
        c += [(k0, n, max(m - 1, 0)) + a + (WANT_ALL, True), (k0, n, 0) + a + (8 | 16, ref_n), (k0, n, m) + a + (1, ref_n), (k0, n, m) + a + (2, ref_n),
              (k0, n, m) + a + (4, ref_n), (k0, n, m + 2) + a + (7, ref_n), (k0, n, 0) + a + (16, ref_n), (k0, n, 1) + a + (WANT_ALL, ref_n)]
    return c


def test_calls_under_the_host_sanitizers(sim_route, tmp_path):
    """The hand-built views with the window and cap cases of the tests above on the CPU build with -fsanitize=address,undefined, a
    stand-alone program: sources of exactly the views' sizes (the reference slice cut at ref_len, the role array of exactly n_lib
    bytes), a scratch of exactly brc_runs_workspace bytes, start / end / cls of exactly cap elements, per_class of exactly n_cut + 2 — a
    load or store outside them is a report — and the results are the reference's.  NOT the 70 000-position case: its carry is a loop
    of the device's k_runs_parts alone, which the CPU build does not have.  Never under the gpu mark; nothing is loaded into python
    with a sanitizer."""
    route = sim_route
    some = 0
    wins = ts.window_list(SHAPE_P) + [(64, 192), (256, 256), (263, 1)]
    for i, (name, (depth, keep)) in enumerate(shape_depths().items()):
        v, d, D, keepalive = hand(route, depth)
        calls = []
        for j, (k0, n) in enumerate(wins):
            calls += _calls_of(D, k0, n, SHAPE_CUTS, keep=keep, every=(i + j) % 4 == 0)
        calls.append((17, 0, 5, SHAPE_CUTS, MIN, None, keep, False, WANT_ALL, False))
        some += _sanitized(tmp_path, "shape%d" % i, v, d, D, calls)
    assert some > 3000
    v, d, D, keepalive = hand(route, np.arange(300) % 20)
    _sanitized(tmp_path, "cuts", v, d, D, [c for cuts in ((3, 7), (7,), tuple(range(15))) for c in _calls_of(D, 0, 300, cuts)])
    v, d, D, keepalive = big_views(route)
    _sanitized(tmp_path, "big", v, d, D, [c for combine in (MIN, MAX, SUM) for c in _calls_of(D, 0, D.n_pos, BIG_CUTS, combine)])
    v, d, D, keepalive = two_lib_views(route)
    _sanitized(tmp_path, "two", v, d, D, [c for combine in (MIN, MAX, SUM) for role in (None, [1, 0], [0, 1]) for c in _calls_of(D, 3, 390, (1, 10, 20), combine, role)])
    for what, (v, d, D, keepalive), _ in ts.refchar_views(route):
        _sanitized(tmp_path, "ref", v, d, D, _calls_of(D, 0, D.n_pos, (5, 7), ref_n=True) + _calls_of(D, 3, D.n_pos - 5, (5, 7), ref_n=True, keep=1 << 3) +
                   _calls_of(D, 0, D.n_pos, (5, 7), every=False))
    v, d, D, keepalive = lib254_views(route)
    _sanitized(tmp_path, "lib254", v, d, D, [c for combine, cuts in ((MIN, (1, 2)), (SUM, (600, 700, 800))) for c in _calls_of(D, 0, D.n_pos, cuts, combine, LIB254_ROLE, ref_n=True)])
    v, d, D, keepalive = low_views(route)
    _sanitized(tmp_path, "low", v, d, D, [c for k0, n in ts.window_list(D.n_pos) for c in _calls_of(D, k0, n, LOW_CUTS, SUM, ref_n=True)])


# ------------------------------------------------------------------------------------------------ 8. what a mutation pass of the core left standing

def test_roles_above_the_first_role_words(route):
    """254 libraries with a role pattern that is no copy of itself 16, 32, 64 or 128 libraries further (ts.lib_pattern), and one
    position per library at which that library alone decides the class: depth 10 everywhere, 0 (even libraries: the minimum) or 50
    (odd ones: the maximum) at position l of library l.  A role table indexed modulo 16 .. 128 libraries gives other classes under
    MIN, MAX and SUM — asserted on the reference's side."""
    L = 254
    role = ts.lib_pattern(2)
    depth = np.full((L, L), 10, np.uint32)
    depth[np.arange(L), np.arange(L)] = np.where(np.arange(L) % 2, 50, 0)
    v, d, D, keepalive = hand(route, depth)
    n1 = sum(role)
    for combine, cuts in ((MIN, (5,)), (MAX, (20,)), (SUM, (10 * n1 - 5, 10 * n1 + 5))):
        w = check(route, v, d, D, cuts=cuts, combine=combine, role=role, what="role pattern %d" % combine, min_runs=20, min_classes=2)
        c = classes_of(D, 0, L, cuts, combine, role)
        for period in (16, 32, 64, 128):
            assert not np.array_equal(c, classes_of(D, 0, L, cuts, combine, ts.folded(role, period))), (combine, period)
        assert (c[128:] != c[128:].min()).any() and (c[:128] != c[:128].min()).any()          # deciding libraries on both sides of 128


def test_one_list_alone_with_a_short_capacity(route):
    """`end` alone, `start` alone and `cls` alone at cap = total - 1, total and 0: exactly min(total, cap) elements of the one list,
    nothing else"""
    v, d, D, keepalive = low_views(route)
    P = D.n_pos
    w0, w1, wc, wp = reference(D, 0, P, LOW_CUTS)
    m = len(w0)
    assert m > 65
    want = {"start": w0.astype(np.int32).view(np.uint32), "end": w1.astype(np.int32).view(np.uint32), "cls": wc.astype(np.uint32)}
    for one in ("end", "start", "cls"):
        for cap in (m - 1, m, 0):
            rc, total, gs, ge, gc, gp = call(route, v, None, 0, P, cap, cuts=LOW_CUTS, want=(one,))
            got = {"start": gs, "end": ge, "cls": gc}
            t = min(m, cap)
            assert rc == 0 and total == SENT and untouched(gp), (one, cap)
            for k, g in got.items():
                if k == one:
                    assert np.array_equal(g[:t], want[k][:t]) and untouched(g[t:]), "%s alone, cap %d: %r" % (one, cap, g[max(t - 2, 0):t + PAD])
                else:
                    assert untouched(g), (one, cap, k)
            # ... and with the counts beside it
            rc, total, gs, ge, gc, gp = call(route, v, None, 0, P, cap, cuts=LOW_CUTS, want=(one, "counts"))
            g = {"start": gs, "end": ge, "cls": gc}[one]
            assert rc == 0 and total == m and np.array_equal(g[:t], want[one][:t]) and untouched(g[t:]), (one, cap)


def test_the_no_reference_class_with_8_and_15_cuts(route):
    """BRC_RUNS_REF_N with n_cut = 8 and n_cut = 15: class 9 and class 16 (the last bit of `keep` a call can have) appear, alone too"""
    P = 200
    k = np.arange(P)
    ref = bytes(b"ACGTN"[x] for x in (k // 3) % 5)
    depth = (k * 7 % 23).astype(np.uint32)
    v, d, D, keepalive = hand(route, depth, ref)
    for cuts in (tuple(range(1, 9)), tuple(range(1, 16))):
        nc = len(cuts)
        w0, w1, wc, wp = check(route, v, d, D, cuts=cuts, ref_n=True, what="%d cuts, ref_n" % nc, min_runs=20, min_classes=nc)
        assert (wc == nc + 1).sum() >= 10 and wp[nc + 1] == ref.count(b"N") and (wc == nc).any()
        x0, x1, xc, xp = check(route, v, d, D, 2, P - 5, cuts=cuts, ref_n=True, keep=1 << (nc + 1), what="%d cuts, the last class alone" % nc, min_runs=10)
        assert (xc == nc + 1).all()
        w = check(route, v, d, D, cuts=cuts, what="%d cuts, flag off" % nc, with_d=True)
        assert w[3][nc + 1] == 0


def test_sums_of_one_two_and_three_libraries_beyond_32_bits(route):
    """three libraries with depths around 2^31 and 2^32 - 1: counted alone a library's sum fits, with two and with three counted it
    passes 2^32 and a 32-bit sum lands in another class"""
    P = 70
    depth = np.ones((3, P), np.uint32)
    depth[:, 5:15] = [[2 ** 31 + 5], [2 ** 31 + 7], [2 ** 31]]; depth[:, 63:65] = 2 ** 32 - 1; depth[:2, 40:50] = 2 ** 31
    v, d, D, keepalive = hand(route, depth)
    cuts = (20, 2 ** 32 - 1)
    for role in ([1, 0, 0], [1, 1, 0], [0, 1, 1], [1, 1, 1]):
        w = check(route, v, d, D, cuts=cuts, combine=SUM, role=role, what="sum, roles %r" % role, min_runs=3, min_classes=2)
        c = classes_of(D, 0, P, cuts, SUM, role)
        s = D.depth[np.asarray(role) == 1].astype(np.uint64).sum(axis=0)
        wrapped = np.searchsorted(np.asarray(cuts, np.uint64), s & np.uint64(2 ** 32 - 1), "right")
        assert (wrapped != c).any() == (sum(role) > 1), role
        assert c[63] == (2 if sum(role) > 0 else 0) and c[5] == (2 if sum(role) > 1 else 1)
