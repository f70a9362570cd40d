"""brc_dense_expand over hand-made views (tests/handmade_views.py) at every edge the engine's own output never reaches: window and
stride geometry (D1), every slot situation on lanes 0, 63 and 64 (D2), third-allele records on the window's edges and outside the view
(D3), counts and sums at the edges of fp32 and quotients next to a rounding tie (D4).  The reference is expand_reference — plain
Python, no library under test — and everything is compared as uint32 bit patterns; the only cells left out are the metrics of the ONE
NaN sum D4 places (asserted to be NaNs).

Every body runs on [sim] (tests/sim_dense, CPU suite) and on [hip] (the product's library, gpu-marked).  DESIGN.md 5, "Hand-made views at
the edges of the dense, panel and indel libraries", has the census and the mutants these tests were run against."""
import struct

import numpy as np
import pytest

import handmade_views as hv
from route import Route

KINDS = hv.KINDS


@pytest.fixture(scope="module", params=["sim", pytest.param("hip", marks=pytest.mark.gpu)])
def route(request):
    return Route(request.param, ("dense",))


_cache = {}


def cached(key, make):
    """a case and its reference, computed once and shared by the routes"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def d1_views():
    """(L, P, stride): P = 1, 64, 257, 513 with stride == P and P rounded up to 64 (64: the next multiple); L = 1, 2, 3, 255"""
    return [(1, 1, 1), (255, 1, 64), (2, 64, 64), (255, 64, 128), (3, 257, 257), (2, 257, 320), (3, 513, 513), (1, 513, 576)]


def d1_windows(P):
    out = []
    for n in (1, 63, 64, 65, 255, 256, 257, 513):
        if n <= P:
            out += [(k0, n) for k0 in sorted({k for k in (0, 1, 63, 64, P - n) if 0 <= k <= P - n})]
    return out


def d1_case(L, P, stride):
    A = hv.unique_arrays(L, P)
    return A, hv.expand_reference(A)


def check(route, v, want, k0, n, ds, what, kinds=KINDS, skew=False):
    rc, got = hv.run_dense(route, v, k0, n, ds, kinds=kinds, skew=skew)
    assert rc == 0, (what, route.dense.lib.brc_dense_last_error(route.dense.h))
    cols = {k: want[k][:, k0:k0 + n] for k in kinds}
    nan = int(np.isnan(cols["metrics"].view(np.float32)).sum()) if "metrics" in kinds else 0
    hv.assert_planes(got, cols, n, what, nan_cells=nan)
    return nan


# ------------------------------------------------------------------------------------------------ 0. the references hold each other

def test_the_reference_alone_holds_on_every_constructed_cell():
    """Before any route runs: unique cell values and no duplicate records (asserted by the builders), the double-quotient metrics ==
    numpy's fp32 division (test_dense.metrics_of) on every constructed cell, the floor on rounding ties found, one NaN cell.  Prints
    the census DESIGN.md quotes (pytest -s)."""
    census = []
    for L, P, stride in d1_views():
        A, want = cached(("d1", L, P), lambda: d1_case(L, P, stride))
        assert hv.assert_equals_fp32_division(want, L) == 0
    census.append("D1: %d views, positions 1..513, libraries 1..255, %d windows" % (len(d1_views()), sum(len(d1_windows(P)) for _, P, _ in d1_views())))
    A, kinds = hv.d2_arrays()
    want = hv.expand_reference(A)
    assert hv.assert_equals_fp32_division(want, 2) == 0
    assert sorted(set(kinds.ravel().tolist())) == list(range(hv.D2_KINDS))
    census.append("D2: %d positions, 2 libraries, %d slot situations" % (A["ncol"].shape[1], hv.D2_KINDS))
    for R in (255, 256, 257):
        A, rec = hv.d3_case(R)
        assert hv.assert_equals_fp32_division(hv.expand_reference(A, rec), 2) == 0
    census.append("D3: 300 positions, 2 libraries, 255 / 256 / 257 records (4 unused, 6 outside the view)")
    nans = 0
    for via in (False, True):
        A, rec, n_found, n_nan = hv.d4_case(via)
        nans = hv.assert_equals_fp32_division(hv.expand_reference(A, rec), 1)
        assert nans == n_nan == 1
    ties, n_found = hv.rounding_ties()
    assert len(ties) == hv.TIE_FLOOR and n_found >= hv.TIE_FLOOR
    census.append("D4: %d positions, 1 library, %d rounding-tie pairs found by the search, the nearest %d placed (x 2 operand sizes x 9 quotient columns), "
                  "%d NaN cell left out" % (A["ncol"].shape[1], n_found, len(ties), nans))
    print("\n".join(census))


# ------------------------------------------------------------------------------------------------ D1 geometry

@pytest.mark.parametrize("L,P,stride", d1_views(), ids=lambda x: str(x))
def test_d1_windows_strides_and_libraries(route, L, P, stride):
    A, want = cached(("d1", L, P), lambda: d1_case(L, P, stride))
    v, keep = hv.make_view(route, A, stride=stride, pos0=1000)
    for c, (k0, n) in enumerate(d1_windows(P)):
        ds = n if c % 2 == 0 else n + 3
        check(route, v, want, k0, n, ds, "L %d P %d stride %d window %r ds %d" % (L, P, stride, (k0, n), ds), skew=c % 3 == 1)
    check(route, v, want, 0, P, P + 3, "whole", skew=True)


# ------------------------------------------------------------------------------------------------ D2 slots

def test_d2_every_slot_situation_on_lanes_0_63_and_64(route):
    A, kinds = cached("d2", hv.d2_arrays)
    want = cached("d2want", lambda: hv.expand_reference(A))
    P = A["ncol"].shape[1]
    v, keep = hv.make_view(route, A, stride=P)                            # (75: no multiple of 64, and equal to n_pos)
    seen = set()
    for k0 in range(hv.D2_KINDS):
        check(route, v, want, k0, 65, 65 + (k0 % 2), "D2 window from %d" % k0)
        seen |= {(int(kinds[l, k0 + lane]), lane) for l in range(2) for lane in (0, 63, 64)}
    assert seen == {(kind, lane) for kind in range(hv.D2_KINDS) for lane in (0, 63, 64)}
    check(route, v, want, 0, P, P, "D2 whole")


# ------------------------------------------------------------------------------------------------ D3 records

D3_WINDOWS = [(37, 130), (0, 300), (299, 1), (0, 1), (36, 1), (167, 133), (38, 128)]


@pytest.mark.parametrize("n_records", [255, 256, 257])
def test_d3_records_on_the_window_edges_and_outside_the_view(route, n_records):
    A, rec = cached(("d3", n_records), lambda: hv.d3_case(n_records))
    want = cached(("d3want", n_records), lambda: hv.expand_reference(A, rec))
    bare = cached("d3bare", lambda: hv.expand_reference(A))
    assert not np.array_equal(want["istat"], bare["istat"])
    v, keep = hv.make_view(route, A, rec, stride=320)
    for c, (k0, n) in enumerate(D3_WINDOWS):
        check(route, v, want, k0, n, n + 3 * (c % 2), "D3 %d records, window %r" % (n_records, (k0, n)))
    # each bucket destination alone; and depth alone: the record launch is skipped, nothing else is written
    k0, n = D3_WINDOWS[0]
    for kind in ("istat", "fstat", "metrics", "depth"):
        check(route, v, want, k0, n, n + 3, "D3 %s alone" % kind, kinds=(kind,))


def test_d3_a_view_whose_every_bucket_comes_from_records(route):
    A, rec = cached("d3empty", lambda: hv.d3_case(257, empty_slots=True))
    want = cached("d3emptywant", lambda: hv.expand_reference(A, rec))
    assert (A["slotid"] == 0xFFFF).all() and (want["istat"] != 0).any()
    v, keep = hv.make_view(route, A, rec, stride=300)
    for k0, n in D3_WINDOWS[:4]:
        check(route, v, want, k0, n, n, "D3 records only, window %r" % ((k0, n),))


# ------------------------------------------------------------------------------------------------ D4 numbers

@pytest.mark.parametrize("via_records", [False, True], ids=["slots", "records"])
def test_d4_counts_sums_rounding_ties_and_special_floats(route, via_records):
    A, rec, n_found, n_nan = cached(("d4", via_records), lambda: hv.d4_case(via_records))
    want = cached(("d4want", via_records), lambda: hv.expand_reference(A, rec))
    P = A["ncol"].shape[1]
    v, keep = hv.make_view(route, A, rec, stride=P)
    assert check(route, v, want, 0, P, P, "D4 whole") == n_nan == 1           # the cells left out of the bit comparison: this one
    assert check(route, v, want, 1, P - 1, P, "D4 from 1") == 1
    assert check(route, v, want, 0, P - 1, P - 1, "D4 without the NaN's position") == 0
    # fstat stays a bit copy, the NaN included
    rc, got = hv.run_dense(route, v, 0, P, P, kinds=("fstat",))
    assert rc == 0 and np.array_equal(got["fstat"], want["fstat"]) and (want["fstat"] == hv.QUIET_NAN).sum() == 1


# ------------------------------------------------------------------------------------------------ the host sanitizers

def test_handmade_views_under_the_host_sanitizers(tmp_path):
    """D2 and D3 (257 records) through dense_check_asan: sources of exactly the view's sizes (stride == P for D2), destinations of
    exactly (planes - 1) * dst_stride + n elements."""
    A2, _ = cached("d2", hv.d2_arrays)
    A3, rec3 = cached(("d3", 257), lambda: hv.d3_case(257))
    cases = [(A2, [], None, [(k0, 65, 65 + k0 % 2) for k0 in range(hv.D2_KINDS)]), (A3, rec3, 320, [(k0, n, n + 3 * (c % 2)) for c, (k0, n) in enumerate(D3_WINDOWS)])]
    for j, (A, rec, stride, wins) in enumerate(cases):
        want = hv.expand_reference(A, rec)
        d = hv.run_checker("dense", hv.serialize_view(A, rec, stride, 0, [struct.pack("<qqq", *w) for w in wins]), tmp_path, "%d windows" % len(wins))
        d = d.view(np.uint32); o = 0
        for k0, n, ds in wins:
            assert d[o].view(np.int32) == 0; o += 1
            got, o = hv.read_checked(d, o, A["ncol"].shape[0], n, ds)
            hv.assert_planes(got, {k: want[k][:, k0:k0 + n] for k in KINDS}, n, "asan case %d window %r" % (j, (k0, n, ds)))
        assert o == d.size
