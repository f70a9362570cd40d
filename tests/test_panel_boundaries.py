"""brc_panel_gather over hand-made views (tests/handmade_views.py): lists that end on every wave and workgroup edge and lay runs of
one index across elements 63 | 64 and 255 | 256 (P1); third-allele records whose position is listed first, last, in a run of 1, 2 and
300 equal elements, and nowhere — below the list, between two listed positions, above it — lists that begin with negative indices and
end with indices >= P, and a list equal to a window, which must give brc_dense_expand's bytes (P2); the status word alone (P3).  The
reference is expand_reference's columns at the listed indices — plain Python — compared as uint32 bit patterns.

Every body runs on [sim] (tests/sim_panel, CPU suite) and on [hip] (the product's library, gpu-marked).  DESIGN.md 5, "Hand-made views at
the edges of the dense, panel and indel libraries", has the census and the mutants these tests were run against."""
import struct

import numpy as np
import pytest

import handmade_views as hv
from route import Route

KINDS = hv.KINDS
L, P = 3, 513
K_REC = (5, 100, 101, 300, P - 1)          # the positions that carry third-allele records


@pytest.fixture(scope="module", params=["sim", pytest.param("hip", marks=pytest.mark.gpu)])
def route(request):
    return Route(request.param, ("dense", "panel"))


_case = []


def case():
    """(arrays, records, reference) of the one view of this file: 3 libraries, 513 positions, stride == P; two records on every
    position of K_REC, unused ones, and records outside the view"""
    if not _case:
        A = hv.unique_arrays(L, P)
        rec = []
        for j, k in enumerate(K_REC):
            rec.append(hv.record(k, j % L, 4 + j % 2, *hv.body(2 * j + 1)))
            rec.append(hv.record(k, (j + 1) % L, int(A["slotid"][0, k]) & 0xFF, *hv.body(2 * j + 2)))       # a bucket slot 0 names: the record wins
        rec += [hv.record(hv.NONE32, 0, 1, *hv.body(90), pad=9), hv.record(100, L, 4, *hv.body(91)), hv.record(101, 0, 6, *hv.body(92)),
                hv.record(P, 0, 4, *hv.body(93)), hv.record(1 << 31, 1, 4, *hv.body(94)), hv.record(0xFFFFFFFE, 1, 4, *hv.body(95))]
        rec = [rec[i] for i in np.random.default_rng(5).permutation(len(rec))]
        want = hv.expand_reference(A, rec)
        assert hv.assert_equals_fp32_division(want, L) == 0
        assert not np.array_equal(want["istat"], hv.expand_reference(A)["istat"])
        _case.append((A, rec, want))
    return _case[0]


@pytest.fixture(scope="module")
def view(route):
    A, rec, want = case()
    v, keep = hv.make_view(route, A, rec, stride=P, pos0=77)
    yield v
    del keep


def check(route, v, idx, ds, what, status=0, skew=False):
    want = case()[2]
    rc, st, got = hv.run_panel(route, v, idx, ds, skew=skew)
    assert rc == 0, (what, route.panel.lib.brc_panel_last_error(route.panel.h))
    assert st == status, (what, st)
    hv.assert_planes(got, hv.panel_columns(want, idx), len(idx), what)
    return got


def run_across(n, at, index):
    """an ascending list of n elements whose elements at - 2 .. at + 2 all hold `index`"""
    below = list(range(index - (at - 2), index)); run = [index] * 5
    return (below + run + list(range(index + 1, index + 1 + max(n - len(below) - 5, 0))))[:n]


def p1_lists():
    out = []
    for n in (1, 63, 64, 65, 255, 256, 257, 513):
        out.append(("%d ascending" % n, list(range(3, 3 + n)) if n < P else list(range(P))))
        out.append(("%d with gaps" % n, sorted({(j * P) // n for j in range(n)})))
        if n >= 65:                                                        # (100 and 300 carry records; 513 elements leave no room above them)
            out.append(("%d, a run across 63 | 64" % n, run_across(n, 64, 100 if n < P else 62)))
        if n >= 257:
            out.append(("%d, a run across 255 | 256" % n, run_across(n, 256, 300 if n < P else 254)))
    return out


def p2_lists():
    """(name, list, status)"""
    below_between_above = list(range(6, 100)) + list(range(102, 300))
    return [("a record's position first", [5, 6, 7, 200], 0), ("a record's position last", [7, 8, 99, 300], 0), ("the last position listed", [0, 511, P - 1], 0),
            ("a run of 1", [99, 100, 102], 0), ("a run of 2", [99, 100, 100, 101, 101, 102], 0), ("a run of 300", [4] + [100] * 300 + [101] * 300 + [102], 0),
            ("records below, between and above the list", below_between_above, 0),
            ("negative indices first, indices >= P last", [-2 ** 31, -5, -1, 5, 100, 300, P - 1, P, P + 1, 2 ** 31 - 1], hv.OOR),
            ("nothing but indices outside", [-3, -2, P, P], hv.OOR)]


def test_the_lists_hold_what_their_names_say():
    for name, idx in p1_lists():
        assert idx == sorted(idx) and 0 <= idx[0] and idx[-1] < P, name
    n = {name: idx for name, idx in p1_lists()}
    assert len(set(n["257, a run across 255 | 256"][254:259])) == 1 and len(set(n["65, a run across 63 | 64"][62:67])) == 1
    assert [len(idx) for name, idx in p1_lists() if "ascending" in name] == [1, 63, 64, 65, 255, 256, 257, 513]
    nowhere = p2_lists()[6][1]
    assert not set(K_REC) & set(nowhere) and K_REC[0] < nowhere[0] and nowhere[-1] < K_REC[3] and 99 in nowhere and 102 in nowhere


def test_p1_lists_on_every_wave_and_workgroup_edge(route, view):
    for c, (name, idx) in enumerate(p1_lists()):
        n = len(idx)
        check(route, view, idx, n if c % 2 == 0 else n + 3, name, skew=c % 3 == 1)


_other = {}


def other_case(name):
    """D2's slot situations and D4's numbers (through slots and through records), the views of test_dense_boundaries.py"""
    if name not in _other:
        A, rec = (hv.d2_arrays()[0], []) if name == "d2" else hv.d4_case(name == "d4_records")[:2]
        _other[name] = (A, rec, hv.expand_reference(A, rec))
    return _other[name]


@pytest.mark.parametrize("name", ["d2", "d4_slots", "d4_records"])
def test_p1_slot_situations_and_numbers_through_lists(route, name):
    """gather_lane restates expand_lane: b0 == b1, slot 1 alone, bucket ids 6 .. 0xFE and garbage in the upper half on lanes 0, 63 and
    64 of a list, and the counts, sums and rounding ties of D4; the one NaN sum's cell is a NaN and left out of the comparison"""
    A, rec, want = other_case(name)
    n_pos = A["ncol"].shape[1]
    v, keep = hv.make_view(route, A, rec, stride=n_pos)
    lists = [list(range(k0, k0 + 65)) for k0 in range(hv.D2_KINDS)] + [list(range(n_pos)), list(range(0, n_pos, 3)), [j // 2 for j in range(2 * n_pos)]]
    nans = 0
    for c, idx in enumerate(lists):
        rc, st, got = hv.run_panel(route, v, idx, len(idx) + 3 * (c % 2))
        assert rc == 0 and st == 0
        cols = hv.panel_columns(want, idx)
        nan = int(np.isnan(cols["metrics"].view(np.float32)).sum())
        hv.assert_planes(got, cols, len(idx), "%s list %d" % (name, c), nan_cells=nan)
        nans = max(nans, nan)
    assert nans == (0 if name == "d2" else 2)                                 # (the list that names every position twice meets it twice)


def test_p2_records_listed_first_last_in_runs_and_nowhere(route, view):
    for c, (name, idx, status) in enumerate(p2_lists()):
        check(route, view, idx, len(idx) + 3 * (c % 2), name, status=status)


@pytest.mark.parametrize("k0,n", [(0, P), (1, 257), (63, 65), (99, 3), (P - 64, 64), (300, 1)])
def test_p2_a_list_equal_to_a_window_gives_the_dense_bytes(route, view, k0, n):
    rc, dense = hv.run_dense(route, view, k0, n, n + 3)
    assert rc == 0
    got = check(route, view, list(range(k0, k0 + n)), n + 3, "window %r as a list" % ((k0, n),))
    for k in KINDS:
        assert got[k].tobytes() == dense[k].tobytes(), k


def p3_lists():
    desc_64 = list(range(64)) + [62] + list(range(70, 80))                 # the one descent lies across elements 63 | 64
    desc_256 = list(range(256)) + [200] + list(range(300, 310))            # ... across 255 | 256
    return [("clean", list(range(0, P, 2)), 0), ("equal neighbours", [7] * 70, 0), ("a descent across 63 | 64", desc_64, hv.DESC),
            ("a descent across 255 | 256", desc_256, hv.DESC), ("the last element outside", list(range(300)) + [P], hv.OOR),
            ("element 256 negative, then in order", [-1] * 257 + [3], hv.OOR), ("both", [5, -1, P], hv.OOR | hv.DESC), ("empty", [], 0)]


def test_p3_the_status_word_alone(route, view):
    """no destination: library 0's lanes judge the list, nothing but the word is written; n == 0: the word is cleared"""
    assert view.n_lib == 3
    for name, idx, status in p3_lists():
        rc, st, got = hv.run_panel(route, view, idx, len(idx), kinds=())
        assert rc == 0 and st == status, (name, rc, st)
    rc, st, got = hv.run_panel(route, view, [], 0)                         # n == 0 with destinations and a status word
    assert rc == 0 and st == 0 and all(g.size == 0 for g in got.values())
    rc, st, got = hv.run_panel(route, view, [3, 4], 2, status=False)       # no status word: it keeps the sentinel
    assert rc == 0 and st == hv.SENT


def test_handmade_lists_under_the_host_sanitizers(tmp_path):
    """P2's lists (and the runs of P1) through panel_check_asan: a view with stride == P of exactly its sizes, lists of exactly n
    indices, destinations of exactly (planes - 1) * dst_stride + n elements."""
    A, rec, want = case()
    lists = p2_lists() + [(name, idx, 0) for name, idx in p1_lists() if "run" in name]
    tail = [struct.pack("<qq", len(idx), len(idx) + 3 * (c % 2)) + np.asarray(idx, np.int32).tobytes() for c, (_, idx, _) in enumerate(lists)]
    d = hv.run_checker("panel", hv.serialize_view(A, rec, None, 77, tail), tmp_path, "%d lists" % len(lists)).view(np.uint32)
    o = 0
    for c, (name, idx, status) in enumerate(lists):
        n, ds = len(idx), len(idx) + 3 * (c % 2)
        assert d[o].view(np.int32) == 0 and d[o + 1] == status, name
        got, o = hv.read_checked(d, o + 2, L, n, ds)
        hv.assert_planes(got, hv.panel_columns(want, idx), n, "asan: " + name)
    assert o == d.size
