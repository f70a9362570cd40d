"""Device-resident site panels (include/brc_panel.h): brc_device_view_get + brc_panel_gather, and bam_readcount_amd.tensors.sites,
against the ORACLE's dense brc_result indexed with numpy at the listed positions — integers equal, floats and the thirteen metric
columns (numpy's fp32 division on the oracle's planes) equal as uint32 bit patterns.

Every body runs twice (the `route` fixture): [sim] = libbrc_sim.so + tests/sim_panel/libbrc_panel_sim.so, host memory, in the CPU
suite; [hip] = the product's libraries on the GPU (gpu-marked), the index list, the status word and the destinations in device memory
allocated through torch.  Destinations are filled with 0xA5A5A5A5 first: the padding [n, dst_stride) of every plane must keep it.
The host sanitizers run the CPU build over every list of the suite.

Sizes that matter to the kernels (brc_panel.hip): a wave is 64 consecutive list elements, a workgroup 256 — the lists end at 63 / 64 /
65 and 257 elements, and lay runs of equal indices across element 64."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from bam_readcount_amd import capi
from conftest import GOLDEN
import abi_side as side
from route import Route, SENT
import test_dense as td
import test_indels as ti

KINDS = td.KINDS
OOR, DESC = 1, 2
planes_of = td.planes_of
PER_LIB = dict(lib_names=["libA", "libB"], per_lib=True)


@pytest.fixture(scope="module", params=["sim", pytest.param("hip", marks=pytest.mark.gpu)])
def route(request):
    return Route(request.param, ("dense", "panel", "indels"), engine=True)


def gather(route, view, idx, ds, kinds=KINDS, n=None, status=True, no_idx=False, handle=True, words=None):
    """brc_panel_gather of the list into sentinel-filled buffers of [planes][ds] (or `words` words each) and a sentinel-filled
    status word; returns (rc, status word, {kind: uint32 words [planes, ds]})"""
    L = int(view.n_lib) if view is not None and view.n_lib > 0 else 1
    n = len(idx) if n is None else n
    size = {k: planes_of(k, L) * max(ds, 0) if words is None else words for k in kinds}
    bufs = {k: route.sentinel_words(size[k]) for k in kinds}
    st = route.sentinel_words(1)
    ibuf = route.ints(idx)
    fn = route.panel.lib.brc_panel_gather
    args = {k: route.ptr(b) for k, b in bufs.items()}
    rc = fn(route.panel.h if handle else None, C.byref(view) if view is not None else None, None if no_idx else route.ptr(ibuf), n, ds,
            *[args.get(k) for k in KINDS], route.ptr(st) if status else None, None)
    out = {}
    for k, b in bufs.items():
        w = route.words(b)[:size[k]]
        out[k] = w.reshape(planes_of(k, L), max(ds, 0)) if words is None else w.reshape(1, -1)
    return rc, int(route.words(st)[0]), out


_columns = {}


def columns(res):
    """{kind: uint32 words [planes, P + 1]} of the oracle's result, computed once per result: column k is plane position k, column
    P an EMPTY position (what an index outside the planes is written as)"""
    if id(res) not in _columns:
        whole = td.want_planes(res, 0, res.n_pos)
        ext = {}
        for k, w in whole.items():
            e = np.full((w.shape[0], 1), 0xFFFFFFFF if k == "unavail" else 0, np.uint32)
            ext[k] = np.concatenate([w, e], axis=1)
            ext[k].setflags(write=False)
        _columns[id(res)] = (res, ext)
    return _columns[id(res)][1]


def want_at(res, idx, kinds=KINDS):
    idx = np.asarray(idx, np.int64)
    col = np.where((idx >= 0) & (idx < res.n_pos), idx, res.n_pos)
    c = columns(res)
    return {k: c[k][:, col] for k in kinds}


def assert_list(got, want, n, what, kinds=KINDS):
    for k in kinds:
        assert np.array_equal(got[k][:, :n], want[k]), "%s: %s differs at %r" % (what, k, np.argwhere(got[k][:, :n] != want[k])[:4].tolist())
        assert (got[k][:, n:] == SENT).all(), "%s: %s wrote into the padding" % (what, k)


def check_list(route, view, res, idx, ds, what, status=0):
    rc, st, got = gather(route, view, idx, ds)
    assert rc == 0, (what, route.panel.lib.brc_panel_last_error(route.panel.h))
    assert st == status, (what, st)
    assert_list(got, want_at(res, idx), len(idx), what)
    return got


def index_lists(P):
    """(name, list, dst_stride) of test 1"""
    run = list(range(0, 62 * 2, 2)) + [130] * 5 + list(range(131, 140))           # elements 62..66 hold one index
    return [("lead", [0], 1), ("last", [P - 1], 1), ("last, padded", [P - 1], 64), ("63", list(range(3, 66)), 63), ("64", list(range(3, 67)), 64),
            ("65", list(range(3, 68)), 65), ("257 x stride 5", list(range(3, 3 + 5 * 257, 5)), 257), ("one index three times", [777] * 3, 3),
            ("a run across the wave edge", run, len(run)), ("every index", list(range(P)), P), ("empty", [], 5)]


def status_lists(P):
    """(name, list, dst_stride, status) of test 4"""
    bad = [-1, 5, 6, P, 700, 2 ** 31 - 1]
    bad_sorted = sorted(bad)
    desc = list(range(10, 80)) + list(range(40, 300))
    return [("ascending", list(range(5, 500, 7)), 80, 0), ("out of range", bad_sorted, 9, OOR), ("out of range, unsorted", bad, 6, OOR | DESC),
            ("one descent", desc, len(desc) + 3, DESC)]


def third_allele_case(route, oracle_lib, opts, beg0, end):
    ref, arrs = td.third_allele_inputs()
    res, _ = td.oracle_result(oracle_lib, arrs, beg0, end, ref, **opts)
    eng = td.computed(route.knob_lib, arrs, beg0, end, ref, **opts)
    return res, eng


def hot_positions(res):
    """plane positions where at least three of the five base buckets (A C G T N) of some library are non-zero: with two slots per
    position, the third one's sums can only sit in an XAgg record"""
    nz = res.istat[:, 1:6, 0, :] != 0
    hot = np.nonzero((nz.sum(axis=1) >= 3).any(axis=0))[0]
    assert hot.size >= 1, "no position with three non-zero base buckets"
    return hot


def hot_lists(res):
    hot = hot_positions(res)
    near = np.unique(np.clip(np.concatenate([hot - 1, hot, hot + 1]), 0, res.n_pos - 1))
    cold = np.setdiff1d(np.arange(res.n_pos), hot)[:300]
    return [("hot once", hot.tolist()), ("hot twice", np.repeat(hot, 2).tolist()), ("hot with neighbours", near.tolist()), ("none hot", cold.tolist())]


# ------------------------------------------------------------------------------------------------ 1. index-list shapes

def test_index_lists_equal_the_oracle_columns(route, oracle_lib):
    ref, arrs = td.third_allele_inputs()
    res, _ = td.oracle_result(oracle_lib, arrs, 100, 1900, ref, **PER_LIB)
    eng = td.computed(route.engine_lib, arrs, 100, 1900, ref, **PER_LIB)
    v = eng.device_view()
    P = res.n_pos
    assert (v.n_lib, v.pos0, v.n_pos) == (2, res.pos0, P) and P > 3 + 5 * 257
    for name, idx, ds in index_lists(P):
        got = check_list(route, v, res, idx, ds, name)
        if name == "every index":         # ... which is the dense expansion of the whole region, byte for byte
            rc, dense = td.expand(route, v, 0, P, P)
            assert rc == 0
            for k in KINDS:
                assert got[k].tobytes() == dense[k].tobytes(), k
    # a subset of the destinations: the others are not needed, the wanted ones are the same
    idx = list(range(5, 105))
    rc, st, got = gather(route, v, idx, 100, kinds=("metrics", "depth"))
    assert rc == 0 and st == 0
    assert_list(got, want_at(res, idx), 100, "metrics and depth alone", kinds=("metrics", "depth"))
    # the verdict alone, and a call that wants nothing at all
    rc, st, _ = gather(route, v, idx, 100, kinds=())
    assert rc == 0 and st == 0
    assert gather(route, v, idx, 100, kinds=(), status=False)[0] == 0
    t = route.panel.last_timing()
    assert t["bytes_written"] == 0
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. third alleles

@pytest.mark.parametrize("opts", [dict(), dict(PER_LIB, min_bq=10)], ids=["all-lib", "per-lib"])
def test_third_allele_records_reach_their_listed_elements(route, oracle_lib, monkeypatch, opts):
    """The knob libraries under BRC_FORCE_DOM=3 + BRC_XEV_CAP=1 (as tests/test_dense.py): positions whose third base bucket sits in
    an XAgg record, listed once, twice, between their neighbours — and a list that holds none of them."""
    monkeypatch.setenv("BRC_FORCE_DOM", "3"); monkeypatch.setenv("BRC_XEV_CAP", "1")
    res, eng = third_allele_case(route, oracle_lib, opts, 0, 2000)
    v = eng.device_view()
    assert v.n_xagg > 0, "the view holds no third-allele record: the second launch was not reached"
    for name, idx in hot_lists(res):
        check_list(route, v, res, idx, len(idx), "%s %r" % (name, opts))
    eng.close()


# ------------------------------------------------------------------------------------------------ 3. a site-list region

def host_words(route, a):
    return np.ascontiguousarray(route.host(a)).view(np.uint32)


def check_sites(route, r, res, pos, site, what):
    from bam_readcount_amd import tensors
    n = len(pos)
    assert (r["n"], r["n_lib"], r["pos0"]) == (n, res.n_lib, res.pos0), what
    assert np.array_equal(route.host(r["pos"]), np.asarray(pos, np.int32)) and np.array_equal(route.host(r["site"]), np.asarray(site, np.int32)), what
    want = want_at(res, np.asarray(pos) - res.pos0)
    for k in KINDS:
        assert tuple(r[k].shape) == tensors.shapes(res.n_lib, n)[k][0], (what, k)
        assert np.array_equal(host_words(route, r[k]).reshape(want[k].shape), want[k]), (what, k)
    assert int(host_words(route, r["status"])[0]) == 0, what


def check_listed_indels(route, t, res, pos, what):
    pos = np.asarray(pos)
    recs = [d for d in res.indels if d["pos"] in set(pos.tolist())]
    want = ti.table_of(recs)
    m = len(recs)
    assert t["m"] == m, (what, t["m"], m)
    for k in capi.INDEL_DESTS:
        got = host_words(route, t[k]) if k != "alleles" else route.host(t[k])
        assert np.array_equal(got.reshape(want[k].shape), want[k]), (what, k)
    assert np.array_equal(route.host(t["j"]), np.searchsorted(pos, [d["pos"] for d in recs]).astype(np.int32)), what
    return m


def test_sites_of_announced_windows_equal_the_unhinted_oracle(route, oracle_lib, twolib):
    """Engine.region_windows + tensors.sites(windows=...): one-position windows, a 70-position one over a tile edge, adjacent and
    repeated ones; the indel records at the listed positions with them."""
    from bam_readcount_amd import tensors
    ref, arrs = td.third_allele_inputs()
    res, _ = td.oracle_result(oracle_lib, arrs, 100, 1900, ref, **PER_LIB)
    with_indel = sorted({d["pos"] for d in res.indels if 1000 <= d["pos"] < 1400})[:3]
    assert with_indel, "no indel between 1000 and 1400"
    wins = sorted([(150, 151), (151, 152), (300, 301), (640, 710), (900, 901), (900, 901), (1500, 1501), (1899, 1900)] + [(p, p + 1) for p in with_indel])
    b = np.array([w[0] for w in wins], np.int32); e = np.array([w[1] for w in wins], np.int32)
    eng = capi.Engine(route.engine_lib, **PER_LIB)
    eng.begin_region(0, 100, 1900, ref)
    eng.push_reads(capi.select_reads(arrs, capi.fetch_overlapping(arrs, capi.read_ends(arrs), 99, 1900)))
    eng.region_windows(b, e)
    eng.upload(); eng.compute()
    pos = np.concatenate([np.arange(x, y) for x, y in wins]); site = np.concatenate([np.full(y - x, i) for i, (x, y) in enumerate(wins)])
    r = tensors.sites(eng, route.panel, windows=(b, e), want=tensors.KINDS, indels=route.indels)
    check_sites(route, r, res, pos, site, "announced windows")
    assert check_listed_indels(route, r["indels"], res, pos, "announced windows") >= len(with_indel)
    eng.close()
    # the golden two-library fixture at the positions of its site list ("contig first last", 1-based, inclusive)
    names = [str(s) for s in twolib["lib_names"]]
    opts = dict(lib_names=names, per_lib=True, insertion_centric=True, ref_len_check=True)
    end = int(twolib["ref"].size)
    res, _ = td.oracle_result(oracle_lib, twolib, 0, end, twolib["ref"], **opts)
    pos = np.concatenate([np.arange(int(f[1]) - 1, int(f[2])) for f in (l.split() for l in open(os.path.join(GOLDEN, "twolib_site_list.txt")) if l.strip())])
    assert pos.size == 11
    eng = td.computed(route.engine_lib, twolib, 0, end, twolib["ref"], **opts)
    r = tensors.sites(eng, route.panel, positions=pos, want=tensors.KINDS, indels=route.indels)
    check_sites(route, r, res, pos, np.arange(pos.size), "twolib")
    check_listed_indels(route, r["indels"], res, pos, "twolib")
    eng.close()


# ------------------------------------------------------------------------------------------------ 4. the status word

def test_status_word_and_what_is_written_for_bad_lists(route, oracle_lib, monkeypatch):
    """The bounds contract: an index outside the planes reads nothing and is written as an empty position; a descent leaves ncol /
    depth / unavail and every bucket without a record exact, and a bucket with a record at one of its two permitted values.  (The
    same lists run under the host sanitizers in test_lists_under_the_host_sanitizers.)"""
    monkeypatch.setenv("BRC_FORCE_DOM", "3"); monkeypatch.setenv("BRC_XEV_CAP", "1")
    res, eng = third_allele_case(route, oracle_lib, PER_LIB, 100, 1900)
    v = eng.device_view()
    P = res.n_pos
    assert v.n_xagg > 0
    for name, idx, ds, status in status_lists(P):
        rc, st, got = gather(route, v, idx, ds)
        assert rc == 0 and st == status, (name, rc, st)
        n = len(idx)
        want = want_at(res, idx)
        if not status & DESC:
            assert_list(got, want, n, name)
            continue
        # the slots' values of the bucket a record overwrites: the dense expansion with the records taken out of the view
        bare = capi.DeviceView.from_buffer_copy(v); bare.n_xagg = 0
        rc, _, slots = gather(route, bare, idx, ds)
        assert rc == 0
        for k in KINDS:
            exact = got[k][:, :n] == want[k]
            if k in ("ncol", "depth", "unavail"):
                assert exact.all(), (name, k)
            else:
                f = {"istat": 9, "fstat": 4, "metrics": 13}[k]
                ok = (exact | (got[k][:, :n] == slots[k][:, :n])).reshape(-1, f, n).all(axis=1)            # per (library, bucket, element)
                assert ok.all(), (name, k)
                differs = ~(slots[k][:, :n] == want[k]).reshape(-1, f, n).all(axis=1)                      # buckets that have a record
                assert ((got[k][:, :n] == want[k]).reshape(-1, f, n).all(axis=1) | differs).all(), (name, k)
                assert differs.any() or name != "one descent", "the descending list meets no bucket with a record"
            assert (got[k][:, n:] == SENT).all(), (name, k)
    eng.close()


# ------------------------------------------------------------------------------------------------ 5. the host sanitizers

def _serialize(v, lists):
    """the host view of a sim engine and the lists as panel_check.cpp reads them"""
    b = td._serialize_view(v, [])
    b = b[:36] + struct.pack("<i", len(lists)) + b[40:]
    for idx, ds in lists:
        b += struct.pack("<qq", len(idx), ds) + np.asarray(idx, np.int32).tobytes()
    return b


def test_lists_under_the_host_sanitizers(oracle_lib, sim_lib, tmp_path, monkeypatch):
    """The lists of tests 1, 2 and 4 on the CPU build with -fsanitize=address,undefined: sources of exactly the view's sizes, lists of
    exactly n indices, destinations of exactly (planes - 1) * dst_stride + n elements — a load or store outside them is a report —
    and whatever the contract promises about the results holds."""
    checker = side.sim_checker(side.SIDE["panel"])
    monkeypatch.setenv("BRC_FORCE_DOM", "3"); monkeypatch.setenv("BRC_XEV_CAP", "1")
    ref, arrs = td.third_allele_inputs()
    res, _ = td.oracle_result(oracle_lib, arrs, 100, 1900, ref, **PER_LIB)
    eng = td.computed(sim_lib, arrs, 100, 1900, ref, **PER_LIB)
    v = eng.device_view()
    assert v.memory == capi.MEM_HOST and v.n_xagg > 0
    P = res.n_pos
    lists = [(idx, ds, 0) for _, idx, ds in index_lists(P)] + [(idx, len(idx), 0) for _, idx in hot_lists(res)] + [(idx, ds, st) for _, idx, ds, st in status_lists(P)]
    open(tmp_path / "case.bin", "wb").write(_serialize(v, [(idx, ds) for idx, ds, _ in lists]))
    eng.close()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([checker, str(tmp_path / "case.bin"), str(tmp_path / "res.bin")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    assert p.stdout.decode().strip() == "%d lists" % len(lists)
    d = np.fromfile(tmp_path / "res.bin", np.uint32); o = 0
    L = res.n_lib
    for idx, ds, status in lists:
        n = len(idx)
        assert d[o].view(np.int32) == 0 and d[o + 1] == status, (idx[:8], d[o + 1]); o += 2
        want = want_at(res, idx)
        for k in KINDS:
            pl = planes_of(k, L)
            elems = (pl - 1) * ds + n if n else 0
            flat = np.full(pl * ds, SENT, np.uint32); flat[:elems] = d[o:o + elems]; o += elems
            got = flat.reshape(pl, ds)
            if not status & DESC or k in ("ncol", "depth", "unavail"):
                assert np.array_equal(got[:, :n], want[k]), (k, idx[:8], ds)
            assert (got[:, n:] == SENT).all(), (k, idx[:8], ds)
    assert o == d.size


# ------------------------------------------------------------------------------------------------ 6. refusals

def test_refused_calls_write_nothing(route, test_bam):
    beg0, end = 10403000, 10403500
    eng = td.computed(route.engine_lib, test_bam, beg0, end, test_bam["ref"], tid=20)
    v = eng.device_view()
    P = int(v.n_pos)
    assert P >= 100

    def altered(**kw):
        w = capi.DeviceView.from_buffer_copy(v)
        for k, x in kw.items():
            setattr(w, k, x)
        return w
    other = capi.MEM_HOST if route.mem == capi.MEM_DEVICE else capi.MEM_DEVICE
    idx = list(range(10))
    W = 6 * 13 * 16                       # words of every buffer: the largest destination of an accepted (n = 10, dst_stride = 16) call
    cases = [("no handle", dict(view=v, handle=False)), ("no view", dict(view=None)), ("no list", dict(view=v, no_idx=True)), ("n < 0", dict(view=v, n=-1)),
             ("dst_stride < n", dict(view=v, ds=9)), ("memory of the other kind", dict(view=altered(memory=other))), ("memory 0", dict(view=altered(memory=0))),
             ("another device", dict(view=altered(device=int(v.device) + 1))), ("a view without planes", dict(view=altered(si=None))),
             ("a view without planes (slotid)", dict(view=altered(slotid=None))), ("not a view", dict(view=capi.DeviceView())),
             ("too large for one launch", dict(view=v, n=(2 ** 31 - 1) * 256 + 1, ds=2 ** 40))]
    for what, kw in cases:
        kw = dict(dict(ds=16, words=W), **kw)
        view = kw.pop("view")
        rc, st, got = gather(route, view, idx, **kw)
        assert rc == capi.E_ARG, what
        assert st == SENT, "%s: the status word was written" % what
        for k in KINDS:
            assert (got[k] == SENT).all(), "%s: %s was written" % (what, k)
        if kw.get("handle", True):
            assert route.panel.lib.brc_panel_last_error(route.panel.h), what
    # n == 0 is fine and writes no destination (the status word of an empty list is 0); so is a call that wants nothing
    rc, st, got = gather(route, v, [], 16)
    assert rc == 0 and st == 0 and all((got[k] == SENT).all() for k in KINDS)
    assert gather(route, v, [], 0, kinds=(), status=False, no_idx=True)[0] == 0
    assert route.panel.lib.brc_panel_last_error(route.panel.h) == b""
    eng.close()


# ------------------------------------------------------------------------------------------------ 7. tensors.sites

def test_tensors_sites_arguments(route, oracle_lib):
    from bam_readcount_amd import tensors
    ref, arrs = td.third_allele_inputs()
    res, _ = td.oracle_result(oracle_lib, arrs, 100, 1900, ref, **PER_LIB)
    eng = td.computed(route.engine_lib, arrs, 100, 1900, ref, **PER_LIB)
    pos = [res.pos0, res.pos0 + 7, res.pos0 + 7, res.pos0 + 64, res.pos0 + 65, res.pos0 + res.n_pos - 1]
    forms = [pos, np.array(pos, np.int64)]
    if route.name == "hip":
        forms.append(route.torch.tensor(pos, dtype=route.torch.int32, device="cuda"))
    rs = [tensors.sites(eng, route.panel, positions=p, want=tensors.KINDS) for p in forms] + [tensors.sites(eng, route.panel, positions=pos, want=tensors.KINDS)]
    for r in rs:
        check_sites(route, r, res, pos, np.arange(len(pos)), "positions")
        if route.name == "sim":
            assert all(isinstance(r[k], np.ndarray) for k in tensors.KINDS + ("pos", "site", "status"))
        else:
            assert all(r[k].is_cuda for k in tensors.KINDS + ("pos", "site", "status"))
        for k in tensors.KINDS:                      # every form, and a second call: byte-identical
            assert host_words(route, r[k]).tobytes() == host_words(route, rs[0][k]).tobytes(), k
    d = tensors.sites(eng, route.panel, positions=pos)
    assert set(tensors.DEFAULT_WANT) <= set(d) and "unavail" not in d and "indels" not in d
    # out: filled in place
    again = tensors.sites(eng, route.panel, positions=pos, want=("metrics",), out={"metrics": d["metrics"]})
    assert again["metrics"] is d["metrics"]
    with pytest.raises(ValueError):
        tensors.sites(eng, route.panel, positions=pos[:-1], want=("metrics",), out={"metrics": d["metrics"]})       # wrong shape
    # an empty list
    e = tensors.sites(eng, route.panel, positions=[], want=("depth",), indels=route.indels)
    assert e["n"] == 0 and tuple(e["depth"].shape) == (2, 0) and e["indels"]["m"] == 0
    # host lists are checked before anything is queued
    untouched = route.sentinel_words(2 * len(pos))
    keep = untouched.view(route.torch.uint32).view(2, len(pos)) if route.name == "hip" else untouched.reshape(2, len(pos))
    for bad in (dict(positions=pos[::-1]), dict(positions=[res.pos0 - 1] + pos[1:]), dict(positions=pos[:-1] + [res.pos0 + res.n_pos]),
                dict(windows=(np.array([300, 200], np.int32), np.array([301, 204], np.int32))), dict(windows=(np.array([300], np.int32), np.array([299], np.int32))),
                dict(windows=(np.array([1895], np.int32), np.array([1901], np.int32))), dict(), dict(positions=pos, windows=(np.array([300]), np.array([301])))):
        with pytest.raises(ValueError):
            tensors.sites(eng, route.panel, want=("depth",), out={"depth": keep}, **bad)
    with pytest.raises(ValueError):
        tensors.sites(eng, route.panel, positions=pos, want=("nonsense",))
    assert (route.words(untouched) == SENT).all()
    eng.close()


def test_sites_work_on_text_only_engines_and_after_a_fetch(route, oracle_lib, test_bam):
    from bam_readcount_amd import tensors
    beg0, end = 10403000, 10403700
    res, text = td.oracle_result(oracle_lib, test_bam, beg0, end, test_bam["ref"], tid=20, chrom="21")
    assert res.n_pos > 201
    pos = (res.pos0 + np.array([0, 1, 63, 64, 65, 200, 200, res.n_pos - 1])).tolist()
    for opts in (dict(text_only=True), dict(device_text="21")):
        eng = td.computed(route.engine_lib, test_bam, beg0, end, test_bam["ref"], tid=20, **opts)
        check_sites(route, tensors.sites(eng, route.panel, positions=pos, want=tensors.KINDS), res, pos, np.arange(len(pos)), "before fetch %r" % opts)
        eng.fetch_result()
        assert eng.format_region("21") == text
        check_sites(route, tensors.sites(eng, route.panel, positions=pos, want=tensors.KINDS), res, pos, np.arange(len(pos)), "after fetch %r" % opts)
        eng.close()
