"""Device-resident results (include/brc_dense.h): brc_device_view_get + brc_dense_expand against the ORACLE's dense brc_result — integers
equal, floats equal as uint32 bit patterns — and the thirteen metric columns against numpy's fp32 division on the oracle's planes
and against the text the oracle prints.

Every body runs twice (the `route` fixture): [sim] = libbrc_sim.so + tests/sim_dense/libbrc_dense_sim.so, host memory, in the CPU
suite; [hip] = the product's libraries on the GPU (gpu-marked), destinations in device memory allocated through torch.  The knob
test drives the libraries of conftest's knob_lib.  The host sanitizers run the CPU build over the window list."""
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

KINDS = ("ncol", "depth", "unavail", "istat", "fstat", "metrics")


def planes_of(kind, L):
    return {"ncol": L, "depth": L, "unavail": 1, "istat": L * 6 * 9, "fstat": L * 6 * 4, "metrics": L * 6 * 13}[kind]


@pytest.fixture(scope="module", params=["sim", pytest.param("hip", marks=pytest.mark.gpu)])
def route(request):
    return Route(request.param, ("dense",), engine=True)


def expand(route, view, k0, n, ds, kinds=KINDS):
    """brc_dense_expand into sentinel-filled buffers of [planes][ds]; returns (rc, {kind: uint32 words [planes, ds]})"""
    L = int(view.n_lib) if view is not None and view.n_lib > 0 else 1
    bufs = {k: route.sentinel_words(planes_of(k, L) * max(ds, 0)) for k in kinds}
    rc = route.dense.expand_raw(view, k0, n, ds, **{k: route.ptr(b) for k, b in bufs.items()})
    out = {}
    for k, b in bufs.items():
        w = route.words(b)
        out[k] = w[:planes_of(k, L) * max(ds, 0)].reshape(planes_of(k, L), max(ds, 0)) if ds > 0 else w[:0].reshape(planes_of(k, L), 0)
    return rc, out


def computed(lib, arrs, beg0, end, ref, tid=0, **opts):
    """an engine of `lib` holding the computed region [beg0, end) (reads fetched the reference's way)"""
    eng = capi.Engine(lib, **opts)
    idx = capi.fetch_overlapping(arrs, capi.read_ends(arrs), beg0 - 1, end)
    eng.begin_region(tid, beg0, end, ref)
    eng.push_reads(capi.select_reads(arrs, idx))
    eng.upload(); eng.compute()
    return eng


def oracle_result(oracle_lib, arrs, beg0, end, ref, tid=0, chrom="chrS", **opts):
    eng = capi.Engine(oracle_lib, **opts)
    idx = capi.fetch_overlapping(arrs, capi.read_ends(arrs), beg0 - 1, end)
    eng.begin_region(tid, beg0, end, ref)
    eng.push_reads(capi.select_reads(arrs, idx))
    res = eng.end_region()
    text = eng.format_region(chrom)
    eng.close()
    return res, text


def metrics_of(istat, fstat):
    """The thirteen printed columns (BasicStat.cpp:117-140) from dense planes [L][6][9|4][P], by numpy's fp32 division of the sums
    converted with astype(np.float32)."""
    i = istat.astype(np.float32); f = fstat
    c = i[:, :, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        nq2 = i[:, :, 5]
        cols = [c, i[:, :, 1] / c, i[:, :, 8] / c, i[:, :, 2] / c, i[:, :, 3], i[:, :, 4], f[:, :, 0] / c, f[:, :, 2] / c, i[:, :, 6] / c,
                nq2, np.where(istat[:, :, 5] > 0, f[:, :, 1] / nq2, np.float32(0)), i[:, :, 7] / c, f[:, :, 3] / c]
    m = np.stack([np.asarray(x, np.float32) for x in cols], axis=2)
    m[np.broadcast_to((istat[:, :, 0] == 0)[:, :, None, :], m.shape)] = 0
    assert m.dtype == np.float32
    return m


def want_planes(res, k0, n):
    """{kind: uint32 words [planes, n]} of the oracle's result for the window"""
    L = res.n_lib
    un = res.unavail if res.unavail is not None else np.full(res.n_pos, 0xFFFFFFFF, np.uint32)
    d = {"ncol": res.ncol, "depth": res.depth, "unavail": un[None, :], "istat": res.istat, "fstat": res.fstat.view(np.uint32),
         "metrics": metrics_of(res.istat, res.fstat).view(np.uint32)}
    return {k: np.ascontiguousarray(v.reshape(planes_of(k, L), res.n_pos)[:, k0:k0 + n]) for k, v in d.items()}


def assert_window(got, want, n, ds, what):
    for k in KINDS:
        assert np.array_equal(got[k][:, :n], want[k]), "%s: %s differs at %r" % (what, k, np.argwhere(got[k][:, :n] != want[k])[:4].tolist())
        assert (got[k][:, n:] == SENT).all(), "%s: %s wrote into the padding" % (what, k)


def check_whole(route, eng, res, what):
    v = eng.device_view()
    assert v.memory == route.mem
    assert (v.n_lib, v.pos0, v.n_pos) == (res.n_lib, res.pos0, res.n_pos) and v.stride >= v.n_pos, what
    rc, got = expand(route, v, 0, res.n_pos, res.n_pos)
    assert rc == 0, route.dense.lib.brc_dense_last_error(route.dense.h)
    assert_window(got, want_planes(res, 0, res.n_pos), res.n_pos, res.n_pos, what)
    return v, got


# ------------------------------------------------------------------------------------------------ 1. fixtures

def test_fixture_all_lib_whole_region_equals_oracle(route, oracle_lib, test_bam):
    beg0, end = 10402736, 10405248
    for ic in (False, True):
        opts = dict(insertion_centric=ic)
        res, _ = oracle_result(oracle_lib, test_bam, beg0, end, test_bam["ref"], tid=20, **opts)
        assert res.n_pos > 2000 and res.istat[:, :, 0].sum() > 90000
        eng = computed(route.engine_lib, test_bam, beg0, end, test_bam["ref"], tid=20, **opts)
        check_whole(route, eng, res, "test_bam ic=%d" % ic)
        eng.close()


def test_fixture_per_lib_whole_region_equals_oracle(route, oracle_lib, twolib):
    names = [str(s) for s in twolib["lib_names"]]
    opts = dict(lib_names=names, per_lib=True, insertion_centric=True, ref_len_check=True)
    end = int(twolib["ref"].size)
    res, _ = oracle_result(oracle_lib, twolib, 0, end, twolib["ref"], **opts)
    assert res.n_lib > 1 and res.n_pos > 100 and res.unavail is not None
    eng = computed(route.engine_lib, twolib, 0, end, twolib["ref"], **opts)
    v, _ = check_whole(route, eng, res, "twolib")
    assert v.unavail
    eng.close()


def test_view_works_on_text_only_engines_and_after_a_fetch(route, oracle_lib, test_bam):
    """brc_device_view_get with BRC_OPT_TEXT_ONLY (and device text), before and after brc_fetch_result: the same planes."""
    beg0, end = 10403000, 10403700
    res, text = oracle_result(oracle_lib, test_bam, beg0, end, test_bam["ref"], tid=20, chrom="21")
    for opts in (dict(text_only=True), dict(device_text="21")):
        eng = computed(route.engine_lib, test_bam, beg0, end, test_bam["ref"], tid=20, **opts)
        check_whole(route, eng, res, "before fetch %r" % opts)
        eng.fetch_result()
        assert eng.format_region("21") == text
        check_whole(route, eng, res, "after fetch %r" % opts)
        eng.close()


# ------------------------------------------------------------------------------------------------ 2. third alleles

def third_allele_inputs():
    rng = np.random.default_rng(7)
    ref = synth.make_ref(rng, 2000, weird=0.01)
    arrs = synth.make_batch(1207, ref, 1500, read_len=(80, 140), style="mixed", n_libs=2, mismatch=0.15, p_iupac_read=0.02)
    return ref, arrs


def test_third_alleles_and_n_bases_reach_the_record_launch(route, oracle_lib, monkeypatch):
    """A deep batch with mismatches and N bases, every lane forced to treat bucket 3 as dominant and third-allele lists of one entry
    (grow and compute again): buckets whose sums sit in the XAgg table — the second launch — must come out as the oracle's."""
    monkeypatch.setenv("BRC_FORCE_DOM", "3"); monkeypatch.setenv("BRC_XEV_CAP", "1")
    ref, arrs = third_allele_inputs()
    for opts in (dict(), dict(lib_names=["libA", "libB"], per_lib=True, min_bq=10)):
        res, _ = oracle_result(oracle_lib, arrs, 0, 2000, ref, **opts)
        nz = res.istat[:, 1:5, 0, :] != 0                        # A C G T buckets with reads
        assert (nz.sum(axis=1) >= 3).any(), "no position with three non-zero base buckets"
        assert (res.istat[:, 5, 0, :] != 0).any(), "no position with a non-zero N bucket"
        eng = computed(route.knob_lib, arrs, 0, 2000, ref, **opts)
        v, _ = check_whole(route, eng, res, "third alleles %r" % (opts,))
        assert v.n_xagg > 0, "the view holds no third-allele record: the second launch was not reached"
        eng.close()


# ------------------------------------------------------------------------------------------------ 3. windows

def window_list(P):
    """(k0, n, dst_stride): k0 and n not multiples of 64, n = 1, the last position, strides above n, a tile-aligned one, n = 0"""
    return [(0, P, P), (3, 61, 61), (63, 130, 200), (64, 64, 64), (65, 1, 1), (65, 1, 7), (P - 1, 1, 1), (P - 1, 1, 64), (P - 77, 77, 100),
            (130, P - 130, P), (17, 0, 5)]


def test_windows_equal_the_slices_of_the_whole_region(route, oracle_lib):
    ref, arrs = third_allele_inputs()
    opts = dict(lib_names=["libA", "libB"], per_lib=True)
    res, _ = oracle_result(oracle_lib, arrs, 100, 1900, ref, **opts)
    eng = computed(route.engine_lib, arrs, 100, 1900, ref, **opts)
    v, whole = check_whole(route, eng, res, "whole")
    P = res.n_pos
    assert P > 300
    for k0, n, ds in window_list(P):
        rc, got = expand(route, v, k0, n, ds)
        assert rc == 0, (k0, n, ds)
        assert_window(got, {k: whole[k][:, k0:k0 + n] for k in KINDS}, n, ds, "window %r" % ((k0, n, ds),))
    # a subset of the destinations: the others are not needed, the wanted ones are the same
    rc, got = expand(route, v, 5, 100, 128, kinds=("metrics", "depth"))
    assert rc == 0
    for k in ("metrics", "depth"):
        assert np.array_equal(got[k][:, :100], whole[k][:, 5:105]) and (got[k][:, 100:] == SENT).all()
    eng.close()


def _serialize_view(v, windows):
    """the host view of a sim engine as dense_check.cpp reads it"""
    L, PS, nx = int(v.n_lib), int(v.stride), int(v.n_xagg)

    def words(p, n):
        return bytes(np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), shape=(n,))) if n else b""
    b = struct.pack("<iiqqQii", L, v.pos0, v.n_pos, PS, nx, 1 if v.unavail else 0, len(windows))
    b += words(v.ncol, L * PS) + words(v.depth, L * PS) + words(v.slotid, L * PS) + words(v.si, L * 18 * PS) + words(v.sf, L * 8 * PS)
    if v.unavail:
        b += words(v.unavail, PS)
    b += words(v.xagg, nx * 16)
    for w in windows:
        b += struct.pack("<qqq", *w)
    return b


def test_windows_under_the_host_sanitizers(oracle_lib, sim_lib, tmp_path):
    """The window list on the CPU build with -fsanitize=address,undefined: sources of exactly the view's sizes, destinations of
    exactly (planes - 1) * dst_stride + n elements — a load or store outside them is a report — and the results are the oracle's."""
    checker = side.sim_checker(side.SIDE["dense"])
    ref, arrs = third_allele_inputs()
    opts = dict(lib_names=["libA", "libB"], per_lib=True)
    res, _ = oracle_result(oracle_lib, arrs, 100, 1900, ref, **opts)
    eng = computed(sim_lib, arrs, 100, 1900, ref, **opts)
    v = eng.device_view()
    assert v.memory == capi.MEM_HOST and v.n_xagg > 0
    wins = window_list(res.n_pos)
    open(tmp_path / "case.bin", "wb").write(_serialize_view(v, wins))
    eng.close()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([checker, str(tmp_path / "case.bin"), str(tmp_path / "res.bin")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    assert p.stdout.decode().strip() == "%d windows" % len(wins)
    d = np.fromfile(tmp_path / "res.bin", np.uint32); o = 0
    L = res.n_lib
    for k0, n, ds in wins:
        assert d[o].view(np.int32) == 0; o += 1
        want = want_planes(res, k0, n)
        for k in KINDS:
            pl = planes_of(k, L)
            elems = (pl - 1) * ds + n if n else 0
            flat = np.full(pl * ds, SENT, np.uint32); flat[:elems] = d[o:o + elems]; o += elems
            got = flat.reshape(pl, ds)
            assert np.array_equal(got[:, :n], want[k]), (k, k0, n, ds)
            assert (got[:, n:] == SENT).all(), (k, k0, n, ds)
    assert o == d.size


# ------------------------------------------------------------------------------------------------ 4. metrics

def test_metrics_print_as_the_oracle_text(route, oracle_lib, test_bam):
    """'%.2f' of every metric of every printed bucket == the field of the line the oracle prints (all-lib mode: six base buckets per
    line; indel entries are not part of the tensor); the integer columns print as integers."""
    beg0, end = 10402736, 10405248
    res, text = oracle_result(oracle_lib, test_bam, beg0, end, test_bam["ref"], tid=20, chrom="21")
    eng = computed(route.engine_lib, test_bam, beg0, end, test_bam["ref"], tid=20)
    v, got = check_whole(route, eng, res, "test_bam")          # (includes: metrics bit-equal to numpy's fp32 division on the oracle's planes)
    eng.close()
    m = got["metrics"].view(np.float32).reshape(1, 6, 13, res.n_pos)
    lines = text.decode().splitlines()
    assert len(lines) == 796
    n_fields = 0
    for line in lines:
        cols = line.split("\t")
        k = int(cols[1]) - 1 - res.pos0
        seen = set()
        for entry in cols[4:]:
            f = entry.split(":")
            if f[0][0] in "+-":
                continue
            b = "=ACGTN".index(f[0]); seen.add(b)
            assert len(f) == 14
            for c in range(13):
                x = m[0, b, c, k]
                mine = "%d" % int(x) if c in (0, 4, 5, 9) else "%.2f" % float(x)
                assert mine == f[1 + c], (line, f[0], c, mine)
                n_fields += 1
        assert seen == set(range(6)), line
    assert n_fields == 796 * 6 * 13


# ------------------------------------------------------------------------------------------------ 5. arguments

def test_refused_calls_write_nothing(route, test_bam):
    beg0, end = 10403000, 10403500
    eng = capi.Engine(route.engine_lib)
    idx = capi.fetch_overlapping(test_bam, capi.read_ends(test_bam), beg0 - 1, end)
    eng.begin_region(20, beg0, end, test_bam["ref"]); eng.push_reads(capi.select_reads(test_bam, idx)); eng.upload()
    # before a compute: BRC_E_ARG, and the struct the caller handed in is no view
    early = capi.DeviceView()
    assert route.engine_lib.lib.brc_device_view_get(eng.h, C.byref(early)) == capi.E_ARG
    with pytest.raises(capi.BrcError):
        eng.device_view()
    eng.compute()
    v = eng.device_view()
    P = int(v.n_pos)
    assert P >= 100

    def altered(**kw):
        w = capi.DeviceView.from_buffer_copy(v)
        for k, x in kw.items():
            setattr(w, k, x)
        return w
    other = capi.MEM_HOST if route.mem == capi.MEM_DEVICE else capi.MEM_DEVICE
    cases = [("no view", None, 0, 10, 16), ("a view taken before compute", early, 0, 10, 16), ("k0 < 0", v, -1, 10, 16), ("n < 0", v, 0, -1, 16),
             ("k0 + n > n_pos", v, P - 5, 6, 16), ("k0 beyond the planes", v, P + 1, 0, 16), ("n > n_pos", v, 0, P + 1, P + 1),
             ("dst_stride < n", v, 0, 10, 9), ("memory of the other kind", altered(memory=other), 0, 10, 16),
             ("memory 0", altered(memory=0), 0, 10, 16), ("another device", altered(device=int(v.device) + 1), 0, 10, 16)]
    if route.name == "hip":
        assert other == capi.MEM_HOST          # (a BRC_MEM_HOST view handed to the hip library is in the list)
    for what, view, k0, n, ds in cases:
        rc, got = expand(route, view, k0, n, ds)
        assert rc == capi.E_ARG, what
        for k in KINDS:
            assert (got[k] == SENT).all(), "%s: %s was written" % (what, k)
    # n == 0 is fine and writes nothing; so is a call that wants nothing
    rc, got = expand(route, v, 7, 0, 16)
    assert rc == 0 and all((got[k] == SENT).all() for k in KINDS)
    assert route.dense.expand_raw(v, 0, 10, 16) == 0
    assert route.dense.expand_raw(v, P, 0, 0) == 0
    assert route.dense.lib.brc_dense_expand(None, C.byref(v), 0, 0, 0, None, None, None, None, None, None, None) == capi.E_ARG
    eng.close()


# ------------------------------------------------------------------------------------------------ the Python interface, CPU route

def test_tensors_region_windows_and_out(route, oracle_lib):
    """bam_readcount_amd.tensors.region: shapes without padding, windows in reference coordinates, `out` reused; ([hip]: the same
    body returns CUDA tensors, compared through .cpu())"""
    from bam_readcount_amd import tensors
    ref, arrs = third_allele_inputs()
    opts = dict(lib_names=["libA", "libB"], per_lib=True)
    res, _ = oracle_result(oracle_lib, arrs, 100, 1900, ref, **opts)
    eng = computed(route.engine_lib, arrs, 100, 1900, ref, **opts)

    def host(a):
        return a.cpu().numpy() if route.name == "hip" else a
    r = tensors.region(eng, route.dense, want=tensors.KINDS)
    assert (r["pos0"], r["first"], r["n"], r["n_lib"]) == (res.pos0, res.pos0, res.n_pos, 2)
    if route.name == "sim":
        assert all(isinstance(r[k], np.ndarray) for k in tensors.KINDS)
    else:
        assert all(r[k].is_cuda for k in tensors.KINDS)
    want = want_planes(res, 0, res.n_pos)
    for k in tensors.KINDS:
        assert tuple(r[k].shape) == tensors.shapes(2, res.n_pos)[k][0]
        assert np.array_equal(host(r[k]).view(np.uint32).reshape(want[k].shape), want[k]), k
    # a window in reference coordinates, clipped to the planes; default kinds
    w = tensors.region(eng, route.dense, beg0=res.pos0 + 70, end=res.pos0 + 201)
    assert (w["first"], w["n"]) == (res.pos0 + 70, 131) and set(tensors.DEFAULT_WANT) <= set(w) and "unavail" not in w
    for k in tensors.DEFAULT_WANT:
        assert np.array_equal(host(w[k]), host(r[k])[..., 70:201]), k
    c = tensors.region(eng, route.dense, beg0=0, end=10 ** 9, want=("depth",))
    assert c["n"] == res.n_pos and np.array_equal(host(c["depth"]), res.depth)
    e = tensors.region(eng, route.dense, beg0=res.pos0 + res.n_pos + 5, want=("depth",))
    assert e["n"] == 0 and tuple(e["depth"].shape) == (2, 0)
    # out: filled in place
    again = tensors.region(eng, route.dense, beg0=res.pos0 + 70, end=res.pos0 + 201, want=("metrics",), out={"metrics": w["metrics"]})
    assert again["metrics"] is w["metrics"]
    with pytest.raises(ValueError):
        tensors.region(eng, route.dense, want=("metrics",), out={"metrics": w["metrics"]})       # wrong shape
    with pytest.raises(ValueError):
        tensors.region(eng, route.dense, want=("nonsense",))
    eng.close()
