"""Device-side candidate filter (include/brc_vet.h): brc_vet_sites and bam_readcount_amd.tensors.vet against the header's predicate
written in numpy float32 / uint64 over the ORACLE's dense brc_result (istat, fstat, depth, refbase; the thirteen columns by numpy's fp32
division, test_dense.metrics_of) — fail, keep and vals equal as bit patterns, no tolerance.

Every body runs twice (the `route` fixture): [sim] = libbrc_sim.so + tests/sim_vet/libbrc_vet_sim.so, host memory, in the CPU suite;
[hip] = the product's libraries on the GPU (gpu-marked), lists, destinations and scratch in device memory allocated through torch.
Destinations are filled with 0xA5A5A5A5 first and are PAD elements wider than needed: elements [n, dst_stride) and every destination
that was not asked for must keep it.  The scratch has exactly brc_vet_workspace bytes.

Where no engine can produce the shape — a metric one ulp from its threshold, a difference that a fused or double-precision evaluation
decides otherwise, counts next to 2^32, 254 libraries, reference characters and slices of every kind, a bucket that lives in a record
of a given element — the views are built by hand (`full_views`: test_select.build_views with all thirteen sums per bucket) in the
route's memory, and the reference is the same numpy predicate over the dense sums given.

Sizes that matter to the kernels (brc_vet.hip): a wave is 64 consecutive list elements, a workgroup 256."""
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

LIBS = ("dense", "select", "vet")
PAD = 3
NVAL = capi.VET_NVAL
ALL = ("fail", "keep", "vals")
BIT = capi.VET_BIT
NOT_ASKED, NO_SITE = capi.VET_NOT_ASKED, capi.VET_NO_SITE
PER_LIB = ts.PER_LIB
F32 = np.float32
U64 = np.uint64
# columns of the thirteen (include/brc_dense.h) behind the six tested ones, in vals' order: AVG_POS, AVG_3P, AVG_BQ, AVG_MAPQ, AVG_MMQ, AVG_CLIPPED
MCOL = (6, 12, 2, 1, 8, 11)
# thresholds that judge nothing: every test passes on any finite data
OPEN = dict(min_depth=0, min_var_count=0, freq_num=0, freq_den=1, min_strand_reads=0, strand_num=0, strand_den=1, min_ref_reads=0,
            min_var_readpos=-3e38, min_var_dist3=-3e38, min_var_bq=-3e38, min_var_mapq=-3e38, max_var_mmqs=3e38, min_var_rl=-3e38,
            min_ref_readpos=-3e38, min_ref_dist3=-3e38, min_ref_bq=-3e38, min_ref_mapq=-3e38, min_ref_rl=-3e38, max_mmqs_diff=3e38,
            max_mapq_diff=3e38, max_rl_diff=3e38)


def T_(**kw):
    return dict(OPEN, **kw)


@pytest.fixture(scope="module", params=["sim", pytest.param("hip", marks=pytest.mark.gpu)])
def route(request):
    return Route(request.param, LIBS, engine=True)


@pytest.fixture(scope="module")
def sim_route():
    return Route("sim", LIBS, engine=True)


# ------------------------------------------------------------------------------------------------ the reference predicate

class Dense:
    """what the reference predicate reads: depth [L, P], istat [L, 6, 9, P], fstat [L, 6, 4, P], refbase (P characters), and the thirteen
    columns of every bucket by numpy's fp32 division, computed once"""

    def __init__(self, depth, istat, fstat, refbase, pos0):
        self.depth, self.istat, self.fstat, self.refbase, self.pos0 = np.asarray(depth, np.uint32), istat, fstat, bytes(refbase), pos0
        self.n_lib, self.n_pos = self.depth.shape
        self.metrics = td.metrics_of(istat, fstat)
        self.rb = ts._REFCODE[np.frombuffer(self.refbase, np.uint8)]

    @classmethod
    def of(cls, res):
        return cls(res.depth, res.istat, res.fstat, res.refbase, res.pos0)

    @classmethod
    def of_counts(cls, h):
        """a test_select.Dense (counts alone: every other sum is zero)"""
        istat = np.zeros((h.n_lib, 6, 9, h.n_pos), np.uint32)
        istat[:, 1:5, 0, :] = h.cnt
        return cls(h.depth, istat, np.zeros((h.n_lib, 6, 4, h.n_pos), np.float32), h.refbase, h.pos0)


def reference(D, idx, alt=None, lib_on=None, tests=capi.VET_ALL_TESTS, f64=False, **t):
    """The header's predicate: (fail uint32 [L, 4, n], keep uint32 [n], vals float32 [L, 4, NVAL, n], status).  f64: the differences
    evaluated in double precision (what the header forbids), for the tests that show the difference."""
    idx = np.asarray(idx, np.int64); n = idx.size
    L, P = D.n_lib, D.n_pos
    alt = np.full(n, 15, np.int64) if alt is None else np.asarray(alt, np.int64)
    on = np.ones(L, bool) if lib_on is None else np.asarray(lib_on, bool)
    inr = (idx >= 0) & (idx < P)
    k = np.where(inr, idx, 0)
    rb = np.where(inr, D.rb[k], -1) if P else np.full(n, -1)
    status = (capi.VET_OUT_OF_RANGE if (~inr).any() else 0) | (capi.VET_NOT_ASCENDING if (idx[1:] < idx[:-1]).any() else 0)
    fail = np.zeros((L, 4, n), np.uint32); vals = np.zeros((L, 4, NVAL, n), np.float32); keep = np.zeros(n, np.uint32)
    r = np.maximum(rb, 0) + 1
    wide = np.float64 if f64 else np.float32
    for l in range(L):
        if not on[l]:
            fail[l] = NOT_ASKED
            continue
        Dl = D.depth[l, k]
        Cr = D.istat[l, r, 0, k]
        mr = D.metrics[l][r[:, None], np.array(MCOL)[None, :], k[:, None]]
        for v in range(4):
            Cv, Pv, Mv = (D.istat[l, v + 1, f, k] for f in (0, 3, 4))
            mv = D.metrics[l][v + 1, np.array(MCOL)[None, :], k[:, None]]
            S = Pv.astype(U64) + Mv.astype(U64)
            f = np.zeros(n, np.uint32)

            def bit(name, cond):
                f[cond] |= BIT[name]
            bit("DEPTH", Dl < np.uint32(t["min_depth"]))
            bit("VAR_COUNT", Cv < np.uint32(t["min_var_count"]))
            bit("VAR_FREQ", Cv.astype(U64) * U64(t["freq_den"]) < U64(t["freq_num"]) * Dl.astype(U64))
            bit("STRAND", (S >= U64(t["min_strand_reads"])) & (np.minimum(Pv, Mv).astype(U64) * U64(t["strand_den"]) < U64(t["strand_num"]) * S))
            var, ref = Cv > 0, Cr >= np.uint32(t["min_ref_reads"])
            for c, (name, key) in enumerate((("READPOS", "readpos"), ("DIST3", "dist3"), ("BQ", "bq"), ("MAPQ", "mapq"), ("MMQS", None), ("RL", "rl"))):
                if key:
                    bit("VAR_" + name, var & (mv[:, c] < F32(t["min_var_" + key])))
                    bit("REF_" + name, ref & (mr[:, c] < F32(t["min_ref_" + key])))
            bit("VAR_MMQS", var & (mv[:, 4] > F32(t["max_var_mmqs"])))
            mvw, mrw = mv.astype(wide), mr.astype(wide)
            d_mmqs, d_mapq, d_rl = mvw[:, 4] - mrw[:, 4], mrw[:, 3] - mvw[:, 3], mrw[:, 5] - mvw[:, 5]
            bound = wide(F32(t["max_rl_diff"])) * mrw[:, 5]
            assert f64 or (d_rl.dtype == np.float32 and bound.dtype == np.float32)
            bit("MMQS_DIFF", var & ref & (d_mmqs > F32(t["max_mmqs_diff"])))
            bit("MAPQ_DIFF", var & ref & (d_mapq > F32(t["max_mapq_diff"])))
            bit("RL_DIFF", var & ref & (d_rl > bound))
            f &= np.uint32(tests)
            with np.errstate(divide="ignore", invalid="ignore"):
                freq = np.where(Dl > 0, Cv.astype(F32) / Dl.astype(F32), F32(0)).astype(F32)
                strand = np.where(S > 0, Pv.astype(F32) / S.astype(F32), F32(0)).astype(F32)
            val = np.stack([Cv.astype(F32), Cr.astype(F32), Dl.astype(F32), freq, strand, d_mmqs.astype(F32), d_mapq.astype(F32), d_rl.astype(F32)] +
                           [mv[:, c] for c in range(6)] + [mr[:, c] for c in range(6)])
            judged = (rb >= 0) & (rb != v) & ((alt >> v) & 1).astype(bool)
            fail[l, v] = np.where(rb < 0, NO_SITE, np.where(judged, f, NOT_ASKED))
            vals[l, v] = np.where(judged[None, :], val, F32(0))
            keep |= (judged & (f == 0)).astype(np.uint32) << np.uint32(v)
    return fail, keep, vals, status


# ------------------------------------------------------------------------------------------------ calling the library

def call(route, v, d, idx, alt=None, lib_on=None, tests=capi.VET_ALL_TESTS, want=ALL, ds=None, status=True, handle=True, params=True, ws=True, no_idx=False,
         n=None, fields=None, **t):
    """brc_vet_sites into sentinel-filled buffers of [planes][n + PAD] and a scratch of exactly brc_vet_workspace bytes; returns
    (rc, status word, fail words [L, 4, ds], keep words [ds], vals words [L, 4, NVAL, ds])"""
    par, keepalive = capi.vet_params(lib_on, tests, **t)
    for k, x in (fields or {}).items():
        setattr(par, k, x)
    idx = np.asarray(idx, np.int32)
    n = idx.size if n is None else n
    ds = max(n, 0) + PAD if ds is None else ds
    L = int(v.n_lib) if v is not None and 0 < v.n_lib < 1000 else 1
    w = max(ds, 1)
    bf, bk, bv, bs = route.sentinel_words(L * 4 * w), route.sentinel_words(w), route.sentinel_words(L * 4 * NVAL * w), route.sentinel_words(1)
    wsb = route.vet.workspace(v, n) if v is not None else 0
    assert wsb % 4 == 0
    bw = route.sentinel_words(wsb // 4)
    bi = route.put(idx)
    ba = route.put(np.asarray(alt, np.uint32)) if alt is not None else None
    rc = route.vet.lib.brc_vet_sites(route.vet.h if handle else None, C.byref(v) if v is not None else None, C.byref(d) if d is not None else None,
                                     C.byref(par) if params else None, None if no_idx else route.ptr(bi), route.ptr(ba) if ba is not None else None, n, ds,
                                     route.ptr(bf) if "fail" in want else None, route.ptr(bk) if "keep" in want else None,
                                     route.ptr(bv) if "vals" in want else None, route.ptr(bs) if status else None, route.ptr(bw) if ws else None, None)
    del keepalive
    return (rc, int(route.words(bs)[0]), route.words(bf)[:L * 4 * w].reshape(L, 4, w).copy(), route.words(bk)[:w].copy(),
            route.words(bv)[:L * 4 * NVAL * w].reshape(L, 4, NVAL, w).copy())


def untouched(*arrays):
    return all((a == SENT).all() for a in arrays)


def check(route, v, d, D, idx, alt=None, lib_on=None, tests=capi.VET_ALL_TESTS, what="", want=ALL, **t):
    """one call against the reference, bit for bit, sentinels included; returns the reference's (fail, keep, vals, status)"""
    wf, wk, wv, wst = reference(D, idx, alt, lib_on, tests, **t)
    n = len(idx)
    rc, st, gf, gk, gv = call(route, v, d, idx, alt, lib_on, tests, want=want, **t)
    assert rc == 0, (what, route.vet.lib.brc_vet_last_error(route.vet.h))
    assert st == wst, (what, st, wst)
    if "fail" in want:
        assert np.array_equal(gf[:, :, :n], wf), (what, "fail", np.argwhere(gf[:, :, :n] != wf)[:4].tolist())
    if "keep" in want:
        assert np.array_equal(gk[:n], wk), (what, "keep", np.argwhere(gk[:n] != wk)[:4].tolist())
    if "vals" in want:
        assert np.array_equal(gv[:, :, :, :n], wv.view(np.uint32)), (what, "vals", np.argwhere(gv[:, :, :, :n] != wv.view(np.uint32))[:4].tolist())
    assert untouched(gf[:, :, n:] if "fail" in want else gf, gk[n:] if "keep" in want else gk, gv[:, :, :, n:] if "vals" in want else gv), "%s: wrote outside [0, n)" % what
    return wf, wk, wv, wst


def bits_seen(fail):
    return int(np.bitwise_or.reduce(fail[fail < NOT_ASKED].ravel())) if (fail < NOT_ASKED).any() else 0


# ------------------------------------------------------------------------------------------------ hand-made views

NONE32 = ts.NONE32


def full_views(route, depth, istat, fstat, ref=None, ref_lo=0, ref_len=None, pos0=0, dead=3, in_record=()):
    """test_select.build_views with every sum of a bucket: a brc_device_view + brc_device_indels in the route's memory that expand to
    depth [L, P], istat [L, 6, 9, P], fstat [L, 6, 4, P] (base buckets 1..4 are placed; the others must be empty).  Per (library,
    position) the first two non-empty base buckets go to the two slots, the others to third-allele records; in_record: (library, bucket
    1..4, position) triples that go to a record whatever the slots hold.  Returns (view, indels view, Dense, keepalive)."""
    depth = np.asarray(depth, np.uint32); istat = np.asarray(istat, np.uint32); fstat = np.asarray(fstat, np.float32)
    L, Pn = depth.shape
    assert not istat[:, (0, 5)].any()
    PS = (Pn + 63) // 64 * 64
    rng = np.random.default_rng(L * 1000 + Pn)

    def planes(a, k):
        out = np.zeros((k, PS), a.dtype); out[:, :Pn] = a.reshape(k, Pn); return out
    slotid = np.full((L, Pn), 0xFFFF, np.uint32)
    si = np.zeros((L, 2, 9, Pn), np.uint32); sf = np.zeros((L, 2, 4, Pn), np.float32)
    recs = []
    full = istat[:, 1:5].any(axis=2) | (fstat[:, 1:5] != 0).any(axis=2)                  # [L, 4, P]
    for l, k in zip(*np.nonzero(full.any(axis=1))):
        nz = [b for b in range(4) if full[l, b, k]]
        if len(nz) == 4:
            nz = [nz[3], nz[0], nz[2], nz[1]]                                  # (slot order is not bucket order)
        to_rec = [b for b in nz if (l, b + 1, k) in in_record]
        nz = [b for b in nz if b not in to_rec]
        sid = 0xFFFF
        for s, b in enumerate(nz[:2]):
            sid = (sid & ~(0xFF << (8 * s))) | ((b + 1) << (8 * s))
            si[l, s, :, k] = istat[l, b + 1, :, k]; sf[l, s, :, k] = fstat[l, b + 1, :, k]
        slotid[l, k] = sid
        for b in nz[2:] + to_rec:
            recs.append((k, (l << 8) | (b + 1), istat[l, b + 1, :, k], fstat[l, b + 1, :, k]))
    for _ in range(dead if recs else 0):
        recs.append((NONE32, 0, np.full(9, 7, np.uint32), np.zeros(4, np.float32)))
    recs = [recs[i] for i in rng.permutation(len(recs))]
    xagg = np.zeros((len(recs), 16), np.uint32)
    for r, (k, lb, ii, ff) in enumerate(recs):
        xagg[r, 0], xagg[r, 1] = k, lb
        xagg[r, 2:11] = ii; xagg[r, 11:15] = np.asarray(ff, np.float32).view(np.uint32)
    keep = {"ncol": route.put(planes(depth, L)), "depth": route.put(planes(depth, L)), "slotid": route.put(planes(slotid, L)),
            "si": route.put(planes(si, L * 18)), "sf": route.put(planes(sf, L * 8)), "xagg": route.put(xagg)}
    v = capi.DeviceView(route.mem, 0, L, pos0, Pn, PS, *[route.ptr(keep[k]) for k in ("ncol", "depth", "slotid", "si")], None, route.ptr(keep["sf"]),
                        route.ptr(keep["xagg"]) if len(recs) else None, len(recs))
    d = capi.DeviceIndels(route.mem, 0, L, pos0, Pn, None, 0)
    rl = pos0 + Pn if ref_len is None else ref_len
    refbase = bytearray(b"N" * Pn)
    if ref is not None:
        keep["ref"] = route.put(np.frombuffer(bytes(ref), np.uint8))
        d.ref, d.ref_lo, d.ref_hi, d.ref_len = route.ptr(keep["ref"]), ref_lo, ref_lo + len(ref), rl
        for k in range(Pn):
            p = pos0 + k
            if ref_lo <= p < ref_lo + len(ref) and p < rl and ref[p - ref_lo] != 0:
                refbase[k] = ref[p - ref_lo]
    return v, d, Dense(depth, istat, fstat, bytes(refbase), pos0), keep


def random_sums(P, L=2, seed=5, third=0.3):
    """dense sums of a region with every kind of site: the reference base deep, one or two alternative alleles with few reads and
    poorer metrics, empty positions; depth = the buckets' reads"""
    rng = np.random.default_rng(seed)
    ref = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=P).tobytes()
    rb = ts._REFCODE[np.frombuffer(ref, np.uint8)]
    istat = np.zeros((L, 6, 9, P), np.uint32); fstat = np.zeros((L, 6, 4, P), np.float32)
    cnt = np.zeros((L, 4, P), np.int64)
    cnt[:, rb, np.arange(P)] = rng.integers(0, 40, (L, P))
    for rate in (0.5, third):
        m = rng.random((L, P)) < rate
        b = rng.integers(0, 4, (L, P))
        for l in range(L):
            kk = np.nonzero(m[l])[0]
            cnt[l, b[l, kk], kk] += rng.integers(1, 12, kk.size)
    cnt[:, :, rng.random(P) < 0.05] = 0
    c = cnt.astype(np.uint32)
    istat[:, 1:5, 0] = c
    plus = (rng.random((L, 4, P)) * (cnt + 1)).astype(np.uint32)
    istat[:, 1:5, 3] = np.minimum(plus, c); istat[:, 1:5, 4] = c - istat[:, 1:5, 3]
    for f, hi in ((1, 61), (2, 61), (8, 42), (6, 90), (7, 152)):               # smq, sse, sbq, smmq, sclip: a per-read value times the count
        istat[:, 1:5, f] = (rng.integers(0, hi, (L, 4, P)) * cnt).astype(np.uint32)
    istat[:, 1:5, 5] = np.minimum(rng.integers(0, 3, (L, 4, P)), cnt).astype(np.uint32)
    for f in range(4):
        fstat[:, 1:5, f] = (rng.random((L, 4, P)) * cnt).astype(np.float32)
    return cnt.sum(axis=1).astype(np.uint32), istat, fstat, ref


# thresholds that split the fixtures: several failure bits and passes on real data
MID = dict(min_depth=8, min_var_count=3, freq_num=1, freq_den=10, min_strand_reads=4, strand_num=1, strand_den=10, min_ref_reads=2,
           min_var_readpos=0.3, min_var_dist3=0.3, min_var_bq=25.0, min_var_mapq=30.0, max_var_mmqs=40.0, min_var_rl=100.0,
           min_ref_readpos=0.4, min_ref_dist3=0.4, min_ref_bq=28.0, min_ref_mapq=40.0, min_ref_rl=100.0, max_mmqs_diff=20.0,
           max_mapq_diff=10.0, max_rl_diff=0.05)


# ... and a set that lets well-supported alleles pass: a few tests, each with a threshold in the middle of the data
EASY = T_(min_depth=6, min_var_count=2, freq_num=1, freq_den=20, min_var_mapq=15.0, min_ref_mapq=15.0, max_mapq_diff=40.0, min_var_bq=10.0)


def select_list(D, min_alt=2):
    """what brc_select_sites finds with every library a case library: (idx, why) by test_select's reference"""
    h = ts.Dense(D.depth, D.istat[:, 1:5, 0, :], D.refbase, [], D.pos0)
    return h.want(None, ts.P_(ts.SNV, min_alt=min_alt))


# ------------------------------------------------------------------------------------------------ 1. fixtures

EASY_LOW = T_(min_depth=4, min_var_count=1, freq_num=1, freq_den=5, min_var_mapq=10.0, min_var_bq=10.0)


@pytest.fixture(scope="module")
def low_region(oracle_lib):
    """test_select's synthetic low-depth region of two libraries and the oracle's result of it"""
    import synth
    rng = np.random.default_rng(11)
    ref = synth.make_ref(rng, 3000, weird=0.01)
    arrs = synth.make_batch(77, ref, 260, read_len=(60, 120), style="indel", n_libs=2, mismatch=0.06)
    res, _ = td.oracle_result(oracle_lib, arrs, 50, 2950, ref, **PER_LIB)
    return ref, arrs, res


def test_golden_fixture_and_two_libraries(route, oracle_lib, test_bam, low_region):
    """test_bam.npz all-lib: the list select finds with its reason words, and every position with all four bases asked; the two-library
    synthetic batch per library and with lib_on subsets.  On the reference's side each fixture shows several failure bits and a pass."""
    beg0, end = 10402736, 10405248
    res, _ = td.oracle_result(oracle_lib, test_bam, beg0, end, test_bam["ref"], tid=20)
    eng = td.computed(route.engine_lib, test_bam, beg0, end, test_bam["ref"], tid=20)
    v, d = ts.views_of(eng)
    D = Dense.of(res)
    idx, why = select_list(D)
    assert len(idx) > 20
    wf, wk, _, _ = check(route, v, d, D, idx, why, what="test_bam, select's list", **MID)
    assert bin(bits_seen(wf)).count("1") >= 5, bits_seen(wf)
    wf, wk, _, _ = check(route, v, d, D, idx, why, what="test_bam, select's list, few tests", **EASY)
    assert bits_seen(wf) and (wk != 0).any() and (wk == 0).any(), (bits_seen(wf), wk)
    wf, wk, _, _ = check(route, v, d, D, np.arange(res.n_pos), what="test_bam, every position", **MID)
    assert bin(bits_seen(wf)).count("1") >= 6
    wf, wk, _, _ = check(route, v, d, D, np.arange(res.n_pos), what="test_bam, every position, few tests", **EASY)
    assert (wk != 0).any() and (wk == 0).any()
    eng.close()
    ref, arrs, res = low_region
    eng = td.computed(route.engine_lib, arrs, 50, 2950, ref, **PER_LIB)
    v, d = ts.views_of(eng)
    D = Dense.of(res)
    idx, why = select_list(D, 1)
    low = dict(MID, min_depth=3, min_var_count=1, min_var_rl=50.0, min_ref_rl=50.0)
    seen = 0
    for lib_on in (None, [1, 0], [0, 1], [1, 1]):
        wf, wk, _, _ = check(route, v, d, D, idx, why, lib_on, what="two libraries %r" % (lib_on,), **low)
        seen |= bits_seen(wf)
        wf, wk, _, _ = check(route, v, d, D, idx, why, lib_on, what="two libraries %r, few tests" % (lib_on,), **EASY_LOW)
        assert (wk != 0).any() and (wk == 0).any()
        if lib_on and not lib_on[0]:
            assert (wf[0] == NOT_ASKED).all()
    assert bin(seen).count("1") >= 5
    check(route, v, d, D, np.arange(res.n_pos), what="two libraries, every position", **low)
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. the bucket's three homes

def test_buckets_that_live_in_records_only(route, oracle_lib, monkeypatch):
    """The knob libraries under BRC_FORCE_DOM=3 + BRC_XEV_CAP=1: elements whose variant bucket, and elements whose reference bucket,
    exist only in a third-allele record — shown first on the oracle's planes against the view's slots."""
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
    in_slots = slots["istat"].reshape(2, 6, 9, res.n_pos)[:, 1:5, 0, :]
    only_rec = (in_slots != D.istat[:, 1:5, 0, :]) & (D.istat[:, 1:5, 0, :] != 0)      # [L, 4, P]: buckets that exist only in a record
    rbk = D.rb
    ok = rbk >= 0
    ref_in_rec = ok & only_rec[:, np.maximum(rbk, 0), np.arange(res.n_pos)].any(axis=0)
    var_in_rec = ok & (only_rec.any(axis=0) & (np.arange(4)[:, None] != rbk[None, :])).any(axis=0)
    assert ref_in_rec.sum() >= 3 and var_in_rec.sum() >= 3, (ref_in_rec.sum(), var_in_rec.sum())
    idx = np.nonzero(ref_in_rec | var_in_rec)[0]
    idx = np.sort(np.concatenate([idx, idx[:40], np.arange(0, res.n_pos, 7)]))          # (with repeats, and positions without records)
    t = dict(MID, min_depth=4, min_var_count=1)
    wf, wk, wv, _ = check(route, v, d, D, idx, what="records", **t)
    # ... and the records are needed: judged on the slots alone, elements come out otherwise
    rc, st, gf, gk, gv = call(route, bare, d, idx, **t)
    assert rc == 0 and not np.array_equal(gv[:, :, :, :len(idx)], wv.view(np.uint32))
    eng.close()


def two_record_views(route):
    """one position with records of two libraries in different buckets (the variant's in library 0, the reference's in library 1),
    and another such position, listed by elements 62 .. 66 and 254 .. 258 of a list of 300: equal neighbours across a wave edge and across a workgroup edge"""
    P = 400
    depth, istat, fstat, ref = random_sums(P, seed=8, third=0.0)
    ref = bytearray(ref)
    for k in (130, 330):
        ref[k] = ord("A")
        istat[:, 1:5, :, k] = np.arange(1, 5)[None, :, None] * 3 + np.arange(9)[None, None, :] + 2
        istat[:, 1:5, 3, k] = 4; istat[:, 1:5, 4, k] = 3
        fstat[:, 1:5, :, k] = 1.5 + np.arange(4)[None, None, :]
        depth[:, k] = istat[:, 1:5, 0, k].sum(axis=1)
    rec = [(0, 3, 130), (1, 1, 130), (0, 1, 330), (1, 4, 330)]
    v, d, D, keep = full_views(route, depth, istat, fstat, bytes(ref), in_record=rec)
    idx = np.concatenate([np.arange(0, 124, 2), [130] * 5, np.arange(131, 318), [330] * 5, np.arange(331, 372)])
    assert (idx[62:67] == 130).all() and (idx[254:259] == 330).all() and idx.size == 300 and (np.diff(idx) >= 0).all()
    return v, d, D, keep, idx


def test_two_records_of_one_position_and_equal_neighbours_across_the_edges(route):
    v, d, D, keep, idx = two_record_views(route)
    assert v.n_xagg >= 4
    wf, wk, wv, _ = check(route, v, d, D, idx, what="two records", **MID)
    assert (wv[0, 2, 0, 62:67] == wv[0, 2, 0, 62]).all() and wv[0, 2, 0, 62] > 0
    bare = capi.DeviceView.from_buffer_copy(v); bare.n_xagg = 0
    rc, st, gf, gk, gv = call(route, bare, d, idx, **MID)
    for j in (62, 66, 254, 258):                            # without the records every one of those elements differs
        assert not np.array_equal(gv[:, :, :, j], wv.view(np.uint32)[:, :, :, j]), j


# ------------------------------------------------------------------------------------------------ 3. list shapes

def shape_views(route, records=True):
    depth, istat, fstat, ref = random_sums(700, seed=6, third=0.3 if records else 0.0)
    if not records:                                         # at most two base buckets per position: no third-allele record
        full = istat[:, 1:5, 0] != 0
        extra = np.cumsum(full, axis=1) > 2
        istat[:, 1:5][np.broadcast_to(extra[:, :, None, :], istat[:, 1:5].shape)] = 0
        fstat[:, 1:5][np.broadcast_to(extra[:, :, None, :], fstat[:, 1:5].shape)] = 0
    return full_views(route, depth, istat, fstat, ref, pos0=1000, ref_lo=1000)


def test_list_lengths_and_the_workspace(route):
    """n = 0, 1, 63, 64, 65, 256, 257 on a view with records and on one without (no link launch, a scratch of 0 bytes)"""
    for records in (True, False):
        v, d, D, keep = shape_views(route, records)
        assert (v.n_xagg > 0) == records
        rng = np.random.default_rng(3)
        for n in (0, 1, 63, 64, 65, 256, 257):
            idx = np.sort(rng.integers(0, D.n_pos, n))
            alt = rng.integers(0, 64, n)
            assert route.vet.workspace(v, n) == (4 * (n + int(v.n_xagg)) if records and n else 0)
            wf, wk, _, _ = check(route, v, d, D, idx, alt, what="n = %d, records %r" % (n, records), **MID)
            wf2, wk, _, _ = check(route, v, d, D, idx, alt, what="n = %d, records %r, few tests" % (n, records), **EASY)
            if n >= 63:
                assert bits_seen(wf) and bits_seen(wf2) and (wk != 0).any() and (wk == 0).any()
    assert route.vet.workspace(None, 5) == 0 and route.vet.workspace(v, -1) == 0
    # n == 0 clears the status word and touches nothing else
    rc, st, gf, gk, gv = call(route, v, d, [], **MID)
    assert (rc, st) == (0, 0) and untouched(gf, gk, gv)


def test_bad_lists_stay_in_range(route):
    """one element out of range at either end; a descent: the status bits, NO_SITE, and every store inside [0, n)"""
    v, d, D, keep = shape_views(route, records=False)
    P = D.n_pos
    for what, idx, st in (("below", [-1, 3, 9], 1), ("beyond", [3, 9, P], 1), ("far", [-2 ** 31, 5, 2 ** 31 - 1], 1), ("descent", [5, 4, 300, 299, 700 - 1], 2),
                          ("both", [9, 3, P + 7], 3)):
        wf, wk, wv, wst = check(route, v, d, D, idx, what=what, **MID)
        assert wst == st
        if st & 1:
            bad = [j for j, k in enumerate(idx) if not 0 <= k < P]
            assert (wf[:, :, bad] == NO_SITE).all() and not wk[bad].any()
    # a descent on a view WITH records: status and range alone (a bucket with a record is unspecified then)
    v, d, D, keep = shape_views(route, records=True)
    idx = np.concatenate([np.arange(100, 400), np.arange(50, 350)])
    rc, st, gf, gk, gv = call(route, v, d, idx, **MID)
    assert rc == 0 and st == 2 and untouched(gf[:, :, 600:], gk[600:], gv[:, :, :, 600:]) and not (gf[:, :, :600] == SENT).any()


def test_empty_positions_of_a_site_list_axis(route, oracle_lib, low_region):
    ref, arrs, res = low_region
    wins = [(300, 301), (640, 710), (1500, 1501), (2000, 2064)]
    b = np.array([w[0] for w in wins], np.int32); e = np.array([w[1] for w in wins], np.int32)
    eng = capi.Engine(route.engine_lib, **PER_LIB)
    eng.begin_region(0, 50, 2950, ref)
    eng.push_reads(capi.select_reads(arrs, capi.fetch_overlapping(arrs, capi.read_ends(arrs), 49, 2950)))
    eng.region_windows(b, e)
    eng.upload(); eng.compute()
    v, d = ts.views_of(eng)
    asked = np.zeros(res.n_pos, bool)
    for x, y in wins:
        asked[x - 1 - res.pos0:y - res.pos0] = True
    announced = np.zeros(res.n_pos, bool)
    for t in range(0, res.n_pos, 64):
        k = np.nonzero(asked[t:t + 64])[0]
        if k.size:
            announced[t + k[0]:t + k[-1] + 1] = True
    D = Dense(res.depth * announced, res.istat * announced, res.fstat * announced.astype(np.float32), res.refbase, res.pos0)
    idx = np.arange(200, 800)
    wf, wk, wv, _ = check(route, v, d, D, idx, what="site list axis", **dict(MID, min_depth=1, min_var_count=0))
    empty = ~announced[idx]
    assert empty.sum() > 100 and ((wf[:, :, empty] & BIT["DEPTH"]) | (wf[:, :, empty] >= NOT_ASKED)).all()
    assert not wv[:, :, 2][:, :, empty].any()
    eng.close()


# ------------------------------------------------------------------------------------------------ 4. thresholds at the edge

FP_TESTS = [("VAR_READPOS", "min_var_readpos", 0, "v", -1), ("VAR_DIST3", "min_var_dist3", 1, "v", -1), ("VAR_BQ", "min_var_bq", 2, "v", -1),
            ("VAR_MAPQ", "min_var_mapq", 3, "v", -1), ("VAR_MMQS", "max_var_mmqs", 4, "v", +1), ("VAR_RL", "min_var_rl", 5, "v", -1),
            ("REF_READPOS", "min_ref_readpos", 0, "r", -1), ("REF_DIST3", "min_ref_dist3", 1, "r", -1), ("REF_BQ", "min_ref_bq", 2, "r", -1),
            ("REF_MAPQ", "min_ref_mapq", 3, "r", -1), ("REF_RL", "min_ref_rl", 5, "r", -1)]


def edge_views(route):
    """sums whose quotients are no short decimals: 300 positions, reference A everywhere, variant C; counts 1 .. 23"""
    P = 300
    rng = np.random.default_rng(12)
    istat = np.zeros((1, 6, 9, P), np.uint32); fstat = np.zeros((1, 6, 4, P), np.float32)
    for b in (1, 2):
        c = rng.integers(1, 24, P)
        istat[0, b, 0] = c; istat[0, b, 3] = c // 2; istat[0, b, 4] = c - c // 2
        for f in (1, 2, 5, 6, 7, 8):
            istat[0, b, f] = rng.integers(0, 4000, P)
        istat[0, b, 5] = np.minimum(istat[0, b, 5], c)
        fstat[0, b] = (rng.random((4, P)) * c).astype(np.float32)
    depth = istat[:, 1:5, 0].sum(axis=1)
    return full_views(route, depth, istat, fstat, b"A" * P)


def test_every_fp32_test_at_its_threshold_and_one_ulp_beside(route):
    v, d, D, keep = edge_views(route)
    idx = np.arange(D.n_pos)
    alt = np.full(D.n_pos, capi.WHY_C)
    for name, key, c, side, sign in FP_TESTS:
        for k in (7, 100, 263):
            m = D.metrics[0, 2 if side == "v" else 1, MCOL[c], k]
            assert m > 0
            got = []
            for thr in (np.nextafter(m, F32(-np.inf)), m, np.nextafter(m, F32(np.inf))):
                t = T_(**{key: float(thr)})
                wf, _, _, _ = check(route, v, d, D, idx, alt, tests=BIT[name], what="%s at %r" % (name, thr), want=("fail",), **t)
                got.append(bool(wf[0, 1, k] & BIT[name]))
                assert not (wf[0, 1] & ~np.uint32(BIT[name])).any()
            assert got == ([False, False, True] if sign < 0 else [True, False, False]), (name, k, got)


def diff_views(route):
    """random sums behind the three differences: mapping quality, mismatch quality and clipped length of a reference bucket (A) and a
    variant bucket (C) at 200 positions, counts 1 .. 23, so that the averages are no short binary fractions"""
    P = 200
    rng = np.random.default_rng(13)
    istat = np.zeros((1, 6, 9, P), np.uint32); fstat = np.zeros((1, 6, 4, P), np.float32)
    for b in (1, 2):
        c = rng.integers(1, 24, P)
        istat[0, b, 0] = c; istat[0, b, 3] = c // 2; istat[0, b, 4] = c - c // 2
        for f in (1, 6, 7):
            istat[0, b, f] = rng.integers(0, 4000, P)
    depth = istat[:, 1:5, 0].sum(axis=1)
    return full_views(route, depth, istat, fstat, b"A" * P)


def test_differences_are_single_fp32_operations(route):
    """MMQS_DIFF, MAPQ_DIFF and RL_DIFF with the threshold at the fp32 difference and one ulp beside it; for RL_DIFF, positions where a
    float64 evaluation of the same fp32 inputs gives the other answer — found on the reference's side and asserted to exist"""
    v, d, D, keep = diff_views(route)
    idx = np.arange(D.n_pos)
    alt = np.full(D.n_pos, capi.WHY_C)
    mv, mr = D.metrics[0, 2], D.metrics[0, 1]
    for name, key, dv in (("MMQS_DIFF", "max_mmqs_diff", mv[8] - mr[8]), ("MAPQ_DIFF", "max_mapq_diff", mr[1] - mv[1])):
        assert dv.dtype == np.float32
        for k in (3, 77, 150):
            got = []
            for thr in (np.nextafter(dv[k], F32(-np.inf)), dv[k], np.nextafter(dv[k], F32(np.inf))):
                wf, _, _, _ = check(route, v, d, D, idx, alt, tests=BIT[name], what="%s at %r" % (name, thr), want=("fail",), **T_(**{key: float(thr)}))
                got.append(bool(wf[0, 1, k] & BIT[name]))
            assert got == [True, False, False], (name, k, got)
    # RL_DIFF: thresholds chosen per position so that the two sides of the comparison meet: max_rl_diff = fl(d / m_r) and its neighbours
    flips = 0
    d_rl = mr[11] - mv[11]
    with np.errstate(divide="ignore", invalid="ignore"):
        fr = (d_rl / mr[11]).astype(np.float32)
    cand = [k for k in range(D.n_pos) if mr[11][k] > 0 and d_rl[k] > 0 and np.isfinite(fr[k])]
    for k in cand:
        for thr in (fr[k], np.nextafter(fr[k], F32(-np.inf)), np.nextafter(fr[k], F32(np.inf))):
            t = T_(max_rl_diff=float(thr))
            a = reference(D, [k], [capi.WHY_C], tests=BIT["RL_DIFF"], **t)[0][0, 1, 0]
            b = reference(D, [k], [capi.WHY_C], tests=BIT["RL_DIFF"], f64=True, **t)[0][0, 1, 0]
            if a != b:
                flips += 1
                wf, _, _, _ = check(route, v, d, D, idx, alt, tests=BIT["RL_DIFF"], what="RL_DIFF at %d" % k, want=("fail", "vals"), **t)
                assert wf[0, 1, k] == a != b
        if flips >= 3:
            break
    assert flips >= 1, "no position where float64 evaluation decides RL_DIFF otherwise: choose other sums"


def test_integer_tests_met_exactly_and_the_judged_only_when_conditions(route):
    P = 64
    istat = np.zeros((1, 6, 9, P), np.uint32); fstat = np.zeros((1, 6, 4, P), np.float32)
    k = np.arange(P)
    istat[0, 1, 0] = 20; istat[0, 1, 3] = 10; istat[0, 1, 4] = 10; istat[0, 1, 1] = 20 * 60
    istat[0, 2, 0] = k % 8; istat[0, 2, 3] = (k % 8) // 4; istat[0, 2, 4] = k % 8 - (k % 8) // 4; istat[0, 2, 1] = (k % 8) * 10
    depth = (istat[:, 1:5, 0].sum(axis=1) * (k >= 8)).astype(np.uint32)                 # D == 0 on the first eight positions
    v, d, D, keep = full_views(route, depth, istat, fstat, b"A" * P)
    alt = np.full(P, capi.WHY_C)
    t = T_(min_depth=24, min_var_count=4, freq_num=1, freq_den=6, min_strand_reads=4, strand_num=1, strand_den=4, min_ref_reads=21, min_var_mapq=11.0,
           min_ref_mapq=61.0, max_mapq_diff=49.0)
    wf, wk, wv, _ = check(route, v, d, D, k, alt, what="integers", **t)
    f = wf[0, 1]
    assert not f[12] & BIT["DEPTH"] and f[11] & BIT["DEPTH"]                          # D = 24 / 23 against 24
    assert not f[12] & BIT["VAR_COUNT"] and f[11] & BIT["VAR_COUNT"]
    assert not f[12] & BIT["VAR_FREQ"] and f[11] & BIT["VAR_FREQ"]                    # 4 * 6 = 24 * 1; 3 * 6 < 23
    assert not f[12] & BIT["STRAND"] and f[13] & BIT["STRAND"] and not f[11] & BIT["STRAND"]        # 1 * 4 = 4; 1 * 4 < 5; 3 reads: not judged
    assert f[8] == (BIT["DEPTH"] | BIT["VAR_COUNT"] | BIT["VAR_FREQ"])                 # C_v == 0: no variant-side fp32 test, no difference
    assert f[12] & BIT["VAR_MAPQ"] and not f[12] & (BIT["REF_MAPQ"] | BIT["MAPQ_DIFF"])  # C_r = 20 < min_ref_reads: the reference side is not judged
    assert not wv[0, 1, 3, :8].any() and not wv[0, 1, 2, :8].any()
    assert (f[:8] & BIT["DEPTH"]).all() and not (f[1:8] & BIT["VAR_FREQ"]).any()       # D == 0: frequency 0 in vals, c * den < 0 never holds
    wf2, _, _, _ = check(route, v, d, D, k, alt, what="reference judged", **dict(t, min_ref_reads=20))
    assert wf2[0, 1, 12] & BIT["REF_MAPQ"] and wf2[0, 1, 12] & BIT["MAPQ_DIFF"]


def test_counts_and_thresholds_next_to_two_to_the_32(sim_route):
    """host views, CPU build: products that a 32-bit multiplication decides otherwise"""
    route = sim_route
    P = 8
    U = 2 ** 32 - 1
    istat = np.zeros((1, 6, 9, P), np.uint32); fstat = np.zeros((1, 6, 4, P), np.float32)
    istat[0, 1, 0] = 5
    istat[0, 2, 0] = [U, U - 1, 2 ** 31, 2 ** 31 + 1, 3, 2 ** 16, 2 ** 16 + 1, 1]
    istat[0, 2, 3] = [U, 2 ** 31, 2 ** 31, 7, 1, 2 ** 16, 1, 0]; istat[0, 2, 4] = [U, 2 ** 31, 1, 2 ** 31, 2, 2 ** 16, 2 ** 16, 1]
    depth = np.array([[U, U, U, U, 6, 2 ** 17, 2 ** 17, 2]], np.uint32)
    v, d, D, keep = full_views(route, depth, istat, fstat, b"A" * P)
    alt = np.full(P, capi.WHY_C)
    for t in (T_(min_depth=U, min_var_count=U, freq_num=U - 1, freq_den=U), T_(freq_num=2 ** 31, freq_den=U, strand_num=2 ** 31, strand_den=U, min_strand_reads=U),
              T_(freq_num=2 ** 16, freq_den=2 ** 17, strand_num=2 ** 16, strand_den=2 ** 16 + 1), T_(strand_num=U, strand_den=U)):
        wf, _, _, _ = check(route, v, d, D, np.arange(P), alt, what="2^32", **t)
    t = T_(freq_num=2 ** 16, freq_den=2 ** 17)
    c, Dl = istat[0, 2, 0].astype(np.uint64), depth[0].astype(np.uint64)
    wrapped = ((c * np.uint64(t["freq_den"])) & np.uint64(U)) < ((np.uint64(t["freq_num"]) * Dl) & np.uint64(U))
    exact = (reference(D, np.arange(P), alt, **t)[0][0, 1] & BIT["VAR_FREQ"]) != 0
    assert (wrapped != exact).any()


# ------------------------------------------------------------------------------------------------ 5. reference characters, masks, libraries

def test_reference_characters_and_slices(route):
    kinds = set()
    for what, (v, d, h, keepalive), _ in ts.refchar_views(route):
        kinds.add((bool(d.ref), d.ref_lo > d.pos0, d.ref_hi < d.pos0 + d.n_pos, d.ref_len < d.ref_hi))
        D = Dense.of_counts(h)
        wf, wk, _, _ = check(route, v, d, D, np.arange(D.n_pos), what=what, **T_(min_var_count=2))
        if what == "characters":
            assert (wf[0, :, :32] != NO_SITE).all() and (wf[0, :, 32:] == NO_SITE).all()     # ACGTacgt, four positions each
            assert (wf[0, :, :32] == NOT_ASKED).sum() == 32 and np.count_nonzero(wk) == 24
        if what == "no reference":
            assert not d.ref and (wf == NO_SITE).all() and not wk.any()
    assert len(kinds) >= 5


def test_each_test_alone_sets_only_its_own_bit(route):
    v, d, D, keep = shape_views(route)
    idx = np.arange(0, D.n_pos, 3)
    full = reference(D, idx, **MID)[0]
    assert bits_seen(full) == capi.VET_ALL_TESTS, "the thresholds leave a test that never fails: %x" % bits_seen(full)
    for name in capi.VET_TESTS:
        wf, _, _, _ = check(route, v, d, D, idx, tests=BIT[name], what=name, want=("fail", "keep"), **MID)
        assert bits_seen(wf) == BIT[name]
    wf, wk, _, _ = check(route, v, d, D, idx, tests=0, what="no test", **MID)
    assert bits_seen(wf) == 0


def test_alt_masks(route):
    v, d, D, keep = shape_views(route)
    idx = np.arange(5, 305)
    a = np.arange(300) % 16
    w_all = check(route, v, d, D, idx, None, what="alt NULL", **MID)
    assert np.array_equal(w_all[0], reference(D, idx, np.full(300, 15), **MID)[0])
    w = check(route, v, d, D, idx, a | capi.WHY_INS | capi.WHY_DEL | 0xFFFFFF00, what="INS / DEL and high bits", **MID)
    assert np.array_equal(w[0], reference(D, idx, a, **MID)[0])
    wf, wk, wv, _ = check(route, v, d, D, idx, np.zeros(300, np.int64), what="mask 0", **MID)
    assert (wf >= NOT_ASKED).all() and not wk.any() and not wv.any()


def lib254_views(route):
    depth, cnt, ref = ts.low_depth(70, L=254, seed=3, alt=0.1)
    istat = np.zeros((254, 6, 9, 70), np.uint32)
    istat[:, 1:5, 0] = cnt; istat[:, 1:5, 3] = cnt // 2; istat[:, 1:5, 4] = cnt - cnt // 2
    istat[:, 1:5, 1] = cnt * (np.arange(254) % 60)[:, None, None]
    return full_views(route, depth, istat, np.zeros((254, 6, 4, 70), np.float32), ref)


LIB254_ON = [l % 2 for l in range(254)]
LIB254_T = T_(min_depth=4, min_var_count=2, min_var_mapq=20.0, min_ref_mapq=30.0, min_ref_reads=1)


def test_254_libraries(route):
    v, d, D, keep = lib254_views(route)
    assert v.n_lib == 254 and v.n_xagg > 0
    idx = np.arange(70)
    wf, wk, _, _ = check(route, v, d, D, idx, lib_on=LIB254_ON, what="254 libraries", **LIB254_T)
    assert (wf[0::2] == NOT_ASKED).all() and bits_seen(wf[1::2]) and len(set(wk.tolist())) > 3
    check(route, v, d, D, idx, what="254 libraries, all on", **LIB254_T)
    v2 = capi.DeviceView.from_buffer_copy(v); d2 = capi.DeviceIndels.from_buffer_copy(d); v2.n_lib = d2.n_lib = 255
    rc, st, gf, gk, gv = call(route, v2, d2, [1], **MID)
    assert rc == capi.E_ARG and st == SENT


def test_lib_on_above_the_first_words(route):
    """254 libraries judged by test_select.lib_pattern(2), no copy of itself 16 .. 128 libraries further: a lib_on table indexed modulo
    32, 64 or 128 libraries judges other libraries — asserted on the reference's side"""
    v, d, D, keep = lib254_views(route)
    on = ts.lib_pattern(2)
    idx = np.arange(0, 70, 3)
    wf, wk, _, _ = check(route, v, d, D, idx, lib_on=on, what="lib_on pattern", **LIB254_T)
    assert all((wf[l] == NOT_ASKED).all() == (not on[l]) for l in range(254)) and bits_seen(wf)
    for period in (32, 64, 128):
        other = reference(D, idx, lib_on=ts.folded(on, period), **LIB254_T)
        assert not np.array_equal(other[0][128:], wf[128:]) and not np.array_equal(other[1], wk), period


def raw_dense(route, depth, slotid, si, sf, records, ref):
    """test_select.raw_views (the compact form written down) and the Dense its plain expansion gives"""
    v, d, istat, fstat, refbase, keep = ts.raw_views(route, depth, slotid, si, sf, records, ref=ref)
    return v, d, Dense(np.asarray(depth, np.uint32), istat, fstat, refbase, 0), keep


SLOT_I = (np.array([6, 300, 200, 4, 2, 1, 120, 700, 180], np.uint32), np.array([9, 500, 0, 5, 4, 0, 250, 0, 300], np.uint32))
SLOT_F = (np.array([1.5, 2.5, 3.5, 4.5], np.float32), np.array([2.25, 0.75, 5.0, 1.25], np.float32))


def same_bucket_views(route, named, other):
    """both slots of every position name bucket `named`; position k has slot 0 empty or counted (k & 1) and slot 1 empty or counted
    (k & 2), slot 1 with zeros among its integer sums, and the float sums of the two slots differ everywhere, empty slots included.
    Bucket `other` comes from a third-allele record."""
    import handmade_views as hv
    Pn = 134
    si = np.zeros((1, 2, 9, Pn), np.uint32); sf = np.zeros((1, 2, 4, Pn), np.float32)
    k = np.arange(Pn)
    for s in (0, 1):
        si[0, s] = SLOT_I[s][:, None] * ((k >> s) & 1).astype(np.uint32)[None, :]
        sf[0, s] = SLOT_F[s][:, None]
    recs = [hv.record(x, 0, other, [7, 350, 210, 3, 4, 2, 100, 900, 200], hv.f32bits([3.0, 1.0, 2.0, 5.0]).tolist()) for x in range(Pn)]
    return raw_dense(route, np.full((1, Pn), 30), np.full((1, Pn), named | (named << 8)), si, sf, recs, b"A" * Pn)


def test_two_slots_naming_one_bucket(route):
    """slotid with b0 == b1: the later write wins, integers are written only where they are not zero, floats always (expand_lane) —
    so slot 1's float sums stand with slot 0's integer sums wherever slot 1 holds a zero.  The bucket is once the reference's own
    (A, judged against C from a record) and once the asked alternate (C); lists from 0 .. 3 put every combination on lanes 63 and 64.
    Values and failure words, bit for bit."""
    tight = dict(MID, min_depth=1, min_var_count=7, min_var_mapq=52.0, min_ref_mapq=52.0, min_var_readpos=0.3, min_ref_readpos=0.3)
    for what, named, other in (("the reference's bucket", 1, 2), ("an asked alternate", 2, 1)):
        v, d, D, keep = same_bucket_views(route, named, other)
        # what the rule means, on the reference's side: position 3 (both counted), 1 (slot 0 alone), 2 (slot 1 alone), 0 (neither)
        assert D.istat[0, named, :, 3].tolist() == [9, 500, 200, 5, 4, 1, 250, 700, 300] and D.fstat[0, named, :, 3].tolist() == SLOT_F[1].tolist()
        assert D.istat[0, named, :, 1].tolist() == SLOT_I[0].tolist() and D.fstat[0, named, :, 1].tolist() == SLOT_F[1].tolist()
        assert D.istat[0, named, :, 2].tolist() == SLOT_I[1].tolist() and not D.istat[0, named, :, 0].any()
        seen = 0
        for first in range(4):
            idx = np.arange(first, D.n_pos)
            for t in (MID, tight):
                wf, wk, wv, _ = check(route, v, d, D, idx, np.full(idx.size, capi.WHY_C), what="%s from %d" % (what, first), **t)
                seen |= bits_seen(wf)
            count = wv[0, 1, 1 if named == 1 else 0]                                     # the named bucket's read count in vals (cr or cv)
            assert sorted(count[60:64].tolist()) == [0.0, 6.0, 9.0, 9.0]
        assert bin(seen).count("1") >= 3, seen


def test_records_of_libraries_that_do_not_exist(route):
    """third-allele records whose library is n_lib, n_lib + 1 or -1 beside a valid record of the same position (elements 10, 63, 64):
    fail, keep and vals are what the valid records alone give"""
    import handmade_views as hv
    L, Pn = 2, 130
    si = np.zeros((L, 2, 9, Pn), np.uint32); sf = np.zeros((L, 2, 4, Pn), np.float32)
    si[:, 0] = SLOT_I[0][None, :, None] * 3; si[:, 1] = SLOT_I[0][None, :, None]; sf[:, 0] = SLOT_F[0][None, :, None]; sf[:, 1] = SLOT_F[1][None, :, None]
    recs = []
    for t, x in enumerate((10, 63, 64)):
        for bad in (L, L + 1, -1):
            for b in (1, 2, 3):                              # the reference's bucket, the other slot's, a third allele
                recs.append(hv.record(x, bad, b, [50 + b] * 9, hv.f32bits([9.0] * 4).tolist()))
        recs.append(hv.record(x, t % L, 3, [5, 200, 100, 2, 3, 1, 90, 600, 150], hv.f32bits([2.0, 1.0, 3.0, 2.5]).tolist()))
    v, d, D, keep = raw_dense(route, np.full((L, Pn), 30), ts.high_slot_bytes(np.full((L, Pn), 1 | (2 << 8))), si, sf, recs[::-1], b"A" * Pn)
    assert D.istat[0, 3, 0, 10] == 5 and D.istat[1, 3, 0, 63] == 5 and D.istat[1, 3, 0, 10] == 0 and D.istat[0, 1, 0, 10] == 18
    t = dict(MID, min_var_count=2, min_var_rl=10.0, min_ref_rl=10.0)
    for idx in (np.arange(Pn), np.array([10, 10, 63, 64, 64])):
        wf, wk, wv, _ = check(route, v, d, D, idx, what="bad libraries", **t)
    assert wv[0, 2, 0, 0] == 5 and wv[1, 2, 0, 0] == 0 and wv[1, 2, 0, 2] == 5


def test_strand_and_frequency_of_counts_beyond_2_to_the_24(route):
    """P + M just above 2^24 and near 2^32 with P odd, counts and depths of that size: V_STRAND and V_FREQ are ONE fp32 division of the
    converted integers, (float)P / (float)(P + M) — the sum taken in integers.  Adding (float)P and (float)M instead rounds twice:
    the reference's side shows positions where that gives another quotient.  Hand-made views, so both routes run it."""
    Pn = 96
    rng = np.random.default_rng(21)
    plus = np.concatenate([[2 ** 24 + 1, 2 ** 24 + 3, 2 ** 24 - 1, 2 ** 31 + 1, 2 ** 32 - 1, 2 ** 32 - 3, 2 ** 25 + 1, 3],
                           rng.integers(2 ** 24, 2 ** 26, 44) | 1, rng.integers(2 ** 31, 2 ** 32, 44) | 1]).astype(np.uint32)
    minus = np.concatenate([[1, 2 ** 24 + 1, 5, 2 ** 31 - 3, 1, 2 ** 32 - 1, 2 ** 25 + 3, 2 ** 24 + 1],
                            rng.integers(1, 2 ** 24, 44), rng.integers(1, 2 ** 32, 44)]).astype(np.uint32)
    si = np.zeros((1, 2, 9, Pn), np.uint32)
    si[0, 0, 0] = 40; si[0, 0, 3] = 20; si[0, 0, 4] = 20
    si[0, 1, 0] = plus; si[0, 1, 3] = plus; si[0, 1, 4] = minus
    depth = np.maximum(plus, minus)[None, :] | np.uint32(2 ** 24 + 2)
    v, d, D, keep = raw_dense(route, depth, np.full((1, Pn), 1 | (2 << 8)), si, None, (), b"A" * Pn)
    wf, wk, wv, _ = check(route, v, d, D, np.arange(Pn), np.full(Pn, capi.WHY_C), what="large counts", **T_(min_strand_reads=1, strand_num=1, strand_den=3))
    S = plus.astype(np.uint64) + minus.astype(np.uint64)
    assert (S > 2 ** 24).all() and (S > 2 ** 32).sum() > 10 and (plus & 1).all()
    twice = plus.astype(F32) / (plus.astype(F32) + minus.astype(F32))
    strand = wv[0, 1, capi.VET_V_NAMES.index("strand")]
    assert np.array_equal(strand, plus.astype(F32) / S.astype(F32)) and (strand != twice).sum() >= 5, (strand != twice).sum()
    assert (wf[0, 1] & BIT["STRAND"]).any() and not (wf[0, 1] & BIT["STRAND"]).all()


# ------------------------------------------------------------------------------------------------ 6. the contract

def test_each_destination_alone_and_two_calls_identical(route):
    v, d, D, keep = shape_views(route)
    idx = np.sort(np.random.default_rng(4).integers(0, D.n_pos, 300))
    for want in (("fail",), ("keep",), ("vals",), ("fail", "keep"), ()):
        check(route, v, d, D, idx, what="want %r" % (want,), want=want, **MID)
    rc, st, gf, gk, gv = call(route, v, d, idx, want=(), status=False, **MID)
    assert rc == 0 and st == SENT and untouched(gf, gk, gv)
    a = call(route, v, d, idx, **MID); b = call(route, v, d, idx, **MID)
    assert a[0] == b[0] == 0 and all(x.tobytes() == y.tobytes() for x, y in zip(a[2:], b[2:]))
    t = route.vet.last_timing()
    assert t["kernel_s"] > 0 and t["bytes_read"] >= 4 * 300 * 2 * 28 and t["bytes_written"] >= 4 * 300 * (2 * 4 * (1 + NVAL) + 1)


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
    ok = dict(v=v, d=d, idx=[3, 5, 9])
    cases = [("no handle", dict(handle=False)), ("no view", dict(v=None)), ("no indels view", dict(d=None)), ("no parameters", dict(params=False)),
             ("no list", dict(no_idx=True)), ("n < 0", dict(n=-1)), ("dst_stride < n", dict(ds=2)),
             ("memory of the other kind", dict(v=av(memory=other), d=ad(memory=other))), ("memory 0", dict(v=av(memory=0), d=ad(memory=0))),
             ("views of two kinds", dict(d=ad(memory=other))), ("another device", dict(v=av(device=int(v.device) + 1), d=ad(device=int(v.device) + 1))),
             ("views of two devices", dict(v=av(device=int(v.device) + 1))), ("a view without planes", dict(v=av(si=None))),
             ("a view without planes (depth)", dict(v=av(depth=None))), ("not a view", dict(v=capi.DeviceView())),
             ("records without their arrays", dict(d=ad(slots=None))), ("records without the third-allele array", dict(v=av(xagg=None, n_xagg=5))),
             ("n_lib differs", dict(d=ad(n_lib=1))), ("pos0 differs", dict(d=ad(pos0=int(d.pos0) + 1))), ("n_pos differs", dict(d=ad(n_pos=P - 1))),
             ("a lib_on entry above 1", dict(lib_on=[1, 2])), ("no judged library", dict(lib_on=[0, 0])),
             ("freq_den 0", dict(freq_den=0)), ("strand_den 0", dict(strand_den=0)), ("unknown test bits", dict(tests=1 << 18)),
             ("unknown test bits beside known ones", dict(tests=7 | 1 << 30)), ("no workspace", dict(ws=False))]
    cases += [("%s = %r" % (k, x), dict(fields={k: x})) for k in capi.VET_FLOATS for x in (float("nan"), float("inf"))][::3]
    cases += [("min_var_bq = -inf", dict(fields=dict(min_var_bq=float("-inf"))))]
    for what, kw in cases:
        a = dict(ok, **kw)
        rc, st, gf, gk, gv = call(route, a.pop("v"), a.pop("d"), a.pop("idx"), **dict(MID, **a))
        assert rc == capi.E_ARG, what
        assert st == SENT and untouched(gf, gk, gv), "%s: something was written" % what
        if kw.get("handle", True):
            assert route.vet.lib.brc_vet_last_error(route.vet.h), what
    rc, st, gf, gk, gv = call(route, v, d, [], **MID)
    assert (rc, st) == (0, 0) and untouched(gf, gk, gv) and route.vet.lib.brc_vet_last_error(route.vet.h) == b""
    eng.close()


# ------------------------------------------------------------------------------------------------ 7. tensors.vet

def host_words(route, a):
    if route.name == "hip":
        a = a.cpu().numpy()
    return np.ascontiguousarray(a).view(np.uint32)


def check_vet(route, r, D, idx, alt, what, lib_on=None, tests=capi.VET_ALL_TESTS, **t):
    wf, wk, wv, wst = reference(D, idx, alt, lib_on, tests, **t)
    assert r["n"] == len(idx) and r["n_lib"] == D.n_lib and r["pos0"] == D.pos0, what
    assert np.array_equal(host_words(route, r["fail"]), wf) and np.array_equal(host_words(route, r["keep"]), wk), what
    assert np.array_equal(host_words(route, r["vals"]), wv.view(np.uint32)) and int(host_words(route, r["status"])[0]) == wst, what
    for k in ALL:
        assert isinstance(r[k], np.ndarray) if route.name == "sim" else r[k].is_cuda, (what, k)
    return wf, wk


def test_tensors_vet_on_text_only_engines_and_its_errors(route, oracle_lib, test_bam):
    from bam_readcount_amd import tensors
    beg0, end = 10403000, 10403700
    res, text = td.oracle_result(oracle_lib, test_bam, beg0, end, test_bam["ref"], tid=20, chrom="21")
    D = Dense.of(res)
    idx, why = select_list(D)
    assert len(idx) > 5
    for opts in (dict(text_only=True), dict(device_text="21")):
        eng = td.computed(route.engine_lib, test_bam, beg0, end, test_bam["ref"], tid=20, **opts)
        check_vet(route, tensors.vet(eng, route.vet, idx=idx, alt=why, **MID), D, idx, why, "before fetch %r" % opts, **MID)
        eng.fetch_result()
        assert eng.format_region("21") == text
        r = tensors.vet(eng, route.vet, idx=idx.tolist(), libs=[0], tests=("VAR_MAPQ", "DEPTH"), **MID)
        check_vet(route, r, D, idx, None, "after fetch %r" % opts, tests=BIT["VAR_MAPQ"] | BIT["DEPTH"], **MID)
        r = tensors.vet(eng, route.vet, idx=idx, want=("keep",), **MID)
        assert sorted(r) == ["keep", "n", "n_lib", "pos0", "status"]
        e = tensors.vet(eng, route.vet, idx=[])
        assert e["n"] == 0 and tuple(e["fail"].shape) == (1, 4, 0) and tuple(e["vals"].shape) == (1, 4, NVAL, 0)
        bad = [dict(idx=[5, 4]), dict(idx=[-1]), dict(idx=[res.n_pos]), dict(idx=idx, alt=[1]), dict(idx=idx, want=("nothing",)), dict(idx=idx, tests=("NOTHING",)),
               dict(idx=idx, tests=1 << 18), dict(idx=idx, libs=[]), dict(idx=idx, libs=[1]), dict(idx=idx, libs=["nobody"]), dict(idx=idx, freq_den=0),
               dict(idx=idx, strand_den=0), dict(idx=idx, min_depth=-1), dict(idx=idx, min_depth=1.5), dict(idx=idx, min_var_bq=float("nan")),
               dict(idx=idx, max_rl_diff=float("inf")), dict(idx=idx, max_rl_diff=1e39), dict(idx=idx, no_such_threshold=1)]
        for b in bad:
            with pytest.raises(ValueError):
                tensors.vet(eng, route.vet, **b)
        with pytest.raises(TypeError):
            tensors.vet(eng, route.vet)                     # (idx has no default)
        eng.close()


def test_the_chain_select_vet_sites(route, oracle_lib, low_region):
    """tensors.select -> tensors.vet(idx=sel["idx"], alt=sel["why"]) -> keep.nonzero() -> tensors.sites(positions=...), with device lists
    throughout on the GPU route: the panel holds the oracle's planes at the positions the reference predicate keeps"""
    from bam_readcount_amd import tensors
    import test_panel as tp
    panel = route.another("panel")
    ref, arrs, res = low_region
    D = Dense.of(res)
    eng = td.computed(route.engine_lib, arrs, 50, 2950, ref, **PER_LIB)
    sel = tensors.select(eng, route.select, indel=False, min_depth=0, min_alt=1)
    widx, wwhy = select_list(D, 1)
    assert sel["n"] == len(widx) > 20
    low = EASY_LOW
    r = tensors.vet(eng, route.vet, idx=sel["idx"], alt=sel["why"], **low)
    if route.name == "hip":
        assert sel["idx"].is_cuda and sel["why"].is_cuda
    wf, wk = check_vet(route, r, D, widx, wwhy, "chain", **low)
    kept = np.nonzero(wk)[0]
    assert 0 < len(kept) < len(widx)
    k = r["keep"].nonzero()[0] if route.name == "sim" else r["keep"].nonzero()[:, 0]
    p = tensors.sites(eng, panel, positions=sel["pos"][k], want=tensors.KINDS)
    want = tp.want_at(res, widx[kept])
    assert p["n"] == len(kept)
    for kind in tp.KINDS:
        assert np.array_equal(tp.host_words(route, p[kind]).reshape(want[kind].shape), want[kind]), kind
    assert int(tp.host_words(route, p["status"])[0]) == 0
    eng.close()


# ------------------------------------------------------------------------------------------------ 8. the host sanitizers

def _serialize(v, d, calls):
    """the host views and the calls as vet_check.cpp reads them"""
    b = ts._serialize(v, d, [])
    b = b[:36] + struct.pack("<i", len(calls)) + b[40:]
    for idx, alt, lib_on, tests, want, t in calls:
        idx = np.asarray(idx, np.int32)
        b += struct.pack("<qiiiI", idx.size, 0 if alt is None else 1, 0 if lib_on is None else 1, want, tests)
        b += struct.pack("<8I14f", *[t[k] for k in capi.VET_UINTS + capi.VET_FLOATS])
        b += idx.tobytes() + (np.asarray(alt, np.uint32).tobytes() if alt is not None else b"") + bytes(lib_on or [])
    return b


def _sanitized(tmp_path, name, v, d, D, calls):
    """vet_check_asan over one pair of host views: every call must return 0 without a report and give the reference's words, every
    destination that was not wanted as it was filled; returns the number of elements compared"""
    assert v.memory == capi.MEM_HOST and d.memory == capi.MEM_HOST
    case, out = str(tmp_path / (name + ".bin")), str(tmp_path / (name + ".res"))
    open(case, "wb").write(_serialize(v, d, calls))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    pr = subprocess.run([side.sim_checker(side.SIDE["vet"]), case, out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert pr.returncode == 0, (name, pr.stderr.decode()[-3000:])
    assert pr.stdout.decode().strip() == "%d calls" % len(calls), name
    raw = np.fromfile(out, np.uint32); o = 0
    L = D.n_lib
    some = 0
    for idx, alt, lib_on, tests, want, t in calls:
        n = len(idx)
        wf, wk, wv, wst = reference(D, idx, alt, lib_on, tests, **t)
        assert raw[o].view(np.int32) == 0 and raw[o + 1] == (wst if want & 8 else SENT), (name, n, raw[o:o + 2])
        o += 2
        for bit, w in ((1, wf), (2, wk), (4, wv.view(np.uint32))):
            g = raw[o:o + w.size]; o += w.size
            assert np.array_equal(g, w.ravel()) if want & bit else untouched(g), (name, n, bit)
        some += n
    assert o == raw.size, name
    return some


def test_calls_under_the_host_sanitizers(sim_route, tmp_path):
    """Hand-built views on the CPU build with -fsanitize=address,undefined, a stand-alone program: sources of exactly the views' sizes
    (the reference slice cut at ref_len, lib_on of exactly n_lib bytes), idx and alt of exactly n elements, a scratch of exactly
    brc_vet_workspace bytes, destinations of exactly [planes][n] — a load or store outside them is a report — and the results are the
    reference's.  Never under the gpu mark; nothing is loaded into python with a sanitizer."""
    route = sim_route
    rng = np.random.default_rng(2)
    some = 0
    for records in (True, False):
        v, d, D, keep = shape_views(route, records)
        calls = []
        for n in (0, 1, 63, 64, 65, 256, 257):
            idx = np.sort(rng.integers(0, D.n_pos, n))
            calls += [(idx, rng.integers(0, 64, n), None, capi.VET_ALL_TESTS, 15, MID), (idx, None, [1, 0], capi.VET_ALL_TESTS, 15, MID)]
        idx = np.arange(0, 300)
        calls += [(idx, None, None, BIT["RL_DIFF"], w, MID) for w in (1, 2, 4, 8, 0, 7)]
        calls += [([-1, 3, 9], None, None, 7, 15, MID), ([3, 9, D.n_pos], None, [0, 1], 7, 15, MID)]
        if not records:
            calls += [([5, 4, 300, 299, 699], None, None, capi.VET_ALL_TESTS, 15, MID)]
        some += _sanitized(tmp_path, "shapes%d" % records, v, d, D, calls)
    assert some > 2000
    v, d, D, keep, idx = two_record_views(route)
    _sanitized(tmp_path, "two", v, d, D, [(idx, None, None, capi.VET_ALL_TESTS, 15, MID), (idx[60:70], [15] * 10, [0, 1], capi.VET_ALL_TESTS, 15, MID)])
    for what, (v, d, h, keepalive), _ in ts.refchar_views(route):
        D = Dense.of_counts(h)
        _sanitized(tmp_path, "ref", v, d, D, [(np.arange(D.n_pos), None, None, capi.VET_ALL_TESTS, 15, T_(min_var_count=2))])
    v, d, D, keep = lib254_views(route)
    _sanitized(tmp_path, "lib254", v, d, D, [(np.arange(70), None, LIB254_ON, capi.VET_ALL_TESTS, 15, LIB254_T), (np.arange(70), None, None, 1, 3, LIB254_T)])
    v, d, D, keep = edge_views(route)
    _sanitized(tmp_path, "edge", v, d, D, [(np.arange(D.n_pos), np.full(D.n_pos, 2), None, capi.VET_ALL_TESTS, 15, MID)])
