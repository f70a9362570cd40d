"""Device-side site selection (include/brc_select.h): brc_select_sites and bam_readcount_amd.tensors.select against the header's integer
predicate written in numpy over the ORACLE's dense brc_result (depth, istat[..][BRC_I_N], refbase) and its indel list — idx and why
equal exactly, no tolerance.

Every body runs twice (the `route` fixture): [sim] = libbrc_sim.so + tests/sim_select/libbrc_select_sim.so, host memory, in the CPU
suite; [hip] = the product's libraries on the GPU (gpu-marked), lists, counts and scratch in device memory allocated through torch.
Destinations are filled with 0xA5A5A5A5 first: everything at or behind min(total, cap) must keep it.  The scratch has exactly
brc_select_workspace bytes.  The host sanitizers run the CPU build over the calls of the suite.

Where no engine can produce the shape — counts next to 2^32, 254 libraries, reference characters and slices of every kind, an exact
number of selected lanes per wave — the two views are built by hand (`build_views`) from dense counts, in the route's memory, and the
reference is the same numpy predicate over those dense counts.

Sizes that matter to the kernels (brc_select.hip): a wave is 64 consecutive positions, a workgroup and a scan tile 256, the scan of
the workgroups' counts takes 256 of them per pass — a window of more than 65536 positions makes it carry.

The condition "the wanted list is neither empty nor the whole window" is asserted on the oracle side for every whole-region case
(`check(..., proper=True)`); the windows and counts that the edge tests ask for by name (n = 1, no position selected, a full wave) are
exempt by their nature."""
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

PAD = 3                                   # elements of idx / why behind `cap`
SNV, INDEL, BOTH = capi.SELECT_SNV, capi.SELECT_INDEL, capi.SELECT_SNV | capi.SELECT_INDEL
U32 = 2 ** 32 - 1
PER_LIB = dict(lib_names=["libA", "libB"], per_lib=True)


def P_(flags=BOTH, min_depth=0, min_alt=1, frac=(0, 1), ctl_min_depth=0, ctl_max_alt=U32, ctl_frac=(1, 1)):
    return dict(flags=flags, min_depth=min_depth, min_alt=min_alt, frac=frac, ctl_min_depth=ctl_min_depth, ctl_max_alt=ctl_max_alt, ctl_frac=ctl_frac)


LIBS = ("dense", "select")


@pytest.fixture(scope="module", params=["sim", pytest.param("hip", marks=pytest.mark.gpu)])
def route(request):
    return Route(request.param, LIBS, engine=True)


# ------------------------------------------------------------------------------------------------ the reference predicate

_REFCODE = np.full(256, -1, np.int64)
for _i, _c in enumerate("ACGT"):
    _REFCODE[ord(_c)] = _REFCODE[ord(_c.lower())] = _i


def reference(depth, cnt, refbase, indels, pos0, role, p, k0, n):
    """The header's predicate on dense data: depth [L, P], cnt [L, 4, P] (A C G T read counts), refbase: P characters, indels:
    (pos, lib, len, count) records -> (idx int64 [m], why int64 [m]) of the window [k0, k0 + n)"""
    L = depth.shape[0]
    role = np.ones(L, np.int64) if role is None else np.asarray(role, np.int64)
    case, ctl = role == 1, role == 2
    u = np.uint64
    D = depth[:, k0:k0 + n].astype(u)
    c = cnt[:, :, k0:k0 + n].astype(u)
    Db = D[:, None, :]
    case_ok = (Db >= u(p["min_depth"])) & (c >= u(p["min_alt"])) & (c * u(p["frac"][1]) >= u(p["frac"][0]) * Db)
    ctl_ok = (Db >= u(p["ctl_min_depth"])) & (c <= u(p["ctl_max_alt"])) & (c * u(p["ctl_frac"][1]) <= u(p["ctl_frac"][0]) * Db)
    why = np.zeros(n, np.int64)
    if p["flags"] & SNV:
        ok = case_ok[case].any(axis=0) & ctl_ok[ctl].all(axis=0)                      # [4, n]
        rb = _REFCODE[np.frombuffer(bytes(refbase), np.uint8)[k0:k0 + n]]
        for b in range(4):
            why |= (ok[b] & (rb >= 0) & (rb != b)).astype(np.int64) << b
    if p["flags"] & INDEL:
        cand = np.zeros((2, n), bool); veto = np.zeros((2, n), bool)
        for pos, lib, ln, count in indels:
            j = pos - pos0 - k0
            if ln == 0 or not 0 <= j < n:
                continue
            d, s = int(depth[lib, k0 + j]), 0 if ln > 0 else 1
            if role[lib] == 1 and d >= p["min_depth"] and count >= p["min_alt"] and count * p["frac"][1] >= p["frac"][0] * d:
                cand[s, j] = True
            if role[lib] == 2 and (count > p["ctl_max_alt"] or count * p["ctl_frac"][1] > p["ctl_frac"][0] * d):
                veto[s, j] = True
        shallow = (D[ctl] < u(p["ctl_min_depth"])).any(axis=0)
        for s in range(2):
            why |= (cand[s] & ~veto[s] & ~shallow).astype(np.int64) << (4 + s)
    sel = np.nonzero(why)[0]
    return sel + k0, why[sel]


class Dense:
    """what the reference predicate reads, from an oracle result or from hand-made arrays"""

    def __init__(self, depth, cnt, refbase, indels, pos0):
        self.depth, self.cnt, self.refbase, self.indels, self.pos0 = depth, cnt, refbase, indels, pos0
        self.n_pos, self.n_lib = depth.shape[1], depth.shape[0]

    @classmethod
    def of(cls, res):
        return cls(res.depth, res.istat[:, 1:5, 0, :], res.refbase, [(d["pos"], d["lib"], d["len"], int(d["i"][0])) for d in res.indels], res.pos0)

    def want(self, role, p, k0=0, n=None):
        return reference(self.depth, self.cnt, self.refbase, self.indels, self.pos0, role, p, k0, self.n_pos - k0 if n is None else n)


# ------------------------------------------------------------------------------------------------ calling the library

def call(route, v, d, role, p, k0, n, cap, want=("idx", "why", "counts"), handle=True, params=True, ws=True):
    """brc_select_sites into sentinel-filled buffers of cap + PAD elements and a scratch of exactly brc_select_workspace bytes;
    returns (rc, counts word, idx words, why words)"""
    par, keep = capi.select_params(role, p["flags"], p["min_depth"], p["min_alt"], p["frac"], p["ctl_min_depth"], p["ctl_max_alt"], p["ctl_frac"])
    c = max(cap, 0)
    bi, bw, bc = route.sentinel_words(c + PAD), route.sentinel_words(c + PAD), route.sentinel_words(1)
    wsb = route.select.workspace(v, d, n) if v is not None and d is not None else 0
    bs = route.sentinel_words(wsb // 4)
    assert wsb % 4 == 0
    rc = route.select.lib.brc_select_sites(route.select.h if handle else None, C.byref(v) if v is not None else None, C.byref(d) if d is not None else None,
                                           C.byref(par) if params else None, k0, n, cap, route.ptr(bi) if "idx" in want else None,
                                           route.ptr(bw) if "why" in want else None, route.ptr(bc) if "counts" in want else None,
                                           route.ptr(bs) if ws and wsb else None, None)
    del keep
    return rc, int(route.words(bc)[0]), route.words(bi)[:c + PAD].copy(), route.words(bw)[:c + PAD].copy()


def check(route, v, d, dense, role, p, k0=0, n=None, what="", proper=False, caps=None):
    """counts alone, then the list at cap = total (and at `caps`), against the reference; returns the wanted (idx, why)"""
    n = dense.n_pos - k0 if n is None else n
    widx, wwhy = dense.want(role, p, k0, n)
    m = len(widx)
    if proper:
        assert 0 < m < n, "%s: the reference selects %d of %d positions: choose other thresholds" % (what, m, n)
    rc, total, gi, gw = call(route, v, d, role, p, k0, n, 0, want=("counts",))
    assert rc == 0, (what, route.select.lib.brc_select_last_error(route.select.h))
    assert total == m, (what, total, m)
    assert (gi == SENT).all() and (gw == SENT).all(), what
    for cap in [m] + list(caps or []):
        rc, total, gi, gw = call(route, v, d, role, p, k0, n, cap)
        t = min(m, cap)
        assert rc == 0 and total == m, (what, cap, rc, total)
        assert np.array_equal(gi[:t].view(np.int32), widx[:t].astype(np.int32)), (what, cap, gi[:8], widx[:8])
        assert np.array_equal(gw[:t], wwhy[:t].astype(np.uint32)), (what, cap, gw[:8], wwhy[:8])
        assert (gi[t:] == SENT).all() and (gw[t:] == SENT).all(), "%s: wrote behind the list (cap %d)" % (what, cap)
    return widx, wwhy


def views_of(eng):
    v, d = eng.device_view(), eng.device_indels()
    assert (v.n_lib, v.pos0, v.n_pos, v.memory) == (d.n_lib, d.pos0, d.n_pos, d.memory)
    return v, d


# ------------------------------------------------------------------------------------------------ hand-made views

NONE32 = 0xFFFFFFFF


def build_views(route, depth, cnt, ref=None, ref_lo=0, ref_len=None, indels=(), pos0=0, dead=3, spill="xagg"):
    """A brc_device_view + brc_device_indels in the route's memory that expand to the dense counts given: depth [L, P], cnt [L, 4, P]
    (A C G T).  Per (library, position) the first two non-zero buckets go to the two slots, the others to third-allele records
    (shuffled, with `dead` unused records among them); `indels` (pos, lib, len, count) become 72-byte records between `dead` unused
    ones.  ref: the bytes of the slice [ref_lo, ref_lo + len(ref)) or None.  Returns (view, indels view, Dense, keepalive)."""
    depth = np.asarray(depth, np.uint32); cnt = np.asarray(cnt, np.uint32)
    L, Pn = depth.shape
    PS = (Pn + 63) // 64 * 64
    rng = np.random.default_rng(L * 1000 + Pn)

    def planes(a, k):
        out = np.zeros((k, PS), a.dtype); out[:, :Pn] = a.reshape(k, Pn); return out
    slotid = np.full((L, Pn), 0xFFFF, np.uint32)
    si = np.zeros((L, 2, 9, Pn), np.uint32); sf = np.zeros((L, 2, 4, Pn), np.float32)
    recs = []
    for l, k in zip(*np.nonzero((cnt != 0).any(axis=1))):
        nz = [b for b in range(4) if cnt[l, b, k]]
        if len(nz) == 4:
            nz = [nz[3], nz[0], nz[2], nz[1]]                                  # (slot order is not bucket order)
        sid = 0xFFFF
        for s, b in enumerate(nz[:2]):
            sid = (sid & ~(0xFF << (8 * s))) | ((b + 1) << (8 * s))
            si[l, s, 0, k] = cnt[l, b, k]
        slotid[l, k] = sid
        for b in nz[2:]:
            recs.append((k, (l << 8) | (b + 1), cnt[l, b, k]))
    for _ in range(dead if recs else 0):
        recs.append((NONE32, 0, 7))
    recs = [recs[i] for i in rng.permutation(len(recs))]
    xagg = np.zeros((len(recs), 16), np.uint32)
    for r, (k, lb, c) in enumerate(recs):
        xagg[r, 0], xagg[r, 1], xagg[r, 2] = k, lb, c
    slots = [(p, l, ln, c) for p, l, ln, c in indels] + [(pos0 + 1, 0, 0, 99)] * (dead if len(indels) else 0)
    slots = [slots[i] for i in rng.permutation(len(slots))]
    srec = np.zeros((len(slots), 18), np.uint32)
    for r, (p, l, ln, c) in enumerate(slots):
        srec[r, 0], srec[r, 1], srec[r, 2], srec[r, 5] = np.int64(p) & U32, l, np.int64(ln) & U32, c
    keep = {"ncol": route.put(planes(depth, L)), "depth": route.put(planes(depth, L)), "slotid": route.put(planes(slotid, L)),
            "si": route.put(planes(si, L * 18)), "sf": route.put(planes(sf, L * 8)), "xagg": route.put(xagg), "slots": route.put(srec),
            "one": route.put(np.zeros(8, np.uint8))}
    v = capi.DeviceView(route.mem, 0, L, pos0, Pn, PS, *[route.ptr(keep[k]) for k in ("ncol", "depth", "slotid", "si")], None, route.ptr(keep["sf"]),
                        route.ptr(keep["xagg"]) if len(recs) else None, len(recs))
    d = capi.DeviceIndels(route.mem, 0, L, pos0, Pn, route.ptr(keep["slots"]) if len(slots) else None, len(slots))
    if len(slots):
        d.seq4 = d.seq_off = d.l_qseq = route.ptr(keep["one"])
    rl = pos0 + Pn if ref_len is None else ref_len
    refbase = bytearray(b"N" * Pn)
    if ref is not None:
        keep["ref"] = route.put(np.frombuffer(bytes(ref), np.uint8))
        d.ref, d.ref_lo, d.ref_hi, d.ref_len = route.ptr(keep["ref"]), ref_lo, ref_lo + len(ref), rl
        for k in range(Pn):
            p = pos0 + k
            if ref_lo <= p < ref_lo + len(ref) and p < rl and ref[p - ref_lo] != 0:
                refbase[k] = ref[p - ref_lo]
    return v, d, Dense(depth, cnt, bytes(refbase), list(indels), pos0), keep


def raw_views(route, depth, slotid, si, sf=None, records=(), indels=(), ref=None, pos0=0):
    """The compact form written down, nothing derived and nothing shuffled: depth, slotid [L, P], si [L, 2, 9, P], sf [L, 2, 4, P]
    (float32), third-allele records (handmade_views.record) and indel records (pos, lib, len, count) in the order given, libraries
    outside [0, L) included; ref: the reference characters of the P positions.  Returns (view, indels view, istat [L, 6, 9, P],
    fstat [L, 6, 4, P] float32 — what the view expands to by handmade_views.expand_reference, the plain loops — refbase, keepalive)."""
    import handmade_views as hv
    depth = np.asarray(depth, np.uint32)
    L, Pn = depth.shape
    sf = np.zeros((L, 2, 4, Pn), np.float32) if sf is None else np.ascontiguousarray(sf, np.float32)
    A = {"ncol": depth, "depth": depth, "slotid": np.asarray(slotid, np.uint32), "si": np.asarray(si, np.uint32), "sf": sf.view(np.uint32), "unavail": None}
    v, keep = hv.make_view(route, A, list(records), pos0=pos0)
    want = hv.expand_reference(A, list(records))
    istat = want["istat"].reshape(L, 6, 9, Pn); fstat = want["fstat"].view(np.float32).reshape(L, 6, 4, Pn)
    srec = np.zeros((len(indels), 18), np.uint32)
    for r, (p, l, ln, c) in enumerate(indels):
        srec[r, 0], srec[r, 1], srec[r, 2], srec[r, 5] = np.int64(p) & U32, np.int64(l) & U32, np.int64(ln) & U32, c
    keep["slots"] = route.put(srec); keep["one"] = route.put(np.zeros(8, np.uint8))
    d = capi.DeviceIndels(route.mem, 0, L, pos0, Pn, route.ptr(keep["slots"]) if len(indels) else None, len(indels))
    if len(indels):
        d.seq4 = d.seq_off = d.l_qseq = route.ptr(keep["one"])
    refbase = b"N" * Pn
    if ref is not None:
        assert len(ref) == Pn
        keep["ref"] = route.put(np.frombuffer(bytes(ref), np.uint8))
        d.ref, d.ref_lo, d.ref_hi, d.ref_len = route.ptr(keep["ref"]), pos0, pos0 + Pn, pos0 + Pn
        refbase = bytes(ref)
    return v, d, istat, fstat, refbase, keep


def low_depth(P, L=2, seed=1, alt=0.08, ref=None):
    """dense counts of a low-depth region: depth 0..12, most of it on the reference base, now and then an alternative allele or two"""
    rng = np.random.default_rng(seed)
    ref = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=P).tobytes() if ref is None else ref
    rb = np.maximum(_REFCODE[np.frombuffer(ref, np.uint8)], 0)
    cnt = np.zeros((L, 4, P), np.uint32)
    cnt[:, rb, np.arange(P)] = rng.integers(0, 10, (L, P))
    for _ in range(3):
        m = rng.random((L, P)) < alt
        b = rng.integers(0, 4, (L, P))
        for l in range(L):
            k = np.nonzero(m[l])[0]
            cnt[l, b[l, k], k] += rng.integers(1, 4, k.size).astype(np.uint32)
    depth = cnt.sum(axis=1).astype(np.uint32)
    return depth, cnt, ref


# ------------------------------------------------------------------------------------------------ 1. the golden fixtures

@pytest.fixture(scope="module")
def low_region(oracle_lib):
    """a synthetic low-depth region of two libraries and the oracle's result of it"""
    rng = np.random.default_rng(11)
    ref = synth.make_ref(rng, 3000, weird=0.01)
    arrs = synth.make_batch(77, ref, 260, read_len=(60, 120), style="indel", n_libs=2, mismatch=0.06)
    res, _ = td.oracle_result(oracle_lib, arrs, 50, 2950, ref, **PER_LIB)
    return ref, arrs, res


FIXTURE_PARAMS = [("snv", P_(SNV, min_depth=8, min_alt=2, frac=(1, 10), ctl_max_alt=1, ctl_frac=(1, 20))),
                  ("indel", P_(INDEL, min_depth=4, min_alt=1, frac=(1, 50), ctl_max_alt=0)),
                  ("both", P_(BOTH, min_depth=6, min_alt=2, frac=(1, 20), ctl_min_depth=2, ctl_max_alt=2, ctl_frac=(1, 4)))]


def test_golden_fixtures_whole(route, oracle_lib, test_bam, twolib, low_region):
    """test_bam.npz all-lib; twolib.npz -p with libA case / libB control and the reverse; SNV only, indel only, both.
    twolib.npz holds NO non-reference evidence at all — its deepest position has depth 1 per library, no read differs from the reference
    and the oracle reports no indel record — so no threshold can make its list non-empty: it runs all the same (the list is empty on
    both sides), and the two-library synthetic batch `low_region` stands in for it where the list has to be proper.  It also sets the
    deletion bit, which test_bam.npz lacks."""
    seen = 0
    beg0, end = 10402736, 10405248
    res, _ = td.oracle_result(oracle_lib, test_bam, beg0, end, test_bam["ref"], tid=20)
    eng = td.computed(route.engine_lib, test_bam, beg0, end, test_bam["ref"], tid=20)
    v, d = views_of(eng)
    for name, p in FIXTURE_PARAMS:
        _, why = check(route, v, d, Dense.of(res), None, p, what="test_bam " + name, proper=True)
        seen |= int(np.bitwise_or.reduce(why))
    eng.close()
    names = [str(s) for s in twolib["lib_names"]]
    opts = dict(lib_names=names, per_lib=True, insertion_centric=True, ref_len_check=True)
    end = int(twolib["ref"].size)
    res, _ = td.oracle_result(oracle_lib, twolib, 0, end, twolib["ref"], **opts)
    assert res.n_lib == 2 and res.depth.max() == 1 and not res.indels
    eng = td.computed(route.engine_lib, twolib, 0, end, twolib["ref"], **opts)
    v, d = views_of(eng)
    for role in ([1, 2], [2, 1]):
        for name, p in TWOLIB_PARAMS:
            idx, _ = check(route, v, d, Dense.of(res), role, p, what="twolib %r %s" % (role, name))
            assert len(idx) == 0
    eng.close()
    ref, arrs, res = low_region
    eng = td.computed(route.engine_lib, arrs, 50, 2950, ref, **PER_LIB)
    v, d = views_of(eng)
    for role in ([1, 2], [2, 1]):
        for name, p in TWOLIB_PARAMS:
            _, why = check(route, v, d, Dense.of(res), role, p, what="two synthetic libraries %r %s" % (role, name), proper=True)
            seen |= int(np.bitwise_or.reduce(why))
    eng.close()
    assert seen == 63, "the parameter sets leave a bit of the reason word unset: %d" % seen


TWOLIB_PARAMS = [("snv", P_(SNV, min_depth=1, min_alt=1, ctl_max_alt=0)), ("indel", P_(INDEL, min_depth=1, min_alt=1, ctl_max_alt=0)),
                 ("both", P_(BOTH, min_depth=2, min_alt=1, frac=(1, 10), ctl_frac=(1, 2)))]


# ------------------------------------------------------------------------------------------------ 2. third alleles

def test_third_allele_counts_sit_in_records_only(route, oracle_lib, monkeypatch):
    """The knob libraries under BRC_FORCE_DOM=3 + BRC_XEV_CAP=1: a selected position whose qualifying count is in neither slot of the
    view, and one with records in two libraries of which the control's vetoes."""
    monkeypatch.setenv("BRC_FORCE_DOM", "3"); monkeypatch.setenv("BRC_XEV_CAP", "1")
    ref, arrs = td.third_allele_inputs()
    opts = dict(PER_LIB, min_bq=10)
    res, _ = td.oracle_result(oracle_lib, arrs, 0, 2000, ref, **opts)
    eng = td.computed(route.knob_lib, arrs, 0, 2000, ref, **opts)
    v, d = views_of(eng)
    assert v.n_xagg > 0
    dense = Dense.of(res)
    # the view's slots, through the dense library with the records taken away
    bare = capi.DeviceView.from_buffer_copy(v); bare.n_xagg = 0
    rc, slots = td.expand(route, bare, 0, res.n_pos, res.n_pos, kinds=("istat",))
    assert rc == 0
    in_slots = slots["istat"].reshape(2, 6, 9, res.n_pos)[:, 1:5, 0, :]
    only_rec = (in_slots != dense.cnt) & (dense.cnt != 0)                              # [L, 4, P]: counts that exist only in a record
    assert only_rec.any()
    p = P_(SNV, min_depth=4, min_alt=1, ctl_max_alt=0)
    for role in ([1, 2], [2, 1], None):
        idx, why = check(route, v, d, dense, role, p, what="third alleles %r" % (role,), proper=True)
        case = [l for l in range(2) if role is None or role[l] == 1]
        hit = [(k, b) for k, w in zip(idx, why) for b in range(4) if w >> b & 1 and any(only_rec[l, b, k] for l in case)]
        assert hit, "no selected position owes its bit to a record (%r)" % (role,)
    # records in two libraries at one position, the control's count vetoing: selected with the control ignored, not with it
    both = np.nonzero(only_rec.any(axis=1).all(axis=0))[0]
    assert both.size, "no position with records in both libraries"
    w1 = dict(zip(*dense.want([1, 0], p))); w2 = dict(zip(*dense.want([1, 2], p)))
    vetoed = [k for k in both if any(w1.get(k, 0) >> b & 1 and not w2.get(k, 0) >> b & 1 and only_rec[1, b, k] for b in range(4))]
    assert vetoed, "no position where the control library's record vetoes"
    check(route, v, d, dense, [1, 0], p, what="control ignored")
    eng.close()


# ------------------------------------------------------------------------------------------------ 3. shapes

def window_list(P):
    return [(0, P), (3, 61), (63, 130), (64, 64), (65, 1), (5, 63), (5, 64), (5, 65), (7, 257), (0, 1), (P - 1, 1), (P - 77, 77), (130, P - 130)]


EDGE_P = P_(BOTH, min_depth=3, min_alt=2, frac=(1, 5), ctl_max_alt=1)


def test_windows_off_the_grid(route, low_region):
    ref, arrs, res = low_region
    eng = td.computed(route.engine_lib, arrs, 50, 2950, ref, **PER_LIB)
    v, d = views_of(eng)
    dense = Dense.of(res)
    P = res.n_pos
    assert P > 2000
    for role in ([1, 2], None):
        check(route, v, d, dense, role, EDGE_P, what="whole %r" % (role,), proper=True)
        for k0, n in window_list(P):
            check(route, v, d, dense, role, EDGE_P, k0, n, what="window %r" % ((k0, n),))
    eng.close()


def test_site_list_axis_never_selects_empty_positions(route, oracle_lib, low_region):
    ref, arrs, res = low_region
    dense = Dense.of(res)
    p = P_(BOTH, min_depth=1, min_alt=1)
    full, _ = dense.want(None, p)
    wins = [(300, 301), (640, 710), (full[len(full) // 2] + res.pos0, full[len(full) // 2] + res.pos0 + 1), (2000, 2064)]
    wins = sorted(wins)
    b = np.array([w[0] for w in wins], np.int32); e = np.array([w[1] for w in wins], np.int32)
    eng = capi.Engine(route.engine_lib, **PER_LIB)
    eng.begin_region(0, 50, 2950, ref)
    eng.push_reads(capi.select_reads(arrs, capi.fetch_overlapping(arrs, capi.read_ends(arrs), 49, 2950)))
    eng.region_windows(b, e)
    eng.upload(); eng.compute()
    v, d = views_of(eng)
    rc, total, gi, gw = call(route, v, d, None, p, 0, res.n_pos, res.n_pos)
    assert rc == 0
    got = dict(zip(gi[:total].view(np.int32).tolist(), gw[:total].tolist()))
    want = dict(zip(full.tolist(), dense.want(None, p)[1].tolist()))
    announced = np.concatenate([np.arange(x, y) for x, y in wins]) - res.pos0
    hit = [k for k in announced if k in want]
    assert hit and len(want) > len(hit)
    for k in announced:                     # announced positions: as the unhinted oracle
        assert got.get(int(k), 0) == want.get(int(k), 0), k
    rc, depth = td.expand(route, v, 0, res.n_pos, res.n_pos, kinds=("depth", "ncol"))
    empty = (depth["ncol"] == 0).all(axis=0)
    assert empty.sum() > res.n_pos // 2 and not any(empty[k] for k in got), "an EMPTY position was selected"
    eng.close()


WAVE_P = P_(SNV, min_depth=5, min_alt=2, frac=(1, 10))


def wave_views(route):
    """hand-made views of one library and no third-allele record: (name, the positions that carry three reads of G on a reference of
    A, views)"""
    P = 1000
    base = np.zeros((1, 4, P), np.uint32); base[0, 0] = 9                               # everything on the reference base A
    ref = b"A" * P
    layouts = {"none": [], "lead alone": [0], "last": [P - 1], "64 = one wave": list(range(128, 192)), "65": list(range(127, 192)),
               "257": list(range(300, 557)), "a wave and its neighbours": list(range(64, 128)) + list(range(192, 256)),
               "every second": list(range(1, P, 2))}
    for name, ks in layouts.items():
        cnt = base.copy(); cnt[0, 2, ks] = 3
        yield name, ks, build_views(route, cnt.sum(axis=1), cnt, ref)


def test_selected_counts_and_full_waves(route):
    """hand-made views: 0, 1, 64, 65 and 257 selected positions; a wave with all 64 lanes selected next to one with none; the lead
    position alone; the last position"""
    for name, ks, (v, d, dense, keep) in wave_views(route):
        assert v.n_xagg == 0 and not v.xagg                                             # (the scratch without head and next)
        idx, why = check(route, v, d, dense, None, WAVE_P, what=name, caps=[1, 64])
        assert idx.tolist() == ks and (why == capi.WHY_G).all(), name
        if name == "257":
            check(route, v, d, dense, None, WAVE_P, 299, 259, what="257 in a window of 259")


def test_scan_carry_over_more_than_256_workgroups(route, oracle_lib):
    """70000 positions = 274 workgroups: the scan of their counts takes two passes and carries"""
    rng = np.random.default_rng(5)
    ref = synth.make_ref(rng, 70100)
    arrs = synth.make_batch(31, ref, 3000, read_len=(60, 120), style="indel", mismatch=0.05)
    res, _ = td.oracle_result(oracle_lib, arrs, 50, 70050, ref)
    eng = td.computed(route.engine_lib, arrs, 50, 70050, ref)
    v, d = views_of(eng)
    assert res.n_pos > 256 * 256 + 256
    idx, _ = check(route, v, d, Dense.of(res), None, P_(BOTH, min_depth=2, min_alt=1, frac=(1, 4)), what="70000 positions", proper=True)
    assert (idx > 256 * 256).sum() > 64 and (idx < 256 * 256).sum() > 64
    eng.close()


# ------------------------------------------------------------------------------------------------ 4. arithmetic

THRESHOLD_SETS = [P_(SNV, min_alt=1, frac=(1, 5)), P_(SNV, min_alt=1, frac=(5, 25), ctl_frac=(2, 22)), P_(SNV, min_alt=1, frac=(0, 7)),
                  P_(SNV, min_alt=1, ctl_max_alt=0), P_(SNV, min_alt=3, min_depth=25, ctl_min_depth=22, ctl_max_alt=2), P_(SNV, min_alt=1, ctl_frac=(0, 1))]


def threshold_views(route):
    P = 130
    ref = b"C" * P
    cnt = np.zeros((2, 4, P), np.uint32)
    cnt[:, 1] = 17                                                                      # reference base C
    cnt[0, 3, :] = np.arange(P) % 8                                                     # case library: T counts 0..7
    cnt[1, 3, :] = (np.arange(P) // 8) % 4                                              # control library: T counts 0..3
    depth = cnt.sum(axis=1).astype(np.uint32) + np.array([[3], [3]], np.uint32)         # D = 20 + c: c = 5 of D = 25 is exactly 1 / 5
    return build_views(route, depth, cnt, ref)


def test_thresholds_met_exactly(route):
    """c * den == num * D on the case and on the control side; frac_num = 0; ctl_max_alt = 0"""
    v, d, dense, keep = threshold_views(route)
    sets = THRESHOLD_SETS
    for p in sets:
        idx, _ = check(route, v, d, dense, [1, 2], p, what=repr(p), proper=True)
    idx, _ = dense.want([1, 2], sets[0])
    assert 5 in idx and 4 not in idx                                                    # 5 / 25 passes, 4 / 24 does not
    idx, _ = dense.want([1, 2], sets[1])
    assert 21 in idx and 29 not in idx                                                  # control: 2 / 22 passes, 3 / 23 does not


@pytest.fixture(scope="module")
def sim_route():
    return Route("sim", LIBS, engine=True)


BIG_SETS = [P_(SNV, min_depth=U32, min_alt=2 ** 31, frac=(U32 - 1, U32), ctl_frac=(1, 4)), P_(SNV, min_alt=U32 - 5 * 2 ** 26, frac=(2 ** 31, U32)),
            P_(SNV, min_alt=1, frac=(3, 4), ctl_max_alt=2 ** 30, ctl_frac=(2 ** 16, 2 ** 18 + 1)), P_(SNV, min_alt=1, frac=(2 ** 16 + 1, 2 ** 16 + 2))]


def big_views(route):
    P = 64
    ref = b"G" * P
    cnt = np.zeros((2, 4, P), np.uint32)
    big = np.uint32(U32)
    cnt[0, 0, :] = big - np.arange(P, dtype=np.uint32) * np.uint32(2 ** 26)
    cnt[1, 0, :] = np.arange(P, dtype=np.uint32) * np.uint32(2 ** 25)
    depth = np.full((2, P), big, np.uint32)
    return build_views(route, depth, cnt, ref)


def test_counts_next_to_two_to_the_32(sim_route):
    """hand-made BRC_MEM_HOST views (the CPU build alone: no engine counts that far): products that do not fit 32 bits"""
    route = sim_route
    v, d, dense, keep = big_views(route)
    cnt = dense.cnt
    for p in BIG_SETS:
        check(route, v, d, dense, [1, 2], p, what=repr(p), proper=True)
    # with 32-bit products the first set would select nothing or everything: the reference itself shows the difference
    p = BIG_SETS[3]
    c = cnt[0, 0].astype(np.uint64)
    wrapped = (c * np.uint64(p["frac"][1]) & np.uint64(U32)) >= (np.uint64(p["frac"][0]) * np.uint64(U32) & np.uint64(U32))
    assert wrapped.sum() != len(dense.want([1, 2], p)[0])


REFCHAR_P = P_(SNV, min_alt=2)
SLICES = ((1010, 10 ** 6), (990, 1030), (1000, 1000), (1002, 1020), (2000, 10 ** 6))                  # (ref_lo, ref_len) of a 40-character slice


def refchar_views(route):
    """(what, views, parameters): every kind of reference character, four to each; no reference but an insertion; a 40-character
    slice that starts behind the planes' start, ends before their end, or belongs to a reference that ends first"""
    chars = b"ACGTacgtNnRYKMSWBDHVryU\x00.-*=" + bytes([0xC1, 0xE1, 0x01, 0x21])
    P = len(chars) * 4
    ref = bytes(chars[k // 4] for k in range(P))
    cnt = np.zeros((1, 4, P), np.uint32)
    cnt[0, np.arange(P) % 4, np.arange(P)] = 4                                          # position k carries base k % 4
    depth = np.full((1, P), 6, np.uint32)
    yield "characters", build_views(route, depth, cnt, ref, pos0=1000, ref_lo=1000), REFCHAR_P
    yield "no reference", build_views(route, depth, cnt, None, pos0=1000, indels=[(1005, 0, 2, 3)]), P_(BOTH, min_alt=2)
    for lo, rl in SLICES:
        yield "slice %r" % ((lo, rl),), build_views(route, depth[:, :60], cnt[:, :, :60], b"ACGT" * 10, pos0=1000, ref_lo=lo, ref_len=rl), REFCHAR_P


def test_reference_characters_and_slices(route):
    """acgt, N, IUPAC codes, NUL; no reference at all; positions outside the slice and past ref_len"""
    cases = list(refchar_views(route))
    what, (v, d, dense, keep), p = cases[0]
    idx, why = check(route, v, d, dense, None, p, what=what, proper=True)
    assert len(idx) == 8 * 3                                                            # ACGTacgt x the three other bases
    # no reference: nothing can be an SNV; an indel still is one
    what, (v, d, dense, keep), p = cases[1]
    assert not d.ref
    idx, why = check(route, v, d, dense, None, p, what=what)
    assert idx.tolist() == [5] and why.tolist() == [capi.WHY_INS]
    # a slice that starts behind the planes' start and a reference that ends before the slice does
    for (lo, rl), (what, (v, d, dense, keep), p) in zip(SLICES, cases[2:]):
        idx, _ = check(route, v, d, dense, None, p, what=what)
        assert all(lo <= 1000 + k < min(lo + 40, rl) for k in idx) and (len(idx) > 0) == (lo < 1060 and rl > 1000 and lo + 40 > 1000)


LIB254_CALLS = [([1 + (l % 2) for l in range(254)], P_(BOTH, min_depth=3, min_alt=3, ctl_max_alt=2)),
                ([1 + (l % 2) for l in range(254)], P_(BOTH, min_depth=3, min_alt=2, ctl_max_alt=2, ctl_frac=(1, 3))),
                ([1] + [0] * 252 + [2], P_(BOTH, min_depth=3, min_alt=2, ctl_max_alt=0))]


def lib_pattern(mod, L=254):
    """a per-library value 0 .. mod - 1 from the bits of x = l * 37 % 251, (x >> 1 ^ x >> 4) % mod: the pattern differs from itself
    shifted by 16, 32, 64 and 128 libraries at a quarter of the libraries or more, so a role or lib_on table that is indexed modulo a
    power of two gives another table (select, vet, ivet and runs share it)"""
    pat = [(((l * 37 % 251) >> 1) ^ ((l * 37 % 251) >> 4)) % mod for l in range(L)]
    for shift in (16, 32, 64, 128):
        assert sum(pat[l] != pat[l - shift] for l in range(shift, L)) >= (L - shift) // 4, shift
    return pat


def high_slot_bytes(slotid):
    """slotid [L, 130] with bit 7 set in slot 0's byte at positions 100 .. 109 and in slot 1's byte from 110 on: 0x81 .. 0x85 name no
    bucket (a mask of seven bits would read them as 1 .. 5), so those slots' sums belong to nothing"""
    slotid = np.array(slotid, np.uint32)
    slotid[:, 100:110] |= 0x80; slotid[:, 110:] |= 0x8000
    return slotid


def folded(pat, period):
    """the table an index folded to `period` libraries reads"""
    return [pat[l % period] for l in range(len(pat))]


def lib254_views(route):
    depth, cnt, ref = low_depth(70, L=254, seed=3, alt=0.02)
    return build_views(route, depth, cnt, ref, indels=[(7, 253, -2, 3), (7, 1, -1, 1), (9, 252, 4, 2)])


def test_254_libraries_with_alternating_roles(route):
    v, d, dense, keep = lib254_views(route)
    for role, p in LIB254_CALLS:
        assert len(role) == v.n_lib == 254                                              # (the role array has exactly Lp bytes)
        check(route, v, d, dense, role, p, what="254 libraries", proper=True)
    # one library more is refused
    v2 = capi.DeviceView.from_buffer_copy(v); d2 = capi.DeviceIndels.from_buffer_copy(d); v2.n_lib = d2.n_lib = 255
    assert call(route, v2, d2, None, P_(), 0, 1, 0)[0] == capi.E_ARG


def test_roles_above_the_first_role_words(route):
    """254 libraries with the role pattern of lib_pattern(3) (ignore / case / control, no copy of itself 16 .. 128 libraries further):
    a role table indexed modulo 16, 32, 64 or 128 libraries selects other positions — asserted on the reference's side"""
    v, d, dense, keep = lib254_views(route)
    role = lib_pattern(3)
    assert sorted(set(role)) == [0, 1, 2]
    for p in (P_(BOTH, min_depth=3, min_alt=2, ctl_max_alt=1), P_(SNV, min_depth=2, min_alt=3, ctl_max_alt=2, ctl_frac=(1, 3))):
        idx, why = check(route, v, d, dense, role, p, what="role pattern", proper=True)
        for period in (16, 32, 64, 128):
            other = dense.want(folded(role, period), p)
            assert not (np.array_equal(other[0], idx) and np.array_equal(other[1], why)), period


def SAME_BUCKET(m):
    """(slot 0's reads, slot 1's reads) of the one bucket both slots name"""
    return [(0, 0), (m, 0), (0, m), (m, m - 1), (m - 1, m)]


def test_two_slots_naming_one_bucket(route):
    """slotid with b0 == b1 (only hand-made views have it): expand_lane's rule is that the later write wins and that an integer is written
    only where it is not zero, so the bucket's count is slot 1's unless that is zero.  Counts exactly at min_alt and one below, in
    either order; the bucket is once the reference's own (nothing may be selected) and once an alternate; windows from k0 = 0 .. 4 put
    every combination on lanes 63 and 64."""
    m, Pn = 3, 135
    combos = SAME_BUCKET(m)
    for what, b in (("the reference's bucket", 1), ("an alternate", 3)):
        si = np.zeros((1, 2, 9, Pn), np.uint32)
        for k in range(Pn):
            si[0, 0, 0, k], si[0, 1, 0, k] = combos[k % 5]
        v, d, istat, _, refbase, keep = raw_views(route, np.full((1, Pn), 20), np.full((1, Pn), b | (b << 8)), si, ref=b"A" * Pn)
        dense = Dense(np.full((1, Pn), 20, np.uint32), istat[:, 1:5, 0, :], refbase, [], 0)
        assert dense.cnt[0, b - 1, :5].tolist() == [0, m, m, m - 1, m]
        for k0 in range(5):
            idx, why = check(route, v, d, dense, None, P_(SNV, min_alt=m), k0, Pn - k0, what="%s, k0 %d" % (what, k0), caps=[1])
            if b == 1:
                assert len(idx) == 0
            else:
                assert sorted(set((idx % 5).tolist())) == [1, 2, 4] and (why == capi.WHY_G).all() and {63 + k0, 64 + k0} & set(idx.tolist())


def test_records_of_libraries_that_do_not_exist(route):
    """third-allele records and indel records whose library is n_lib, n_lib + 1 or -1, each beside a valid record of the same position
    (lanes 10, 63 and 64): the list is what the valid records alone give, and nothing outside the contract is written"""
    L, Pn = 2, 130
    import handmade_views as hv
    si = np.zeros((L, 2, 9, Pn), np.uint32); si[:, 0, 0] = 20; si[:, 1, 0, ::7] = 1
    slotid = high_slot_bytes(np.full((L, Pn), 1 | (3 << 8), np.uint32))     # slot 1: G, one read every seventh position; 0x83 from 110 on
    si[:, 1, 0, 112] = 9; si[:, 0, 0, 105] = 9; slotid[:, 105] = 0x83 | 0xFF00             # nine reads in a slot whose byte is 0x83: nobody's
    recs, ind, good = [], [], []
    for t, k in enumerate((10, 63, 64)):
        for bad in (L, L + 1, -1):
            recs.append(hv.record(k, bad, 3, [9] * 9, [0] * 4)); recs.append(hv.record(k, bad, 4, [9] * 9, [0] * 4))
            ind += [(k, bad, 2, 9), (k, bad, -2, 9)]
        recs.append(hv.record(k, t % L, 3, [4] * 9, [0] * 4))
        ind.append((k, t % L, -1, 4)); good.append((k, t % L, -1, 4))
    recs = recs[::-1]
    v, d, istat, _, refbase, keep = raw_views(route, np.full((L, Pn), 25), slotid, si, records=recs, indels=ind, ref=b"A" * Pn)
    dense = Dense(np.full((L, Pn), 25, np.uint32), istat[:, 1:5, 0, :], refbase, good, 0)
    for role in (None, [1, 2], [2, 1]):
        idx, why = check(route, v, d, dense, role, P_(BOTH, min_alt=3, ctl_max_alt=0), what="bad libraries, roles %r" % (role,), proper=True, caps=[1])
        if role is None:
            assert idx.tolist() == [10, 63, 64] and (why == (capi.WHY_G | capi.WHY_DEL)).all()
    check(route, v, d, dense, None, P_(BOTH, min_alt=3), 63, 2, what="bad libraries, lanes 63 and 64 alone")


def test_records_one_position_behind_the_window(route, monkeypatch):
    """a third-allele record and an indel record at k0 + n, inside the planes: neither belongs to the window.  Linked or flagged all the
    same, they would write the word behind head[] / flag[] — next[0], resp. head[0] — and the records of the window's first position
    would come out otherwise: record 0 is the window's first position's, record 1 another position's with more reads of another base.
    On the CPU build the record loop runs in both orders (BRC_SIM_LANES, read by tests/sim_select alone): the word is read back only
    when it is written last.  The product library does not read the variable: on [hip] the second pass is a plain repeat."""
    import handmade_views as hv
    Pn, n = 130, 100
    si = np.zeros((1, 2, 9, Pn), np.uint32); si[0, 0, 0] = 20
    recs = [hv.record(0, 0, 3, [5] * 9, [0] * 4), hv.record(50, 0, 4, [7] * 9, [0] * 4), hv.record(n, 0, 2, [9] * 9, [0] * 4)]
    ind = [(n, 0, 2, 5), (20, 0, 3, 4)]
    v, d, istat, _, refbase, keep = raw_views(route, np.full((1, Pn), 30), np.full((1, Pn), 1 | (0xFF << 8)), si, records=recs, indels=ind, ref=b"A" * Pn)
    dense = Dense(np.full((1, Pn), 30, np.uint32), istat[:, 1:5, 0, :], refbase, ind, 0)
    for order in ("backward", "forward"):
        monkeypatch.setenv("BRC_SIM_LANES", order)
        idx, why = check(route, v, d, dense, None, P_(BOTH, min_alt=3), 0, n, what="records at k0 + n, %s" % order, caps=[1])
        assert idx.tolist() == [0, 20, 50] and why.tolist() == [capi.WHY_G, capi.WHY_INS, capi.WHY_T]
    idx, why = check(route, v, d, dense, None, P_(BOTH, min_alt=3), 0, n + 1, what="... and inside the window")
    assert idx.tolist() == [0, 20, 50, n] and why[-1] == capi.WHY_C | capi.WHY_INS


# ------------------------------------------------------------------------------------------------ 5. indel rules

INDEL_P = P_(INDEL, min_depth=5, min_alt=2, ctl_min_depth=2, ctl_max_alt=0)
INDEL_CALLS = [("indel rules", [1, 2, 2], INDEL_P), ("ctl_max_alt 1", [1, 2, 2], dict(INDEL_P, ctl_max_alt=1, ctl_min_depth=0)),
               ("no control", [1, 0, 0], dict(INDEL_P, min_alt=1)), ("both kinds", [1, 2, 2], dict(INDEL_P, flags=BOTH))]


def indel_views(route, records=True):
    """three libraries of depth 10 on the reference base, the third shallow from position 150 on, and the indel records of the rules
    (records=False: none, n_slots == 0)"""
    P = 200
    depth = np.full((3, P), 10, np.uint32); depth[2, 150:] = 1                          # library 2 (a control) is shallow from 150 on
    cnt = np.zeros((3, 4, P), np.uint32); cnt[:, 0] = 10; cnt[2, 0, 150:] = 1
    ref = b"A" * P
    ind = [(10, 0, 3, 4), (10, 0, -2, 4),                  # insertion and deletion at one position
           (20, 0, 3, 4), (20, 1, 3, 2),                   # case and control of the same sign: vetoed at ctl_max_alt < 2
           (30, 0, 3, 4), (30, 1, -3, 2),                  # ... of opposite sign: no veto
           (40, 0, 2, 4), (40, 1, 5, 1),                   # a control insertion of another length (another spelling) still vetoes
           (50, 1, 3, 4),                                  # a control record alone: nothing
           (60, 0, -1, 1),                                 # a case record below min_alt
           (160, 0, 3, 4),                                 # a control library below ctl_min_depth
           (70, 0, 3, 4), (70, 2, 3, 1), (70, 1, 3, 0)]    # two controls, one vetoes
    return build_views(route, depth, cnt, ref, indels=ind if records else ())


def test_indel_rules(route):
    v, d, dense, keep = indel_views(route)
    got = {}
    for what, role, p in INDEL_CALLS:
        idx, why = check(route, v, d, dense, role, p, what=what, proper=True)
        got[what] = dict(zip(idx.tolist(), why.tolist()))
    assert got["indel rules"] == {10: 48, 30: 16}
    assert got["ctl_max_alt 1"] == {10: 48, 30: 16, 40: 16, 70: 16, 160: 16}
    assert sorted(got["no control"]) == [10, 20, 30, 40, 60, 70, 160]
    # a view without records
    v, d, dense, keep = indel_views(route, records=False)
    assert d.n_slots == 0 and not d.slots
    rc, total, _, _ = call(route, v, d, [1, 2, 2], INDEL_P, 0, dense.n_pos, 4)
    assert (rc, total) == (0, 0)


# ------------------------------------------------------------------------------------------------ 6. capacity

def test_capacity_and_determinism(route, low_region):
    ref, arrs, res = low_region
    eng = td.computed(route.engine_lib, arrs, 50, 2950, ref, **PER_LIB)
    v, d = views_of(eng)
    dense = Dense.of(res)
    P = res.n_pos
    widx, wwhy = check(route, v, d, dense, [1, 2], EDGE_P, what="capacity", proper=True, caps=[0, 1, 63, 64, 65])
    m = len(widx)
    check(route, v, d, dense, [1, 2], EDGE_P, what="total - 1", caps=[m - 1, m + 5])
    a = call(route, v, d, [1, 2], EDGE_P, 0, P, m)
    b = call(route, v, d, [1, 2], EDGE_P, 0, P, m)
    assert a[0] == b[0] == 0 and a[1] == b[1] == m and a[2].tobytes() == b[2].tobytes() and a[3].tobytes() == b[3].tobytes()
    rc, total, gi, gw = call(route, v, d, [1, 2], EDGE_P, 0, P, m, want=("idx",))
    assert rc == 0 and total == SENT and np.array_equal(gi[:m].view(np.int32), widx) and (gi[m:] == SENT).all() and (gw == SENT).all()
    rc, total, gi, gw = call(route, v, d, [1, 2], EDGE_P, 0, P, m, want=("why",))
    assert rc == 0 and total == SENT and np.array_equal(gw[:m], wwhy.astype(np.uint32)) and (gw[m:] == SENT).all() and (gi == SENT).all()
    assert call(route, v, d, [1, 2], EDGE_P, 0, P, m, want=())[0] == 0
    t = route.select.last_timing()
    assert t["bytes_read"] == 0
    call(route, v, d, [1, 2], EDGE_P, 0, P, m)
    t = route.select.last_timing()
    assert t["kernel_s"] > 0 and t["bytes_read"] >= 4 * 4 * 2 * P
    assert route.select.workspace(v, d, 0) == 0 and route.select.workspace(None, None, 5) == 0
    eng.close()


# ------------------------------------------------------------------------------------------------ 7. refusals

def test_refused_calls_write_nothing(route, low_region):
    ref, arrs, res = low_region
    eng = td.computed(route.engine_lib, arrs, 50, 2950, ref, **PER_LIB)
    v, d = views_of(eng)
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
    ok = dict(v=v, d=d, role=[1, 2], p=P_(), k0=0, n=100, cap=8)
    cases = [("no handle", dict(handle=False)), ("no view", dict(v=None)), ("no indel view", dict(d=None)), ("no parameters", dict(params=False)),
             ("k0 < 0", dict(k0=-1)), ("n < 0", dict(n=-1)), ("k0 + n > n_pos", dict(k0=P - 5, n=6)), ("k0 beyond the planes", dict(k0=P + 1, n=0)),
             ("memory of the other kind", dict(v=av(memory=other), d=ad(memory=other))), ("memory 0", dict(v=av(memory=0), d=ad(memory=0))),
             ("views of two kinds", dict(d=ad(memory=other))), ("another device", dict(v=av(device=int(v.device) + 1), d=ad(device=int(v.device) + 1))),
             ("views of two devices", dict(v=av(device=int(v.device) + 1))), ("a view without planes", dict(v=av(si=None))),
             ("a view without planes (depth)", dict(v=av(depth=None))), ("not a view", dict(v=capi.DeviceView())),
             ("records without their arrays", dict(d=ad(slots=None))), ("records without the third-allele array", dict(v=av(xagg=None, n_xagg=5))),
             ("n_lib differs", dict(d=ad(n_lib=1))), ("pos0 differs", dict(d=ad(pos0=int(d.pos0) + 1))), ("n_pos differs", dict(d=ad(n_pos=P - 1))),
             ("flags 0", dict(p=P_(0))), ("unknown flags", dict(p=P_(4))), ("unknown flags beside known ones", dict(p=P_(BOTH | 8))),
             ("min_alt 0", dict(p=P_(min_alt=0))), ("frac_den 0", dict(p=P_(frac=(1, 0)))), ("ctl_frac_den 0", dict(p=P_(ctl_frac=(1, 0)))),
             ("a role above 2", dict(role=[1, 3])), ("no case library", dict(role=[2, 0])), ("no case library (all ignored)", dict(role=[0, 0])),
             ("cap < 0", dict(cap=-1)), ("no workspace", dict(ws=False)),
             ("a window that ends behind index 2^31 - 1", dict(v=av(n_pos=2 ** 31 + 64, stride=2 ** 31 + 64), d=ad(n_pos=2 ** 31 + 64), k0=2 ** 31 - 50, n=100))]
    for what, kw in cases:
        a = dict(ok, **kw)
        rc, total, gi, gw = call(route, a.pop("v"), a.pop("d"), a.pop("role"), a.pop("p"), a.pop("k0"), a.pop("n"), a.pop("cap"), **a)
        assert rc == capi.E_ARG, what
        assert total == SENT and (gi == SENT).all() and (gw == SENT).all(), "%s: something was written" % what
        if kw.get("handle", True):
            assert route.select.lib.brc_select_last_error(route.select.h), what
    # n == 0 is fine: the count is 0, nothing else is written
    rc, total, gi, gw = call(route, v, d, [1, 2], P_(), 7, 0, 8)
    assert (rc, total) == (0, 0) and (gi == SENT).all() and (gw == SENT).all()
    assert call(route, v, d, None, P_(), P, 0, 0, want=())[0] == 0
    assert route.select.lib.brc_select_last_error(route.select.h) == b""
    eng.close()


# ------------------------------------------------------------------------------------------------ 8. the host sanitizers

def _bytes_at(p, n):
    return C.string_at(p, n) if n else b""


def _serialize(v, d, calls):
    """the host views of a sim engine and the calls as select_check.cpp reads them"""
    b = td._serialize_view(v, [])
    b = b[:36] + struct.pack("<i", len(calls)) + b[40:]
    b += struct.pack("<Q", d.n_slots) + _bytes_at(d.slots, int(d.n_slots) * 72)
    nref = max(min(int(d.ref_hi), int(d.ref_len)) - int(d.ref_lo), 0) if d.ref else 0
    b += struct.pack("<iqqqq", 1 if d.ref else 0, d.ref_lo, d.ref_hi, d.ref_len, nref) + _bytes_at(d.ref, nref)
    for k0, n, cap, role, p, want in calls:
        b += struct.pack("<qqq9Iii", k0, n, cap, p["flags"], p["min_depth"], p["min_alt"], p["frac"][0], p["frac"][1], p["ctl_min_depth"],
                         p["ctl_max_alt"], p["ctl_frac"][0], p["ctl_frac"][1], 0 if role is None else 1, want)
        b += bytes(role or [])
    return b


def _sanitized(tmp_path, name, v, d, dense, calls):
    """select_check_asan over one pair of host views: every call must return 0 without a report and give the reference's count, list
    and reason words, with everything behind the list as it was filled; returns the number of list elements compared"""
    assert v.memory == capi.MEM_HOST and d.memory == capi.MEM_HOST
    case, out = str(tmp_path / (name + ".bin")), str(tmp_path / (name + ".res"))
    open(case, "wb").write(_serialize(v, d, calls))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    pr = subprocess.run([side.sim_checker(side.SIDE["select"]), case, out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert pr.returncode == 0, (name, pr.stderr.decode()[-3000:])
    assert pr.stdout.decode().strip() == "%d calls" % len(calls), name
    out = np.fromfile(out, np.uint32); o = 0
    some = 0
    for k0, n, cap, role, p, want in calls:
        widx, wwhy = dense.want(role, p, k0, n)
        m, t = len(widx), min(len(widx), cap)
        some += t
        assert out[o].view(np.int32) == 0, (name, k0, n, cap)
        assert out[o + 1] == (m if want & 4 else SENT), (name, k0, n, cap, out[o + 1], m)
        gi, gw = out[o + 2:o + 2 + cap], out[o + 2 + cap:o + 2 + 2 * cap]; o += 2 + 2 * cap
        ti, tw = (t if want & 1 else 0), (t if want & 2 else 0)
        assert np.array_equal(gi[:ti].view(np.int32), widx[:ti].astype(np.int32)) and (gi[ti:] == SENT).all(), (name, k0, n, cap, want)
        assert np.array_equal(gw[:tw], wwhy[:tw].astype(np.uint32)) and (gw[tw:] == SENT).all(), (name, k0, n, cap, want)
    assert o == out.size, name
    return some


def _calls_of(dense, role, p, k0=0, n=None, every=True):
    """the forms of one call as (k0, n, cap, role, p, want): the list at cap = total; with `every` also total - 1, the count alone,
    idx alone, why alone, and a capacity beyond the total without the count"""
    n = dense.n_pos - k0 if n is None else n
    m = len(dense.want(role, p, k0, n)[0])
    c = [(k0, n, m, role, p, 7)]
    if every:
        c += [(k0, n, max(m - 1, 0), role, p, 7), (k0, n, 0, role, p, 4), (k0, n, m, role, p, 1), (k0, n, m, role, p, 2), (k0, n, m + 2, role, p, 3)]
    return c


def test_calls_under_the_host_sanitizers(oracle_lib, sim_route, low_region, tmp_path, monkeypatch):
    """The views, windows, parameter sets and capacities of the tests above on the CPU build with -fsanitize=address,undefined: sources
    of exactly the views' sizes (the reference slice cut at ref_len, the role array of exactly n_lib bytes), a scratch of exactly
    brc_select_workspace bytes, idx and why of exactly cap elements — a load or store outside them is a report — and the results are
    the reference's.  Engine-made: the third-allele region (records of both kinds) and the low-depth two-library region.  Hand-made
    (build_views on the CPU route, serialised as they are): the selected-count layouts (no third-allele record: a scratch without
    head and next), the exact thresholds, the counts next to 2^32, the reference characters, no reference, the slices that start
    late, end early or pass ref_len, the 254 libraries, the indel rules and the view without indel records.  The 70 000-position
    region of the scan carry stays with the plain routes: the carry is a loop of the device's k_select_parts alone, which the CPU
    build does not have."""
    route = sim_route
    some = 0
    # 2 + the windows of 3 + 6: the third-allele region
    monkeypatch.setenv("BRC_FORCE_DOM", "3"); monkeypatch.setenv("BRC_XEV_CAP", "1")
    ref, arrs = td.third_allele_inputs()
    res, _ = td.oracle_result(oracle_lib, arrs, 100, 1900, ref, **PER_LIB)
    eng = td.computed(route.knob_lib, arrs, 100, 1900, ref, **PER_LIB)
    monkeypatch.delenv("BRC_FORCE_DOM"); monkeypatch.delenv("BRC_XEV_CAP")
    v, d = views_of(eng)
    assert v.n_xagg > 0 and d.n_slots > 0
    dense = Dense.of(res)
    sets = [p for _, p in FIXTURE_PARAMS + TWOLIB_PARAMS] + [EDGE_P, P_(SNV, min_depth=4, min_alt=1, ctl_max_alt=0)]
    calls = []
    for i, (k0, n) in enumerate(window_list(res.n_pos)):
        for j, p in enumerate(sets):
            calls += _calls_of(dense, ([1, 2], [2, 1], None)[(i + j) % 3], p, k0, n, every=j == i % len(sets))
    calls.append((17, 0, 5, None, EDGE_P, 7))
    some += _sanitized(tmp_path, "third", v, d, dense, calls)
    eng.close()
    assert some > 1000
    # 1, 3, 6: the two synthetic libraries
    ref, arrs, res = low_region
    eng = td.computed(route.engine_lib, arrs, 50, 2950, ref, **PER_LIB)
    v, d = views_of(eng)
    dense = Dense.of(res)
    calls = []
    for role in ([1, 2], [2, 1]):
        for _, p in TWOLIB_PARAMS:
            calls += _calls_of(dense, role, p, every=False)
    for i, (k0, n) in enumerate(window_list(res.n_pos)):
        calls += _calls_of(dense, ([1, 2], None)[i % 2], EDGE_P, k0, n)
    some += _sanitized(tmp_path, "low", v, d, dense, calls)
    eng.close()
    # 3: numbers of selected positions, on views without a third-allele record
    bare = 0
    for name, ks, (v, d, dense, keep) in wave_views(route):
        bare += v.n_xagg == 0
        calls = _calls_of(dense, None, WAVE_P) + [(0, dense.n_pos, c, None, WAVE_P, 7) for c in (1, 64)]
        if name == "257":
            calls += _calls_of(dense, None, WAVE_P, 299, 259)
        assert _sanitized(tmp_path, "wave", v, d, dense, calls) >= len(ks)
    assert bare
    # 4: arithmetic, reference characters and slices, 254 libraries
    v, d, dense, keep = threshold_views(route)
    _sanitized(tmp_path, "thresholds", v, d, dense, [c for p in THRESHOLD_SETS for c in _calls_of(dense, [1, 2], p)])
    v, d, dense, keep = big_views(route)
    _sanitized(tmp_path, "big", v, d, dense, [c for p in BIG_SETS for c in _calls_of(dense, [1, 2], p)])
    kinds = set()
    for what, (v, d, dense, keep), p in refchar_views(route):
        kinds.add((bool(d.ref), d.ref_lo > d.pos0, d.ref_hi < d.pos0 + d.n_pos, d.ref_len < d.ref_hi))
        _sanitized(tmp_path, "ref", v, d, dense, _calls_of(dense, None, p) + _calls_of(dense, None, p, 3, dense.n_pos - 5, every=False))
    assert len(kinds) >= 5                          # whole, none, late, early, cut by ref_len
    v, d, dense, keep = lib254_views(route)
    assert v.n_xagg > 0
    _sanitized(tmp_path, "lib254", v, d, dense, [c for role, p in LIB254_CALLS for c in _calls_of(dense, role, p)])
    # 5: the indel rules, and a view without indel records
    v, d, dense, keep = indel_views(route)
    _sanitized(tmp_path, "indels", v, d, dense, [c for _, role, p in INDEL_CALLS for c in _calls_of(dense, role, p)])
    v, d, dense, keep = indel_views(route, records=False)
    assert d.n_slots == 0
    _sanitized(tmp_path, "noslots", v, d, dense, [c for _, role, p in INDEL_CALLS for c in _calls_of(dense, role, p)])


# ------------------------------------------------------------------------------------------------ 9. tensors.select

def check_select(route, r, dense, role, p, what, k0=0, n=None):
    widx, wwhy = dense.want(role, p, k0, n)
    assert 0 < len(widx), what
    assert r["n"] == len(widx) and r["pos0"] == dense.pos0 and r["first"] == dense.pos0 + k0, what
    for k, w in (("idx", widx), ("pos", widx + dense.pos0), ("why", wwhy)):
        a = route.host(r[k])
        assert a.dtype == np.int32 and np.array_equal(a, w.astype(np.int32)), (what, k)
        assert isinstance(r[k], np.ndarray) if route.name == "sim" else r[k].is_cuda, (what, k)


def test_tensors_select_on_text_only_engines_and_after_a_fetch(route, oracle_lib, test_bam):
    from bam_readcount_amd import tensors
    beg0, end = 10403000, 10403700
    res, text = td.oracle_result(oracle_lib, test_bam, beg0, end, test_bam["ref"], tid=20, chrom="21")
    dense = Dense.of(res)
    p = FIXTURE_PARAMS[2][1]
    kw = dict(min_depth=p["min_depth"], min_alt=p["min_alt"], min_frac=p["frac"], ctl_min_depth=p["ctl_min_depth"], ctl_max_alt=p["ctl_max_alt"],
              ctl_max_frac=p["ctl_frac"])
    for opts in (dict(text_only=True), dict(device_text="21")):
        eng = td.computed(route.engine_lib, test_bam, beg0, end, test_bam["ref"], tid=20, **opts)
        check_select(route, tensors.select(eng, route.select, **kw), dense, None, p, "before fetch %r" % opts)
        eng.fetch_result()
        assert eng.format_region("21") == text
        check_select(route, tensors.select(eng, route.select, **kw), dense, None, p, "after fetch %r" % opts)
        # a window in reference coordinates, clipped to the planes; one kind alone
        w = tensors.select(eng, route.select, beg0=res.pos0 + 70, end=10 ** 9, indel=False, **kw)
        check_select(route, w, dense, None, dict(p, flags=SNV), "window", 70, res.n_pos - 70)
        e = tensors.select(eng, route.select, beg0=res.pos0 + res.n_pos + 5, **kw)
        assert e["n"] == 0 and tuple(e["idx"].shape) == (0,) and tuple(e["pos"].shape) == (0,)
        eng.close()


def test_tensors_select_names_errors_and_the_chain_to_sites(route, oracle_lib, twolib, low_region):
    """case= / control= names, refusals, and the chain select -> sites: on twolib.npz (whose list is empty, see
    test_golden_fixtures_whole) and on the synthetic two-library region, where the panel must hold the oracle's planes at the
    oracle-selected positions bit for bit"""
    from bam_readcount_amd import tensors
    import test_panel as tp
    panel = route.another("panel")
    p = TWOLIB_PARAMS[2][1]
    kw = dict(min_depth=p["min_depth"], min_alt=p["min_alt"], min_frac=p["frac"], ctl_max_frac=p["ctl_frac"])

    def chain(eng, res, sel, widx):
        r = tensors.sites(eng, panel, positions=sel["pos"], want=tensors.KINDS)
        want = tp.want_at(res, widx)
        assert r["n"] == len(widx)
        for k in tp.KINDS:
            assert np.array_equal(tp.host_words(route, r[k]).reshape(want[k].shape), want[k]), k
        assert int(tp.host_words(route, r["status"])[0]) == 0
    tnames = [str(s) for s in twolib["lib_names"]]
    opts = dict(lib_names=tnames, per_lib=True, insertion_centric=True, ref_len_check=True)
    end = int(twolib["ref"].size)
    res, _ = td.oracle_result(oracle_lib, twolib, 0, end, twolib["ref"], **opts)
    eng = td.computed(route.engine_lib, twolib, 0, end, twolib["ref"], **opts)
    sel = tensors.select(eng, route.select, case=[tnames[0]], control=[tnames[1]], **kw)
    widx, _ = Dense.of(res).want([1, 2], p)
    assert sel["n"] == len(widx) == 0
    chain(eng, res, sel, widx)
    eng.close()
    ref, arrs, res = low_region
    names = PER_LIB["lib_names"]
    dense = Dense.of(res)
    eng = td.computed(route.engine_lib, arrs, 50, 2950, ref, **PER_LIB)
    check_select(route, tensors.select(eng, route.select, case=[names[0]], control=[names[1]], **kw), dense, [1, 2], p, "case / control")
    check_select(route, tensors.select(eng, route.select, case=names[1], control=names[0].encode(), **kw), dense, [2, 1], p, "control / case")
    check_select(route, tensors.select(eng, route.select, case=[names[1]], **kw), dense, [0, 1], p, "case alone")
    check_select(route, tensors.select(eng, route.select, role=[1, 2], **kw), dense, [1, 2], p, "role")
    sel = tensors.select(eng, route.select, **kw)
    check_select(route, sel, dense, None, p, "every library a case")
    chain(eng, res, sel, dense.want(None, p)[0])
    sel = tensors.select(eng, route.select, case=[names[0]], control=[names[1]], **kw)
    chain(eng, res, sel, dense.want([1, 2], p)[0])
    # refused before anything is queued
    bad = [dict(kw, min_alt=0), dict(kw, min_frac=(1, 0)), dict(kw, ctl_max_frac=(1, 0)), dict(kw, snv=False, indel=False), dict(kw, role=[1, 3]),
           dict(kw, role=[2, 2]), dict(kw, role=[1]), dict(kw, case=["nobody"]), dict(kw, control=[names[0]]), dict(kw, role=[1, 2], case=[names[0]]),
           dict(kw, case=[names[0], names[0]]), dict(kw, min_depth=-1), dict(kw, ctl_max_alt=2 ** 32), dict(kw, min_frac=(1, 2, 3)), dict(kw, min_alt=1.5)]
    for b in bad:
        with pytest.raises(ValueError):
            tensors.select(eng, route.select, **b)
    with pytest.raises(TypeError):
        tensors.select(eng, route.select, min_depth=1)            # (min_alt has no default)
    eng.close()
    # names need an engine that keeps libraries apart
    eng = td.computed(route.engine_lib, arrs, 50, 2950, ref)
    with pytest.raises(ValueError, match="^case / control name libraries: the engine reports one set of counts for all of them$"):
        tensors.select(eng, route.select, case=[names[0]], **kw)
    eng.close()
