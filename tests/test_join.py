"""Device-side join of computed regions (include/brc_join.h): brc_join_views and bam_readcount_amd.tensors.join against a PLAIN-PYTHON
restatement of the header's definition (`reference`: loops over libraries, records and bytes; nothing of the library's core is read),
every output equal as bit patterns, no tolerance, no cell left out; and against a reference that does not come from the code under
test at all: ONE per-library engine over all reads equals the join of all-library engines over one library's reads each, through every
consumer of a view.

Every body runs twice (the `route` fixture): [sim] = tests/sim_join/libbrc_join_sim.so, host memory, in the CPU suite; [hip] = the
product's library on the GPU (gpu-marked), views, scratch and destinations in device memory allocated through torch.  Destinations are
filled with 0xA5 first and are PAD words wider than the contract's sizes: the pad elements [n_pos, stride) of every row, everything
behind a buffer's size and every buffer that was not asked for must keep it.  The scratch has exactly brc_join_workspace bytes.

Sizes that matter to the kernels (brc_join.hip): a lane stores four elements at a 16-byte boundary of its row, a wave 256, a workgroup
1024; a row whose base is not 16-byte aligned has one to three single elements in front."""
import ctypes as C
import struct

import numpy as np
import pytest

from bam_readcount_amd import capi
import handmade_views as hv
from route import Route, SENT, SENT8
import test_dense as td
import test_indels as ti
import test_inorm as tn
import test_ivet as tiv
import test_select as ts
import test_vet as tv

NONE32, PAD = hv.NONE32, hv.PAD
NI, NF = 9, 4
EMPTY_SLOT = 1 | (7 << 8)             # lane2_store (brc_core.h) for a position no read covers: bucket 1, NB_NONE
PLANES = (("ncol", 1), ("depth", 1), ("slotid", 1), ("si", 18), ("sf", 8))
VIEW_BUFS = ("ncol", "depth", "slotid", "si", "sf", "xagg")
INDEL_BUFS = ("slots", "seq_off", "l_qseq", "seq4", "ref")
CASE, CTL = capi.ROLE_CASE, capi.ROLE_CONTROL
LIBS = tn.LIBS + ("join", "panel", "bins", "runs")          # (every row of the table)


@pytest.fixture(scope="module", params=["sim", pytest.param("hip", marks=pytest.mark.gpu)])
def route(request):
    return Route(request.param, LIBS, engine=True)


@pytest.fixture(scope="module")
def sim_route():
    return Route("sim", LIBS, engine=True)


# ------------------------------------------------------------------------------------------------ sources and the reference

def rand_arrays(L, P, seed):
    """compact planes of random words: every bit pattern, NaNs among the float sums"""
    rng = np.random.default_rng(seed)

    def r(*shape):
        return rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)
    return {"ncol": r(L, P), "depth": r(L, P), "slotid": r(L, P), "si": r(L, 2, NI, P), "sf": r(L, 2, NF, P), "unavail": None}


class Src:
    """One hand-made source: planes A at pos0, third-allele records, the stride; I: hv.indel_arrays' dict (None: an indels view without
    records or reference; False: no indels view at all)."""

    def __init__(self, A, pos0, records=(), stride=None, I=None):
        self.A, self.pos0, self.records, self.stride = A, pos0, [list(r) for r in records], stride
        self.L, self.P = A["ncol"].shape
        self.I = hv.indel_arrays([], pos0=pos0, n_pos=self.P, n_lib=self.L) if I is None else I
        if self.I:
            assert (self.I["pos0"], self.I["n_pos"], self.I["n_lib"]) == (pos0, self.P, self.L)

    def place(self, route):
        v, keep = hv.make_view(route, self.A, self.records, self.stride, self.pos0)
        v.memory = route.mem
        d = None
        if self.I:
            d, k2 = hv.make_indels(route, self.I)
            d.memory = route.mem
            keep = (keep, k2)
        return v, d, keep


def reference(srcs, pos0, n):
    """include/brc_join.h, operation by operation"""
    L = sum(s.L for s in srcs)
    W = {"L": L}
    for name, per in PLANES:
        out = np.full((L * per, n), EMPTY_SLOT if name == "slotid" else 0, np.uint32)
        base = 0
        for s in srcs:
            a = np.asarray(s.A[name], np.uint32).reshape(s.L * per, s.P)
            lo, hi = max(pos0, s.pos0), min(pos0 + n, s.pos0 + s.P)
            if hi > lo:
                out[base * per:(base + s.L) * per, lo - pos0:hi - pos0] = a[:, lo - s.pos0:hi - s.pos0]
            base += s.L
        W[name] = out
    xagg, slots, lq, reads, base = [], [], [], [], 0
    for s in srcs:
        for rec in s.records:
            rec = list(rec)
            k, lib = rec[0], rec[1] >> 8
            kj = k + s.pos0 - pos0
            if k != NONE32 and k < s.P and lib < s.L and 0 <= kj < n:
                rec[0], rec[1] = kj, ((lib + base) << 8) | (rec[1] & 0xFF)
            else:
                rec[0] = NONE32
            xagg.append(rec)
        for rec in (s.I["slots"].tolist() if s.I else ()):
            p, lib, ln = hv.i32(rec[0]), hv.i32(rec[1]), hv.i32(rec[2])
            kept = ln != 0 and pos0 <= p < pos0 + n and s.pos0 <= p < s.pos0 + s.P and 0 <= lib < s.L
            r = len(slots)
            codes = []
            if kept and ln > 0:
                rr, rq = rec[3], hv.i32(rec[4])
                for j in range(ln):
                    q = rq + 1 + j
                    if rr < s.I["n_reads"] and 0 <= q < int(s.I["l_qseq"][rr]):
                        byte = int(s.I["seq4"][int(s.I["seq_off"][rr]) + q // 2])
                        codes.append(byte >> 4 if q % 2 == 0 else byte & 15)
                    else:
                        codes.append(15)
            slots.append([rec[0], (lib + base) & hv.U32 if kept else rec[1], rec[2] if kept else 0, r, hv.U32] + rec[5:])
            lq.append(len(codes)); reads.append(codes)
        base += s.L
    W["xagg"] = np.array(xagg, np.uint32).reshape(len(xagg), 16)
    W["slots"] = np.array(slots, np.uint32).reshape(len(slots), 18)
    W["l_qseq"] = np.array(lq, np.int32)
    seq, off = bytearray(), []
    for codes in reads:
        off.append(len(seq))
        codes = codes + [0] * (len(codes) & 1)
        seq += bytes((codes[j] << 4) | codes[j + 1] for j in range(0, len(codes), 2))
    W["seq_off"] = np.array(off, np.uint64); W["seq4"] = np.frombuffer(bytes(seq), np.uint8)
    W["counts"] = [sum(1 for r in slots if r[2] != 0), len(seq)]
    with_ref = [s.I for s in srcs if s.I and s.I["ref"] is not None]
    W["status"] = 0
    if with_ref:
        lo, hi, rl = min(i["ref_lo"] for i in with_ref), max(i["ref_hi"] for i in with_ref), with_ref[0]["ref_len"]
        out = bytearray(hi - lo)
        for p in range(lo, hi):
            for i in with_ref:
                if i["ref_lo"] <= p < i["ref_hi"] and 0 <= p < rl and i["ref"][p - i["ref_lo"]]:
                    c = i["ref"][p - i["ref_lo"]]
                    if not out[p - lo]:
                        out[p - lo] = c
                    elif out[p - lo] != c:
                        W["status"] = capi.JOIN_REF_DIFFERS
        W["ref"], W["ref_lo"], W["ref_hi"], W["ref_len"] = np.frombuffer(bytes(out), np.uint8), lo, hi, rl
    else:
        W["ref"], W["ref_lo"], W["ref_hi"], W["ref_len"] = np.zeros(0, np.uint8), 0, 0, 0
    W["has_ref"] = bool(with_ref)
    return W


def joined_indel_arrays(W, pos0, n):
    """the joined brc_device_indels in hv.indel_arrays' form, for hv.allele_text / hv.indel_table_reference"""
    return dict(slots=W["slots"], seq4=W["seq4"], seq_off=W["seq_off"], l_qseq=W["l_qseq"], n_reads=len(W["slots"]),
                ref=bytes(W["ref"]) if W["has_ref"] else None, ref_lo=W["ref_lo"], ref_hi=W["ref_hi"], ref_len=W["ref_len"], pos0=pos0, n_pos=n, n_lib=W["L"])


def buffer_words(rows, stride, n):
    return ((rows - 1) * stride + n) if n and rows else 0


class Joined:
    """one call's destinations back on the host, and the views it filled in"""


def run(route, srcs, pos0, n, stride=None, skew=False, seq_cap=None, halves=("view", "indels"), status=True, counts=True, placed=None, raw=False):
    """brc_join_views into sentinel-filled destinations of exactly the contract's sizes + PAD words.  seq_cap None: the exact one, read
    from a first call for the counts alone.  -> Joined (rc, the buffers' bytes, the views, the device buffers)"""
    stride = n if stride is None else stride
    placed = placed or [s.place(route) for s in srcs]
    src = capi.join_sources([(v, d) for v, d, _ in placed])
    rc, z = route.join.sizes_raw(src, pos0, n, stride)
    J = Joined()
    J.placed, J.src, J.z = placed, src, z
    if rc:
        z = capi.JoinSizes()
    wsb = int(z.workspace_bytes)
    assert wsb == route.join.workspace(int(z.n_slots))
    ws = route.sentinel_bytes(wsb)
    if seq_cap is None:
        c0 = route.sentinel_bytes(8)
        if "indels" in halves and not rc:
            route.join.views(src, pos0, n, stride, counts=route.ptr(c0), workspace=route.ptr(ws), workspace_bytes=wsb)
            J.first_counts = route.host(c0)[:8].view(np.uint32).tolist()
            seq_cap = J.first_counts[1]
        else:
            seq_cap = 0
    sizes = {k: int(getattr(z, k + "_bytes")) for k in capi.JOIN_DESTS if k != "seq4"}
    sizes["seq4"] = seq_cap
    bufs, off = {}, {}
    for k in capi.JOIN_DESTS:
        bufs[k] = route.sentinel_bytes(sizes[k] + 4 * PAD + (32 if skew else 0))
        off[k] = ((-route.ptr(bufs[k])) % 16 + 4) if skew and k in VIEW_BUFS[:5] else 0
    cbuf, sbuf = route.sentinel_bytes(8), route.sentinel_bytes(4)
    wanted = (VIEW_BUFS if "view" in halves else ()) + (INDEL_BUFS if "indels" in halves else ())
    dest = capi.JoinDest(**{k: route.ptr(bufs[k]) + off[k] for k in wanted})
    J.view, J.indels = capi.DeviceView(), capi.DeviceIndels()
    J.view.n_lib = J.indels.n_lib = -77                                   # (a refused call leaves the host structs alone)
    J.rc = route.join.views_raw(src, pos0, n, stride, dest=dest, out_view=J.view if "view" in halves else None, out_indels=J.indels if "indels" in halves else None,
                                counts=route.ptr(cbuf) if counts else None, seq_cap=seq_cap, status=route.ptr(sbuf) if status else None,
                                workspace=route.ptr(ws), workspace_bytes=wsb)
    J.err = route.join._call("_last_error")(route.join.h).decode()
    J.bufs, J.off, J.sizes, J.dest, J.keep = bufs, off, sizes, dest, (ws, cbuf, sbuf)
    J.got = {k: np.array(route.host(bufs[k])[off[k]:off[k] + sizes[k] + 4 * PAD]) for k in capi.JOIN_DESTS}
    J.counts = np.array(route.host(cbuf)[:8]).view(np.uint32).tolist()
    J.status = int(np.array(route.host(sbuf)[:4]).view(np.uint32)[0])
    J.ws = np.array(route.host(ws))
    return J


def untouched(J, keys=capi.JOIN_DESTS):
    return all((J.got[k] == SENT8).all() for k in keys)


def check(route, srcs, pos0, n, what="", stride=None, **kw):
    """one join against the reference, every byte; -> (Joined, the reference)"""
    stride = n if stride is None else stride
    W = reference(srcs, pos0, n)
    J = run(route, srcs, pos0, n, stride, **kw)
    assert J.rc == 0, (what, J.err)
    z = J.z
    halves = kw.get("halves", ("view", "indels"))
    L = W["L"]
    assert (z.n_lib, z.n_xagg, z.n_slots, bool(z.has_ref), z.ref_lo, z.ref_hi, z.ref_len) == \
        (L, len(W["xagg"]), len(W["slots"]), W["has_ref"], W["ref_lo"], W["ref_hi"], W["ref_len"]), what
    for name, per in PLANES:
        assert J.sizes[name] == 4 * buffer_words(L * per, stride, n), (what, name)
    assert (J.sizes["xagg"], J.sizes["slots"], J.sizes["seq_off"], J.sizes["l_qseq"], J.sizes["ref"]) == \
        (64 * len(W["xagg"]), 72 * len(W["slots"]), 8 * len(W["slots"]), 4 * len(W["slots"]), len(W["ref"])), what
    if "view" in halves:
        for name, per in PLANES:
            want = np.full((L * per, stride), SENT, np.uint32)
            want[:, :n] = W[name]
            want = np.concatenate([want.ravel()[:buffer_words(L * per, stride, n)], np.full(PAD, SENT, np.uint32)])
            g = J.got[name].view(np.uint32)
            assert np.array_equal(g, want), "%s: %s differs at words %r" % (what, name, np.flatnonzero(g != want)[:6].tolist())
        want = np.concatenate([W["xagg"].ravel(), np.full(PAD, SENT, np.uint32)])
        assert np.array_equal(J.got["xagg"].view(np.uint32), want), "%s: xagg differs at %r" % (what, np.flatnonzero(J.got["xagg"].view(np.uint32) != want)[:6].tolist())
        v = J.view
        assert (v.memory, v.device, v.n_lib, v.pos0, v.n_pos, v.stride, v.n_xagg, v.unavail) == (route.mem, 0, L, pos0, n, stride, len(W["xagg"]), None), what
        assert [v.ncol, v.depth, v.slotid, v.si, v.sf] == [route.ptr(J.bufs[k]) + J.off[k] for k in VIEW_BUFS[:5]]
        assert v.xagg == (route.ptr(J.bufs["xagg"]) if len(W["xagg"]) else None)
    else:
        assert untouched(J, VIEW_BUFS) and J.view.n_lib == -77, what
    if "indels" in halves:
        fits = W["counts"][1] <= J.sizes["seq4"]
        for k, w in (("slots", W["slots"]), ("seq_off", W["seq_off"]), ("l_qseq", W["l_qseq"]), ("ref", W["ref"])):
            want = np.concatenate([np.ascontiguousarray(w).ravel().view(np.uint8), np.full(4 * PAD, SENT8, np.uint8)])
            assert np.array_equal(J.got[k], want), "%s: %s differs at bytes %r" % (what, k, np.flatnonzero(J.got[k] != want)[:6].tolist())
        want = np.concatenate([W["seq4"], np.full(4 * PAD, SENT8, np.uint8)]) if fits else np.full(J.sizes["seq4"] + 4 * PAD, SENT8, np.uint8)
        assert np.array_equal(J.got["seq4"], want), (what, "seq4")
        if kw.get("counts", True):
            assert J.counts == W["counts"], what
        d = J.indels
        S = len(W["slots"])
        assert (d.memory, d.device, d.n_lib, d.pos0, d.n_pos, d.n_slots, d.n_reads) == (route.mem, 0, L, pos0, n, S, S), what
        assert (d.ref_lo, d.ref_hi, d.ref_len) == (W["ref_lo"], W["ref_hi"], W["ref_len"]) and (d.ref is not None) == (len(W["ref"]) > 0)
        assert [d.slots, d.seq_off, d.l_qseq] == ([route.ptr(J.bufs[k]) for k in ("slots", "seq_off", "l_qseq")] if S else [None] * 3)
        if kw.get("status", True):
            assert J.status == W["status"], what
    else:
        assert untouched(J, INDEL_BUFS) and J.indels.n_lib == -77, what
    if hasattr(J, "first_counts"):
        assert J.first_counts == W["counts"], what
    return J, W


def spelled(route, view, I, first, n):
    """brc_indels_gather over an indels view in the route's memory: (pos, lib, len, text) per record, in the table's order"""
    wsb = route.indels.workspace(view, n)
    ws, cnt = route.sentinel_bytes(wsb), route.sentinel_bytes(8)
    route.indels.gather(view, first - int(view.pos0), n, workspace=route.ptr(ws), workspace_bytes=wsb, counts=route.ptr(cnt))
    m, nb = route.host(cnt)[:8].view(np.uint32).tolist()
    b = {k: route.sentinel_bytes(4 * (m + 1)) for k in ("pos", "lib", "len", "allele_off")}
    b["alleles"] = route.sentinel_bytes(nb)
    route.indels.gather(view, first - int(view.pos0), n, workspace=route.ptr(ws), workspace_bytes=wsb, cap=m, alleles_cap=nb, **{k: route.ptr(x) for k, x in b.items()})
    h = {k: np.array(route.host(x)) for k, x in b.items()}
    off = h["allele_off"].view(np.uint32)[:m + 1].tolist()
    text = bytes(h["alleles"][:nb])
    return [(int(h["pos"].view(np.int32)[r]), int(h["lib"].view(np.int32)[r]), int(h["len"].view(np.int32)[r]), text[off[r]:off[r + 1]]) for r in range(m)]


# ------------------------------------------------------------------------------------------------ 3. hand-made views at every edge

OFFSETS = (-65, -64, -63, -1, 0, 1, 63, 64, 65, 257)
N_POS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025, 65537)


@pytest.mark.parametrize("off", OFFSETS)
def test_source_offsets(route, off):
    """pos0 - pos0_s of one source at every listed value, beside a second source at offset 0; the source's stride is wider than its planes"""
    n, pos0 = 300, 1000
    a = Src(rand_arrays(2, 290, 1), pos0 - off, stride=293)
    b = Src(rand_arrays(1, n, 2), pos0)
    check(route, [a, b], pos0, n, "offset %d" % off)
    check(route, [a, b], pos0, n, "offset %d, odd stride, skewed base" % off, stride=n + 5, skew=True, halves=("view",))


@pytest.mark.parametrize("n", N_POS)
def test_window_lengths(route, n):
    """the launch and vector-width edges, with the destination's stride equal to n_pos and odd, its base 16-byte aligned and 4 bytes behind"""
    pos0 = 500
    a = Src(rand_arrays(1, min(n + 7, 1500), 3), pos0 - 3)
    b = Src(rand_arrays(2, min(n, 900), 4), pos0 + (n > 10))
    check(route, [a, b], pos0, n, "n_pos %d" % n, halves=("view",))
    check(route, [a, b], pos0, n, "n_pos %d, stride n + 1 | 1, skewed" % n, stride=(n + 1) | 1, skew=True, halves=("view",))


def test_a_long_source_behind_an_odd_offset(route):
    """70 001 positions of which the source covers all but the ends: every group's loads are unaligned with its store"""
    pos0, n = 7, 70001
    check(route, [Src(rand_arrays(1, 69990, 5), pos0 + 5)], pos0, n, "long", halves=("view",), skew=True, stride=n + 2)


def test_sources_covering_the_first_element_the_last_or_none(route):
    pos0, n = 100, 130
    for what, p0, P in (("first only", pos0 - 9, 10), ("last only", pos0 + n - 1, 10), ("before", pos0 - 10, 10), ("behind", pos0 + n, 10), ("inside", pos0 + 50, 20),
                        ("empty source", pos0 + 5, 0)):
        J, W = check(route, [Src(rand_arrays(2, P, 6), p0)], pos0, n, what, halves=("view",))
        covered = (W["ncol"] != 0).any(axis=0).nonzero()[0].tolist()
        assert covered == {"first only": [0], "last only": [n - 1], "inside": list(range(50, 70))}.get(what, []), what


def test_one_engine_over_its_own_window_is_reproduced(route):
    A = rand_arrays(3, 257, 7)
    recs = [hv.record(k, l, b, *hv.body(t)) for t, (k, l, b) in enumerate([(0, 0, 4), (256, 2, 5), (17, 1, 0)])]
    J, W = check(route, [Src(A, 40, recs, stride=260)], 40, 257, "K = 1")
    for name, _ in PLANES:
        assert np.array_equal(W[name], np.asarray(A[name]).reshape(-1, 257))
    assert np.array_equal(W["xagg"], np.array(recs, np.uint32))


def test_sixteen_sources_and_the_library_totals(route):
    n, pos0 = 70, 10
    sixteen = [Src(rand_arrays(1 + s % 3, 40 + s, 10 + s), pos0 - 8 + 3 * s, [hv.record(5, s % 3, 4, *hv.body(s))]) for s in range(16)]
    J, W = check(route, sixteen, pos0, n, "K = 16")
    assert W["L"] == sum(1 + s % 3 for s in range(16)) and (W["xagg"][:, 0] != NONE32).sum() > 8
    for libs in ((1, 1), (2, 3), (127, 127), (254,)):
        srcs = [Src(rand_arrays(L, 66, 30 + s), pos0 + s, [hv.record(1, L - 1, 5, *hv.body(1))]) for s, L in enumerate(libs)]
        J, W = check(route, srcs, pos0, n, "libraries %r" % (libs,), halves=("view",))
        assert W["L"] == sum(libs) and int(W["xagg"][-1, 1]) >> 8 == sum(libs) - 1
    for libs in ((254, 1), (127, 128), (100,) * 3):
        srcs = [Src(rand_arrays(L, 8, 40), pos0) for L in libs]
        J = run(route, srcs, pos0, n)
        assert J.rc == capi.E_ARG and "BRC_JOIN_MAX_LIB" in J.err and untouched(J) and J.view.n_lib == -77, libs


def test_third_allele_records(route):
    """records on the window's first and last position, one outside on each side, unused ones, a library >= n_lib_s, a k >= n_pos_s,
    bucket bytes kept as they are, a pad word"""
    pos0, n = 200, 100
    ps, P = 190, 130                                                     # the source covers [190, 320): window elements are k - 10
    at = lambda p: p - ps
    cases = [(at(pos0), 0, 4), (at(pos0 + n - 1), 1, 5), (at(pos0 - 1), 0, 4), (at(pos0 + n), 1, 2), (NONE32, 0, 1), (NONE32, 1, 0xAB), (at(pos0 + 5), 2, 4),
             (at(pos0 + 6), 0x7FFFFF, 0xFF), (P, 0, 3), (P + 3, 1, 3), (1 << 31, 0, 4), (at(pos0 + 7), 1, 6), (at(pos0 + 8), 0, 0xFF), (at(pos0 + 9), 1, 0)]
    recs = [hv.record(k, l, b, *hv.body(t), pad=t * 7) for t, (k, l, b) in enumerate(cases)]
    other = [hv.record(3, 0, 2, *hv.body(50)), hv.record(NONE32, 0, 2, *hv.body(51))]
    J, W = check(route, [Src(rand_arrays(1, 60, 8), pos0 + 20, other), Src(rand_arrays(2, P, 9), ps, recs)], pos0, n, "records")
    used = {(int(r[0]), int(r[1]) >> 8, int(r[1]) & 0xFF) for r in W["xagg"] if r[0] != NONE32}
    assert used == {(23, 0, 2), (0, 1, 4), (n - 1, 2, 5), (7, 2, 6), (8, 1, 0xFF), (9, 2, 0)}
    # the dense expansion of the joined view is the expansion of each source at its place (hv.expand_reference), through the library
    rc, got = hv.run_dense(route, J.view, 0, n, n, kinds=("istat", "fstat", "ncol"))
    assert rc == 0
    want = hv.expand_reference({"ncol": W["ncol"], "depth": W["depth"], "slotid": W["slotid"], "si": W["si"].reshape(3, 2, NI, n), "sf": W["sf"].reshape(3, 2, NF, n)},
                               [r.tolist() for r in W["xagg"]])
    hv.assert_planes(got, {k: want[k] for k in got}, n, "joined view expanded")


CODES16 = list(range(16))


def slot_source(pos0, P, L, ref, ref_lo, ref_len=None, tag0=0):
    """insertions of length 1, 2, 3, 7 and 8 starting on an even and on an odd source nibble, all sixteen codes, reads that end inside
    the insertion, rep_read >= n_reads, rep_qpos -1 and below; deletions; unused and outside records"""
    reads = [CODES16 + CODES16[::-1], [1, 2, 4, 8, 15, 0, 3], [8] * 9, []]
    S, t = [], tag0

    def add(pos, lib, ln, rr=0, rq=0):
        nonlocal t
        t += 1
        S.append(hv.slot(pos, lib, ln, rr, rq, tag=t))
    p = pos0
    for ln in (1, 2, 3, 7, 8):
        for rq in (1, 2):                                                # inserted bases start at q = rq + 1: even / odd nibble
            add(p, (p - pos0) % L, ln, 0, rq); p += 1
    add(p, 0, 16, 0, -1); p += 1                                          # all sixteen codes from offset 0
    add(p, 0, 8, 1, 3); p += 1                                            # runs past l_qseq = 7
    add(p, 0, 3, 1, 6); p += 1                                            # wholly past it
    add(p, 0, 4, 2, -3); p += 1                                           # begins below offset 0
    add(p, 0, 2, 4, 0); p += 1                                            # rep_read == n_reads
    add(p, 0, 2, 0xFFFFFFFF, 0); p += 1
    add(p, 0, 3, 3, 0); p += 1                                            # an empty read
    add(p, L - 1, -3); p += 1
    add(p, 0, 0, 0, 1); add(p, 0, 0); p += 1                              # unused
    add(pos0 - 1, 0, 2, 0, 1); add(pos0 + P, 0, -2)                       # outside the source's own positions
    add(pos0 + 1, L, 2, 0, 1); add(pos0 + 1, -1, -1)                      # libraries that do not exist
    add(pos0 + P - 1, 0, -4); add(pos0 + P - 2, 0, 5, 2, 1)
    return hv.indel_arrays(S, reads, ref, ref_lo, ref_len, pos0, P, L, max_run=6)


def test_slot_records_and_the_synthetic_reads(route):
    refA = bytes(np.random.default_rng(1).choice(np.frombuffer(b"ACGTacgtN", np.uint8), 80))
    IA = slot_source(1000, 60, 2, refA, 990, ref_len=5000)
    IB = slot_source(1030, 50, 1, None, 0, tag0=100)
    a, b = Src(rand_arrays(2, 60, 11), 1000, I=IA), Src(rand_arrays(1, 50, 12), 1030, I=IB)
    for pos0, n in ((995, 100), (1003, 40), (1000, 60), (1100, 10)):
        J, W = check(route, [a, b], pos0, n, "slots over [%d, %d)" % (pos0, pos0 + n))
        joined = joined_indel_arrays(W, pos0, n)
        texts = {}
        for s, base in ((a, 0), (b, 2)):
            for rec in s.I["slots"]:
                p, lib, ln = hv.i32(rec[0]), hv.i32(rec[1]), hv.i32(rec[2])
                if ln and pos0 <= p < pos0 + n and s.pos0 <= p < s.pos0 + s.P and 0 <= lib < s.L:
                    texts.setdefault((p, lib + base, ln), []).append(hv.allele_text(dict(s.I, ref=joined["ref"], ref_lo=joined["ref_lo"], ref_hi=joined["ref_hi"],
                                                                                         ref_len=joined["ref_len"]) if ln < 0 else s.I, rec))
        # the joined view spells what the sources spell — by the header's rules in Python, and by brc_indels_gather where it lies
        mine = {}
        for rec in W["slots"]:
            if hv.i32(rec[2]):
                mine.setdefault((hv.i32(rec[0]), hv.i32(rec[1]), hv.i32(rec[2])), []).append(hv.allele_text(joined, rec))
        assert {k: sorted(x) for k, x in mine.items()} == {k: sorted(x) for k, x in texts.items()}
        got = spelled(route, J.indels, joined, pos0, n)
        assert sorted(got) == sorted((p, l, ln, t) for (p, l, ln), ts_ in texts.items() for t in ts_), (pos0, n)
        if (pos0, n) == (995, 100):
            assert W["counts"][0] > 30 and b"+=ACNGNNNTNNNNNNN" in [t for _, _, _, t in got] and any(t.startswith(b"+") and t.endswith(b"NN") for _, _, _, t in got)


def test_deletions_over_joined_reference_slices(route):
    """a deletion whose bases lie in the second source's slice only, in a gap between slices, past ref_len; slices that overlap and
    agree, overlap and differ (the first wins, the status bit), a NUL in the first; one source without a reference; none with one"""
    def src(pos0, P, ref, ref_lo, slots, ref_len=400, seed=1):
        return Src(rand_arrays(1, P, seed), pos0, I=hv.indel_arrays(slots, [[1, 2]], ref, ref_lo, ref_len, pos0, P, 1))
    dels = [hv.slot(105, 0, -4, tag=1), hv.slot(118, 0, -6, tag=2), hv.slot(128, 0, -5, tag=3), hv.slot(395, 0, -9, tag=4)]
    a = src(100, 300, b"ACGTACGTACGTACGTACGT", 100, dels)                                      # [100, 120)
    b = src(100, 300, b"ttttttttttGGGGGGGGGG" + b"C" * 280, 110, [hv.slot(106, 0, -3, tag=5)], seed=2)      # [110, 410): agrees nowhere with a on [110, 120)
    J, W = check(route, [a, b], 100, 300, "overlapping slices that differ")
    assert W["status"] == capi.JOIN_REF_DIFFERS and bytes(W["ref"][:20]) == b"ACGTACGTACGTACGTACGT" and (W["ref_lo"], W["ref_hi"], W["ref_len"]) == (100, 410, 400)
    assert bytes(W["ref"][300:]) == b"\0" * 10                                             # past ref_len
    got = {(p, l): t for p, l, _, t in spelled(route, J.indels, None, 100, 300)}
    assert got[(118, 0)] == b"-TGGGGG" and got[(395, 0)] == b"-CCCCNNNNN" and got[(106, 1)] == b"-TAC"
    agree = src(100, 300, b"CGTACGTACG" + b"\0" + b"ACGTACGTA", 101, [], seed=3)            # agrees with a; a NUL at 111: a's character fills it
    J, W = check(route, [agree, a], 100, 300, "overlapping slices that agree")
    assert W["status"] == 0 and bytes(W["ref"][:20]) == b"ACGTACGTACGTACGTACGT"
    gap = src(100, 300, b"GGGGG", 130, [], seed=4)
    J, W = check(route, [a, gap], 100, 300, "a gap between the slices")
    got = {(p, l): t for p, l, _, t in spelled(route, J.indels, None, 100, 300)}
    assert bytes(W["ref"][20:30]) == b"\0" * 10 and got[(128, 0)] == b"-NGGGG" and got[(118, 0)] == b"-TNNNNN"
    none = Src(rand_arrays(1, 300, 5), 100, I=hv.indel_arrays([hv.slot(128, 0, -2, tag=9)], [], None, 0, None, 100, 300, 1))
    J, W = check(route, [none, a], 100, 300, "one source without a reference")
    assert W["has_ref"] and dict(((p, l), t) for p, l, _, t in spelled(route, J.indels, None, 100, 300))[(128, 0)] == b"-NN"
    J, W = check(route, [none, Src(rand_arrays(1, 5, 6), 100, I=False)], 100, 300, "no source with a reference, one without an indels view")
    assert not W["has_ref"] and J.indels.ref is None and (J.indels.ref_lo, J.indels.ref_hi, J.indels.ref_len) == (0, 0, 0)
    other_len = src(100, 300, b"ACGT", 100, [], ref_len=401)
    R = run(route, [a, other_len], 100, 300)
    assert R.rc == capi.E_ARG and "ref_len" in R.err and untouched(R)


def test_seq_cap_one_short_counts_alone_and_two_calls(route):
    IA = slot_source(1000, 60, 2, b"ACGT" * 20, 990)
    srcs = [Src(rand_arrays(2, 60, 11), 1000, I=IA), Src(rand_arrays(1, 50, 12), 1030, I=slot_source(1030, 50, 1, None, 0, tag0=100))]
    placed = [s.place(route) for s in srcs]
    J, W = check(route, srcs, 1000, 80, "exact", placed=placed)
    nb = W["counts"][1]
    assert nb > 20
    J1, _ = check(route, srcs, 1000, 80, "one short", placed=placed, seq_cap=nb - 1)
    assert (J1.got["seq4"] == SENT8).all() and J1.counts == W["counts"]
    J0, _ = check(route, srcs, 1000, 80, "no arena", placed=placed, seq_cap=0)
    J2, _ = check(route, srcs, 1000, 80, "again", placed=placed)
    for k in capi.JOIN_DESTS:
        assert np.array_equal(J.got[k], J2.got[k]), k
    assert J.counts == J2.counts and J.status == J2.status
    # the counts alone: nothing but the two words (and the status word) is written, the host structs are not filled in
    src = capi.join_sources([(v, d) for v, d, _ in placed])
    ws, c, st = route.sentinel_bytes(int(J.z.workspace_bytes)), route.sentinel_bytes(8 + 4 * PAD), route.sentinel_bytes(4)
    v = capi.DeviceView(); v.n_lib = -77
    assert route.join.views_raw(src, 1000, 80, 80, out_view=v, counts=route.ptr(c), status=route.ptr(st), workspace=route.ptr(ws), workspace_bytes=int(J.z.workspace_bytes)) == 0
    assert route.host(c).view(np.uint32).tolist() == W["counts"] + [SENT] * PAD and route.host(st)[:4].view(np.uint32)[0] == 0 and v.n_lib == -77
    # each half alone, and without counts or status
    check(route, srcs, 1000, 80, "the indel half alone", placed=placed, halves=("indels",), status=False)
    check(route, srcs, 1000, 80, "the planes alone", placed=placed, halves=("view",), counts=False)


def test_an_empty_window(route):
    srcs = [Src(rand_arrays(1, 10, 1), 5, [hv.record(1, 0, 4, *hv.body(1))], I=slot_source(5, 10, 1, b"ACGT", 5))]
    J = run(route, srcs, 7, 0)
    assert J.rc == 0 and untouched(J) and J.counts == [0, 0] and J.status == 0
    v, d = J.view, J.indels
    assert (v.n_lib, v.pos0, v.n_pos, v.n_xagg, v.ncol, v.xagg) == (1, 7, 0, 0, None, None) and (d.n_lib, d.n_pos, d.n_slots, d.n_reads, d.slots, d.ref) == (1, 0, 0, 0, None, None)


def test_refused_calls_write_nothing(route):
    n, pos0 = 50, 100
    a, b = Src(rand_arrays(1, 40, 1), 90, [hv.record(11, 0, 4, *hv.body(1))], I=slot_source(90, 40, 1, b"ACGT" * 10, 90)), Src(rand_arrays(2, 40, 2), 120)
    good = run(route, [a, b], pos0, n)
    assert good.rc == 0
    placed, src, z = good.placed, good.src, good.z
    wsb = int(z.workspace_bytes)

    def refused(what, K=None, sources=src, p0=pos0, nn=n, stride=n, dest="all", view=True, indels=True, counts=True, seq_cap=None, ws=True, wsb=wsb, handle=True, drop=()):
        J = good
        bufs = {k: route.sentinel_bytes(J.sizes[k] + 4 * PAD) for k in capi.JOIN_DESTS}
        w, c, st = route.sentinel_bytes(wsb), route.sentinel_bytes(8), route.sentinel_bytes(4)
        d = capi.JoinDest(**{k: route.ptr(x) for k, x in bufs.items() if k not in drop}) if dest == "all" else dest
        v, i = capi.DeviceView(), capi.DeviceIndels()
        v.n_lib = i.n_lib = -77
        h = route.join.h
        if not handle:
            route.join.h = None
        try:
            rc = route.join.views_raw(sources, p0, nn, stride, dest=d, out_view=v if view else None, out_indels=i if indels else None, counts=route.ptr(c) if counts else None,
                                      seq_cap=J.sizes["seq4"] if seq_cap is None else seq_cap, status=route.ptr(st), workspace=route.ptr(w) if ws else None,
                                      workspace_bytes=wsb, K=K)
        finally:
            route.join.h = h
        assert rc == capi.E_ARG, what
        for x in list(bufs.values()) + [w, c, st]:
            assert (route.host(x) == SENT8).all(), what
        assert v.n_lib == -77 and i.n_lib == -77, what
        if handle:
            assert route.join._call("_last_error")(route.join.h), what

    refused("no handle", handle=False)
    refused("no sources", sources=None, K=2)
    refused("K = 0", K=0)
    refused("K = 17", K=17)
    refused("stride below n_pos", stride=n - 1)
    refused("n_pos below 0", nn=-1, stride=0)
    refused("a window beyond 2^31", p0=2 ** 31 - 10)
    refused("positions beyond 32-bit indices", nn=0x7ffffff0, stride=0x7ffffff0)
    refused("seq_cap below 0", seq_cap=-1)
    refused("neither half", view=False, indels=False)
    refused("no workspace", ws=False)
    refused("a short workspace", wsb=wsb - 4)
    refused("no destinations and no counts", dest=None, counts=False)
    for k in ("ncol", "depth", "slotid", "si", "sf", "xagg", "slots", "seq_off", "l_qseq", "seq4", "ref"):
        refused("no " + k, drop=(k,))
    v0, d0, _ = placed[0]

    def mutated(what, which, **fields):
        v, d = capi.DeviceView(), capi.DeviceIndels()
        C.memmove(C.byref(v), C.byref(v0), C.sizeof(v)); C.memmove(C.byref(d), C.byref(d0), C.sizeof(d))
        for k, x in fields.items():
            setattr(v if which == "view" else d, k, x)
        refused(what, sources=capi.join_sources([(v, d), placed[1][:2]]))
    viewless = capi.join_sources([placed[1][:2], placed[1][:2]])
    viewless[0].view = None
    refused("a source without a view", sources=viewless)
    mutated("n_lib 0", "view", n_lib=0)
    mutated("stride below n_pos", "view", stride=39)
    mutated("no planes", "view", si=None)
    mutated("records without an array", "view", xagg=None)
    mutated("a view elsewhere", "view", memory=3 - route.mem)
    mutated("a view on another device", "view", device=1)
    mutated("indels of another n_lib", "indels", n_lib=2)
    mutated("indels of another pos0", "indels", pos0=91)
    mutated("indels of another n_pos", "indels", n_pos=41)
    mutated("indels in other memory", "indels", memory=3 - route.mem)
    mutated("slots without an array", "indels", slots=None)
    # both sources in the memory the library does not serve
    vs = []
    for v_, d_, _ in placed:
        v, d = capi.DeviceView(), capi.DeviceIndels()
        C.memmove(C.byref(v), C.byref(v_), C.sizeof(v)); C.memmove(C.byref(d), C.byref(d_), C.sizeof(d))
        v.memory = d.memory = 3 - route.mem
        vs.append((v, d))
    refused("views of the other kind of memory", sources=capi.join_sources(vs))
    # a destination overlapping a source: the last word of a source plane, its records, its slots, its reference
    keep = placed[0][2]
    for what, k, addr in (("ncol on the source's ncol", "ncol", v0.ncol), ("sf ends inside the source's si", "sf", v0.si - good.sizes["sf"] + 4),
                          ("xagg on the source's records", "xagg", v0.xagg), ("the arena on the source's slots", "seq4", d0.slots + 71),
                          ("ref on the source's l_qseq", "ref", d0.l_qseq), ("slots on the source's reference", "slots", d0.ref - good.sizes["slots"] + 1)):
        bufs = {x: route.sentinel_bytes(good.sizes[x] + 4 * PAD) for x in capi.JOIN_DESTS}
        d = capi.JoinDest(**dict({x: route.ptr(y) for x, y in bufs.items()}, **{k: addr}))
        before = [np.array(route.host(x)) for x in hv_buffers(keep)]
        refused(what, dest=d, seq_cap=max(good.sizes["seq4"], 1))
        assert all(np.array_equal(np.array(route.host(x)), y) for x, y in zip(hv_buffers(keep), before)), what
    del keep


def hv_buffers(keep):
    out = []
    for k in keep:
        out += list(k.values())
    return out


# ------------------------------------------------------------------------------------------------ 1. one per-library engine == the join

@pytest.fixture(scope="module")
def split_batch(oracle_lib):
    """test_ivet.two_libs' kind of batch (two libraries, generated reads with indels) with test_inorm.repeats' hand-written repeat reads,
    and its oracle results: per library over all reads (what engine A must give), and all-library over each library's reads."""
    import synth
    X_REP, X_HOMO, N_CTL = tn.X_REP, tn.X_HOMO, tn.N_CTL
    rng = np.random.default_rng(33)
    ref = bytearray(synth.make_ref(rng, 3000))
    ref[X_REP - 25:X_REP + 30] = bytes(ref[X_REP - 25:X_REP + 30]).upper().replace(b"A", b"T").replace(b"C", b"G")
    ref[X_REP:X_REP + 8] = b"GACACACT"
    ref[X_HOMO - 25:X_HOMO + 30] = bytes(ref[X_HOMO - 25:X_HOMO + 30]).upper().replace(b"A", b"T")
    ref[X_HOMO:X_HOMO + 8] = b"CAAAAAAG"
    ref = bytes(ref)
    main = synth.make_batch(92, ref, 900, read_len=(60, 120), style="indel", n_libs=2)
    rows = [ti.ins_read(X_REP + 6, "AC", 0)] * 2 + [ti.ins_read(X_REP + 5, "CA", 0), ti.ins_read(X_REP + 4, "AC", 0)] + [ti.ins_read(X_REP, "AC", 1)] * N_CTL
    rows += [ti.del_read(X_HOMO + 5, 1, 0)] * 2 + [ti.del_read(X_HOMO + 3, 1, 0)] * 2 + [ti.del_read(X_HOMO, 1, 1)] * N_CTL
    arrs = ti.merged([main, ti.hand_reads(ref, rows)])
    res, _ = td.oracle_result(oracle_lib, arrs, 50, 2950, ref, **ts.PER_LIB)
    return ref, arrs, res


def one_library(arrs, l):
    """the reads of library l as a batch without library tags"""
    sub = capi.select_reads(arrs, np.flatnonzero(np.asarray(arrs["lib"]) == l))
    sub["lib"] = None
    return sub


def same(route, a, b, what, exempt=()):
    """two results of a tensors function, bit for bit"""
    assert sorted(a) == sorted(b), what
    for k in a:
        if k in exempt:
            continue
        x, y = a[k], b[k]
        if isinstance(x, dict):
            same(route, x, y, what + "." + k, exempt)
        elif isinstance(x, (int, float, str, bytes, tuple, list)) or x is None:
            assert x == y, (what, k, x, y)
        else:
            gx, gy = np.asarray(route.host(x)), np.asarray(route.host(y))
            assert gx.shape == gy.shape and gx.dtype == gy.dtype and np.array_equal(gx.reshape(-1).view(np.uint8), gy.reshape(-1).view(np.uint8)), (what, k)


def is_proper(route, x, total):
    """a list that is neither empty nor whole"""
    m = int(np.asarray(route.host(x)).shape[-1])
    assert 0 < m < total, (m, total)
    return m


def chain_over(route, eng, names):
    """every consumer of a view over one engine-like object -> {name: result}"""
    from bam_readcount_amd import tensors
    out = {}
    out["region"] = tensors.region(eng, route.dense, want=tensors.KINDS)
    out["indels"] = tensors.indels(eng, route.indels)
    out["sites"] = tensors.sites(eng, route.panel, positions=[60, 499, 500, 506, 800, 805, 2900], indels=route.indels)
    out["windows"] = tensors.sites(eng, route.panel, windows=([100, 495, 2940], [130, 510, 2950]))
    thr = dict(min_depth=4, min_alt=2)
    out["select"] = tensors.select(eng, route.select, case=[names[0]], control=[names[1]], ctl_max_alt=0, **thr)
    out["select_swapped"] = tensors.select(eng, route.select, case=[names[1]], control=[names[0]], ctl_max_alt=0, **thr)
    out["bins"] = tensors.bins(eng, route.bins, width=100, thresholds=(10, 20), hist=64)
    out["runs"] = tensors.runs(eng, route.runs, cuts=(12,), combine="min", ref_n=True)
    snv = tensors.select(eng, route.select, role=[CASE, capi.ROLE_IGNORE], indel=False, **thr)
    out["snv"] = snv
    out["vet"] = tensors.vet(eng, route.vet, idx=snv["idx"], alt=snv["why"], libs=[names[0]], **dict(tv.OPEN, min_var_count=2, min_depth=14))
    out["norm"] = norm = tensors.normalize_indels(eng, route.inorm, out["indels"])
    out["vet_indels"] = tensors.vet_indels(eng, route.ivet, norm, role=[CASE, CTL], **tiv.T_(min_var_count=2, ctl_max_count=1, ctl_frac_num=1, ctl_frac_den=2))
    return out


EXEMPT = ("unavail", "rep_read", "rep_qpos")


def split_engines(route, arrs, ref, beg0=50, end=2950, windows=None, **opts):
    """A: per library on all reads; B0, B1: all libraries as one, each on one library's reads (windows: their own regions)"""
    A = td.computed(route.engine_lib, arrs, beg0, end, ref, **dict(ts.PER_LIB, **opts))
    Bs = [td.computed(route.engine_lib, one_library(arrs, l), *(windows[l] if windows else (beg0, end)), ref, **opts) for l in (0, 1)]
    return A, Bs


def test_two_engines_joined_equal_one_per_library_engine(route, split_batch, oracle_lib):
    """THE TEST THAT FAILS WITHOUT THE FEATURE: select -> vet -> normalise -> vet_indels over two engines' results"""
    from bam_readcount_amd import tensors
    ref, arrs, res = split_batch
    A, (B0, B1) = split_engines(route, arrs, ref)
    vA = A.device_view()
    J = tensors.join([B0, B1], route.join, names=["libA", "libB"], beg0=int(vA.pos0), end=int(vA.pos0) + int(vA.n_pos))
    assert J._names == [b"libA", b"libB"]
    if route.name == "hip":
        route.torch.cuda.synchronize()
    B0.close(); B1.close()                                               # the joined region is a copy
    a, j = chain_over(route, A, ["libA", "libB"]), chain_over(route, J, ["libA", "libB"])
    for k in a:
        same(route, a[k], j[k], k, EXEMPT)
    # ... and the first two equal the oracle's per-library result
    want = td.want_planes(res, 0, res.n_pos)
    for kind in ("istat", "fstat", "depth", "ncol"):
        assert np.array_equal(tv.host_words(route, j["region"][kind]).reshape(want[kind].shape), want[kind]), kind
    T = tiv.Tab.of_oracle(res.indels)
    assert j["indels"]["m"] == T.m > 400 and np.array_equal(tv.host_words(route, j["indels"]["pos"]).view(np.int32), T.pos)
    assert bytes(np.asarray(route.host(j["indels"]["alleles"]))) == b"".join(T.texts())
    assert np.array_equal(tv.host_words(route, j["indels"]["istat"]), T.istat.view(np.uint32)) and np.array_equal(tv.host_words(route, j["indels"]["fstat"]), T.fstat.view(np.uint32))
    # the lists are neither empty nor whole
    P = int(res.n_pos)
    for k in ("select", "select_swapped", "snv"):
        is_proper(route, j[k]["idx"], P)
    keep = np.asarray(route.host(j["vet"]["keep"])).reshape(-1)
    assert 0 < int(keep.astype(bool).sum()) < keep.size
    passed = tv.host_words(route, j["vet_indels"]["fail"]).reshape(-1) == 0
    assert 0 < int(passed.sum()) < passed.size == j["norm"]["m"] < j["indels"]["m"]
    # CTL_ALLELE fires on the merged repeat record, as test_inorm shows for the single engine
    npos, nlib = np.asarray(route.host(j["norm"]["pos"])), np.asarray(route.host(j["norm"]["lib"]))
    fail = tv.host_words(route, j["vet_indels"]["fail"]).reshape(-1)
    cc = tv.host_words(route, j["vet_indels"]["ctl_count"]).reshape(-1)
    for x in (tn.X_REP, tn.X_HOMO):
        g, = np.flatnonzero((npos == x) & (nlib == 0))
        assert fail[g] & tiv.BIT["CTL_ALLELE"] and cc[g] == tn.N_CTL and not fail[g] & tiv.BIT["VAR_COUNT"], x
    A.close(); J.close()
    with pytest.raises(capi.BrcError):
        J.device_view()


def test_third_allele_records_cross_the_join(route, split_batch, monkeypatch):
    """min_bq = 10 on the knob library's short third-allele lists: n_xagg > 0 in both sources, overlay records cross the join"""
    from bam_readcount_amd import tensors
    ref, arrs, res = split_batch
    monkeypatch.setenv("BRC_TEST_XEV_CAP", "8")
    lib, route_lib = route.knob_lib, route.engine_lib
    route.engine_lib = lib
    try:
        A, Bs = split_engines(route, arrs, ref, min_bq=10)
    finally:
        route.engine_lib = route_lib
    nx = [int(b.device_view().n_xagg) for b in Bs]
    J = tensors.join(Bs, route.join, names=["libA", "libB"], beg0=int(A.device_view().pos0), end=int(A.device_view().pos0) + int(A.device_view().n_pos))
    assert int(J.device_view().n_xagg) == sum(nx)
    a, j = tensors.region(A, route.dense), tensors.region(J, route.dense)
    same(route, a, j, "region with third alleles")
    sa, sj = (tensors.select(e, route.select, role=[CASE, CTL], min_depth=8, min_alt=2, ctl_max_alt=0) for e in (A, J))
    same(route, sa, sj, "select with third alleles")
    used = int((tv.host_words(route, J.arrays["xagg"]).reshape(-1, 16)[:, 0] != NONE32).sum()) if sum(nx) else 0
    print("third-allele records: %r in the sources, %d used in the joined view" % (nx, used))
    assert min(nx) > 0 and used > 0, "the batch puts no third allele into both sources: %r" % (nx,)
    for e in [A, J] + Bs:
        e.close()


# ------------------------------------------------------------------------------------------------ 2. windows that differ

@pytest.mark.parametrize("window", [None, (200, 2100)], ids=["union", "200_2100"])
def test_windows_that_differ(route, split_batch, oracle_lib, window):
    """B0 over [50, 2950), B1 over [300, 2000): the dense expansion of the join is each source's OWN oracle result at its offset and
    zeros elsewhere; at an uncovered position a consumer gives what it gives at a position of an engine's own that no read covers"""
    from bam_readcount_amd import tensors
    ref, arrs, _ = split_batch
    wins = [(50, 2950), (300, 2000)]
    Bs = [td.computed(route.engine_lib, one_library(arrs, l), *wins[l], ref) for l in (0, 1)]
    own = [td.oracle_result(oracle_lib, one_library(arrs, l), *wins[l], ref)[0] for l in (0, 1)]
    J = tensors.join(Bs, route.join, beg0=None if window is None else window[0], end=None if window is None else window[1])
    assert J._names == [b"0", b"1"]
    v = J.device_view()
    lo = min(int(r.pos0) for r in own) if window is None else window[0]
    hi = max(int(r.pos0) + int(r.n_pos) for r in own) if window is None else window[1]
    assert (int(v.pos0), int(v.n_pos), int(v.n_lib)) == (lo, hi - lo, 2)
    got = tensors.region(J, route.dense, want=tensors.KINDS)
    n = hi - lo
    for l, r in enumerate(own):
        w = td.want_planes(r, 0, r.n_pos)
        a, b = max(lo, int(r.pos0)), min(hi, int(r.pos0) + int(r.n_pos))
        for kind in ("istat", "fstat", "metrics", "depth", "ncol"):
            g = tv.host_words(route, got[kind][l]).reshape(-1, n)
            ww = w[kind].reshape(-1, int(r.n_pos))
            assert np.array_equal(g[:, a - lo:b - lo], ww[:, a - int(r.pos0):b - int(r.pos0)]), (l, kind)
            assert not g[:, :a - lo].any() and not g[:, b - lo:].any(), (l, kind)
    assert (tv.host_words(route, got["unavail"]) == NONE32).all()
    # the indel table: each source's own list, the second library renumbered, inside the window and the source's own positions
    t = tensors.indels(J, route.indels)
    want = sorted((d["pos"], l, d["allele"].encode() if isinstance(d["allele"], str) else bytes(d["allele"])) for l, r in enumerate(own) for d in r.indels if lo <= d["pos"] < hi)
    texts = bytes(np.asarray(route.host(t["alleles"])))
    off = tv.host_words(route, t["allele_off"]).tolist()
    pos, lib = tv.host_words(route, t["pos"]).view(np.int32).tolist(), tv.host_words(route, t["lib"]).view(np.int32).tolist()
    assert [(pos[r], lib[r], texts[off[r]:off[r + 1]]) for r in range(t["m"])] == want and t["m"] > 100
    # an uncovered position of library 1 answers as a position no read covers: library 0 of B0 at its own empty positions
    sel = tensors.select(J, route.select, role=[capi.ROLE_IGNORE, CASE], min_depth=0, min_alt=1)
    idx = np.asarray(route.host(sel["idx"])).reshape(-1)
    b1 = own[1]
    assert not ((idx + lo < int(b1.pos0)) | (idx + lo >= int(b1.pos0) + int(b1.n_pos))).any()
    runs = tensors.runs(J, route.runs, cuts=(1,), libs=[1])
    st, en, cl = (np.asarray(route.host(runs[k])).reshape(-1) for k in ("start", "end", "cls"))
    assert cl[0] == 0 and st[0] == lo and en[0] >= max(lo, int(b1.pos0)) and cl[-1] == 0 and en[-1] == hi
    for e in Bs + [J]:
        e.close()


def test_tensors_join_errors(route, split_batch):
    from bam_readcount_amd import tensors
    ref, arrs, _ = split_batch
    Bs = [td.computed(route.engine_lib, one_library(arrs, l), 50, 500, ref) for l in (0, 1)]
    P2 = td.computed(route.engine_lib, arrs, 50, 500, ref, **ts.PER_LIB)
    J = tensors.join([Bs[0], P2], route.join, names=["t", b"n"])
    assert J._names == [b"t", b"n/libA", b"n/libB"] and int(J.device_view().n_lib) == 3
    for bad in (dict(engines=[]), dict(engines=Bs * 9), dict(names=["a"]), dict(names=["a", "a"]), dict(beg0=400, end=400), dict(beg0=500, end=100),
                dict(engines=[P2] * 16 * 8)):
        with pytest.raises(ValueError):
            tensors.join(bad.pop("engines", Bs), route.join, **bad)
    if route.name == "hip":                                              # a mix of host and device engines
        sim = Route("sim", engine=True)
        H = td.computed(sim.engine_lib, one_library(arrs, 0), 50, 500, ref)
        with pytest.raises(ValueError):
            tensors.join([Bs[0], H], route.join)
        H.close()
    for e in Bs + [P2, J]:
        e.close()


# ------------------------------------------------------------------------------------------------ 4. the host sanitizers

def _serialize(srcs, calls):
    """the sources and the calls as tests/sim_join/join_check.cpp reads them"""
    b = struct.pack("<i", len(srcs))
    for s in srcs:
        PS = s.P if s.stride is None else s.stride
        rec = np.array(s.records, np.uint32).reshape(len(s.records), 16)
        b += struct.pack("<iiqqQi", s.L, s.pos0, s.P, PS, len(rec), 1 if s.I else 0)
        for name, per in PLANES:
            out = np.full((s.L * per, PS), hv.POISON, np.uint32); out[:, :s.P] = np.asarray(s.A[name], np.uint32).reshape(s.L * per, s.P)
            b += out.tobytes()
        b += rec.tobytes()
        if s.I:
            I = s.I
            b += struct.pack("<QqQiqqq", len(I["slots"]), I["n_reads"], len(I["seq4"]), 1 if I["ref"] is not None else 0, I["ref_lo"], I["ref_hi"], I["ref_len"])
            b += I["slots"].tobytes() + I["seq_off"].tobytes() + I["l_qseq"].tobytes() + I["seq4"].tobytes() + (I["ref"] if I["ref"] is not None else b"")
    b += struct.pack("<i", len(calls))
    for pos0, n, stride, seq_cap in calls:
        b += struct.pack("<iqqq", pos0, n, stride, seq_cap)
    return b


def test_calls_under_the_host_sanitizers(sim_route, tmp_path):
    """the offset, edge and record cases above through the stand-alone program of the CPU build with -fsanitize=address,undefined:
    sources, scratch and destinations are heap blocks of exactly the contract's sizes; results equal the reference's"""
    refA = b"ACGTNacgt" * 9
    a = Src(rand_arrays(2, 290, 1), 935, [hv.record(k, l, bk, *hv.body(t)) for t, (k, l, bk) in enumerate([(65, 0, 4), (289, 1, 5), (NONE32, 0, 1), (3, 2, 0), (290, 0, 1)])],
            stride=293, I=slot_source(935, 290, 2, refA, 930, ref_len=5000))
    b = Src(rand_arrays(1, 300, 2), 1000, [hv.record(0, 0, 2, *hv.body(9))], I=slot_source(1000, 300, 1, b"ACGTACGTAC", 1005, ref_len=5000, tag0=100))
    c = Src(rand_arrays(3, 64, 3), 1100, I=False)
    srcs = [a, b, c]
    calls = [(1000, 300, 300, -1)] + [(935 + off, n, n | 1, -1) for off, n in zip(OFFSETS, (1, 3, 4, 5, 63, 64, 65, 255, 256, 257))]
    calls += [(900, 1023, 1023, -1), (999, 1025, 1027, 0), (1001, 130, 131, -2), (1000, 0, 0, -1)]
    out = hv.run_checker("join", _serialize(srcs, calls), tmp_path, "%d calls" % len(calls))
    o = 0

    def take(nbytes):
        nonlocal o
        x = out[o:o + nbytes]; o += nbytes
        return x
    for pos0, n, stride, seq_cap in calls:
        W = reference(srcs, pos0, n) if n else None
        rc, status, c0, c1, cap = struct.unpack("<iIIIq", bytes(take(24)))
        assert rc == 0, (pos0, n)
        if not n:
            assert (status, c0, c1) == (0, 0, 0)
            continue
        L = W["L"]
        fits = seq_cap == -1
        assert [c0, c1] == W["counts"] and status == W["status"] and cap == (c1 if seq_cap == -1 else (0 if seq_cap == 0 else c1 - 1))
        for name, per in PLANES:
            g = take(4 * buffer_words(L * per, stride, n)).view(np.uint32)
            want = np.full((L * per, stride), SENT, np.uint32); want[:, :n] = W[name]
            assert np.array_equal(g, want.ravel()[:g.size]), (pos0, n, name)
        for k in ("xagg", "slots", "seq_off", "l_qseq"):
            w = np.ascontiguousarray(W[k]).ravel().view(np.uint8)
            assert np.array_equal(take(w.size), w), (pos0, n, k)
        g = take(cap)
        assert np.array_equal(g, W["seq4"]) if fits else (g == SENT8).all(), (pos0, n)
        assert np.array_equal(take(len(W["ref"])), W["ref"]), (pos0, n)
    assert o == out.size
