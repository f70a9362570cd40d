"""The side libraries on a caller's stream: brc_dense_expand, brc_indels_gather, brc_panel_gather, brc_select_sites, brc_bins_reduce and
brc_runs_find promise to return once their work is queued on `stream`, never to wait, and that work queued on that stream afterwards
sees the result; bam_readcount_amd.tensors hands them torch's current stream.  Every other [hip] test passes the default stream, which
serialises against everything: a launch or memset on stream 0, a hidden wait, a timing event on the wrong stream would leave them green.

The technique: LATE INPUTS BEHIND A BOUNDED HOLD.  Hand-made views (test_select.build_views: 600 positions = three workgroups, two
libraries, third-allele records, indel records, a reference slice) lie in torch tensors.  The buffers whose every content is defined
behaviour are overwritten with a DECOY — depth, ncol and the slots' count words zero, the reference all N, every indel record of the
dead filler form, the panel's list all index 0, the bins' edges all equal — and the device is synchronised.  Then, on a
torch.cuda.Stream() (non-blocking, and probed to run beside the default stream: see streams_beside_the_default) and without touching
the default stream or the host: a hold (torch.cuda._sleep), the real contents copied back, the
0xA5 fill of every destination and of the scratch, an event, the library call, and a copy of every destination.  Right behind the call's
return the event must still be pending (the call did not wait, the hold held: a test whose event has fired FAILS as inconclusive); after
the stream's synchronisation the copies must be, byte for byte and sentinels included, what the modules' numpy references give for the
REAL contents.  Whatever ran beside the stream met the decoy, or cleared a word that the sentinel fill then covered.

No reference is written here: the values come from test_select.reference / Dense.want, test_runs.reference, test_bins.reference,
test_dense.want_planes, test_panel.want_at and test_indels.table_of, fed with the dense counts the views were built from (`HandRes`
dresses them as the oracle result those functions read: build_views writes counts alone, so the float sums are zero and every allele
of an insertion spells N).  Two tests run in the CPU suite: the references of the decoy differ from the real ones in every compared
output (without that a misplaced launch could pass), and the CPU builds of the six libraries give the expected bytes in both states.

fstat and unavail of the dense and panel planes are compared but cannot tell decoy from real: build_views has no float sums and no
unavail plane (the CPU test asserts that they are the only such outputs).

The hold, as calibrated on an MI355X (the `gpu` fixture prints its figures on every run): 118 168 673 ticks of torch.cuda._sleep,
measured at 49.2 ms between two events (wanted: 50 ms).  The warm host-side times of the six calls it was sized against: dense 33 us,
panel 26 us, select 50 us, bins 49 us, runs 27 us, indels 53 us — twenty times the slowest is 1.1 ms.  The hold must also outlast the
host's queueing of the seven input copies, up to twenty fills and the call itself — at a pessimistic half millisecond each some 15 ms —
so it never goes below 50 ms; it is capped at 0.25 s.  kernel_s of the six calls behind that hold: 13 to 33 us.

Which bam_readcount_amd.tensors functions may wait for their stream (read off tensors.py: the host reads device memory in one place,
_Device.read, which only the count-then-fill helper _sized_by_data calls; host lists go up in one place, _Device.upload):
  region                      never: every size is known on the host                                     -> asserted
  bins(width=) and bins(edges= a device tensor)   never                                                 -> asserted for width=
  vet(idx=, alt= device tensors), sites(positions= a device tensor)   never: every size follows from the list's length -> asserted for vet
  bins(edges= a host list), vet(idx= a host list), sites(positions= / windows= on the host)   upload pageable host memory: the copy may wait
  sites(indels=), indels, select, runs            SYNCHRONISE ONCE by contract: the host reads a count to size the arrays

Not here: graph capture (not promised), the inflate and deflate libraries (a stream of their own), sanitizers, machine code."""
import subprocess
import time

import numpy as np
import pytest

from bam_readcount_amd import capi
from route import Route, SENT8
import synth
import test_bins as tb
import test_dense as td
import test_indels as ti
import test_panel as tp
import test_runs as tr
import test_select as ts
import test_vet as tv

P, POS0, L = 600, 1000, 2                 # three workgroups of 256 positions, two libraries
K0, N = 5, 590                            # the window of the calls: off the 64-grid at both ends
PAD = 3
REF_SLICE = (10, 580)                     # the reference slice covers plane positions [10, 580)
INDELS = [(2, 0, 1, 5), (5, 0, 2, 3), (63, 1, -1, 2), (64, 0, -3, 4), (255, 0, 4, 5), (256, 0, 1, 3), (256, 0, -2, 2), (300, 0, 3, 2), (300, 0, 2, 4),
          (300, 1, 2, 1), (599, 1, -1, 1)]                                  # (plane index, library, length, reads)
EDGES = [0, 64, 64, 256, 300, 599]        # both ends outside the window: BRC_BINS_OUTSIDE, the values stay defined
THR, N_HIST = (0, 1, 4, 10), 16
N_IDX = 300
SEL_ROLE, SEL_P = [1, 2], ts.EDGE_P
SEL2_ROLE, SEL2_P = [2, 1], ts.P_(ts.BOTH, min_depth=2, min_alt=1, frac=(1, 10), ctl_frac=(1, 2))
RUNS_CUTS, RUNS2_CUTS = (2, 6), (1, 3, 8)
LATE = ("depth", "ncol", "si", "ref", "slots", "idx", "edges")
HOLD_FLOOR, HOLD_CAP = 0.05, 0.25         # seconds


LIBS = ("dense", "select", "runs", "bins", "panel", "indels", "vet")          # what a Scene's jobs call


def _route(name):
    """LIBS and the engine, with a second handle of the two libraries that take a workspace"""
    r = Route(name, LIBS, engine=True)
    r.select2, r.runs2 = r.another("select"), r.another("runs")
    return r


# ------------------------------------------------------------------------------------------------ the views, real and decoy

class HandRes:
    """A test_select.Dense of build_views as the oracle result that test_dense.want_planes, test_panel.want_at and test_indels.table_of
    read: the counts are all that build_views writes (float sums zero, no unavail plane, ncol a copy of depth); an indel record has
    rep_read 0 of a view without reads, so an inserted base spells N, and a deleted one is the reference's character."""

    def __init__(self, h):
        self.n_lib, self.n_pos, self.pos0 = h.n_lib, h.n_pos, h.pos0
        self.depth = self.ncol = np.asarray(h.depth, np.uint32)
        self.unavail = None
        self.refbase = h.refbase
        self.istat = np.zeros((h.n_lib, 6, 9, h.n_pos), np.uint32)
        self.istat[:, 1:5, 0, :] = h.cnt
        self.fstat = np.zeros((h.n_lib, 6, 4, h.n_pos), np.float32)
        recs = []
        for pos, lib, ln, count in h.indels:
            if ln > 0:
                text = "+" + "N" * ln
            else:
                text = "-" + "".join(chr(h.refbase[pos + 1 + j - h.pos0]) if 0 <= pos + 1 + j - h.pos0 < h.n_pos else "N" for j in range(-ln))
            recs.append(dict(pos=pos, lib=lib, len=ln, rep_read=0, rep_qpos=0, i=[count] + [0] * 8, f=[0.0] * 4, allele=text))
        self.indels = sorted(recs, key=lambda d: (d["pos"], d["lib"], d["allele"].encode("latin1")))


class World:
    """what the references read in one state of the buffers: the dense counts, the panel's list, the bins' edges"""

    def __init__(self, h, idx, edges):
        self.h, self.idx, self.edges = h, np.asarray(idx, np.int32), np.asarray(edges, np.int32)
        self.D = tb.Dense.of_hand(h)
        self.res = HandRes(h)


def _flat(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


class Scene:
    """Hand-made views and the two lists in the route's memory; .real / .decoy: the World of either state.  to_decoy / to_real switch
    the LATE buffers in place and synchronise; restore() QUEUES the real contents on torch's current stream."""

    def __init__(self, route, seed):
        self.route = route
        depth, cnt, ref = ts.low_depth(P, seed=seed)
        ind = [(POS0 + k, l, ln, c) for k, l, ln, c in INDELS]
        self.v, self.d, h, self.keep = ts.build_views(route, depth, cnt, ref[REF_SLICE[0]:REF_SLICE[1]], ref_lo=POS0 + REF_SLICE[0], indels=ind, pos0=POS0)
        assert self.v.n_xagg > 3 and self.d.n_slots == len(INDELS) + 3 and self.d.ref            # third-allele records, indel records, a reference
        self.keep["ref"] = route.put(np.array(_flat(route.host(self.keep["ref"]))))              # (build_views' slice may be read-only host memory)
        self.d.ref = route.ptr(self.keep["ref"])
        rng = np.random.default_rng(seed)
        idx = np.concatenate([np.sort(rng.integers(0, P, N_IDX - 1)), [P]]).astype(np.int32)      # ascending, repeats, the last one out of range
        self.keep["idx"] = route.put(idx)
        self.keep["edges"] = route.put(np.asarray(EDGES, np.int32))
        self.keep["edges0"] = route.put(np.full(3, 7, np.int32))                                 # (the n == 0 call's list: never late)
        self.real = World(h, idx, EDGES)
        self.bytes = {k: _flat(route.host(self.keep[k])).copy() for k in LATE}
        dec = {k: np.zeros_like(self.bytes[k]) for k in ("depth", "ncol", "si", "idx")}
        dec["ref"] = np.full_like(self.bytes["ref"], ord("N"))
        dead = np.zeros((int(self.d.n_slots), 18), np.uint32); dead[:, 0] = POS0 + 1; dead[:, 5] = 99          # build_views' unused record
        dec["slots"] = _flat(dead)
        dec["edges"] = _flat(np.full(len(EDGES), K0, np.int32))
        assert all(dec[k].size == self.bytes[k].size for k in LATE)
        self.decoy_bytes = dec
        # what is left of the counts in the decoy: the third-allele records (their position indices are not decoyed, nor are their counts)
        x = _flat(route.host(self.keep["xagg"])).view(np.uint32).reshape(-1, 16)
        dcnt = np.zeros_like(h.cnt)
        for k, lb, c in x[x[:, 0] != ts.NONE32][:, :3]:
            dcnt[lb >> 8, (lb & 0xFF) - 1, k] = c
        assert dcnt.any() and ((dcnt == 0) | (dcnt == h.cnt)).all()
        self.records_at = np.nonzero(dcnt.any(axis=(0, 1)))[0]
        self.decoy = World(ts.Dense(np.zeros_like(h.depth), dcnt, b"N" * P, [], POS0), np.zeros(N_IDX, np.int32), np.full(len(EDGES), K0, np.int32))
        if route.name == "hip":
            self.staged = {k: self.keep[k].clone() for k in LATE}
            self.decoys = {k: route.torch.from_numpy(dec[k]).cuda() for k in LATE}

    def _set(self, which):
        if self.route.name == "hip":
            for k in LATE:
                self.keep[k].copy_(self.decoys[k] if which == "decoy" else self.staged[k])
            self.route.torch.cuda.synchronize()
        else:
            for k in LATE:
                _flat(self.keep[k])[:] = self.decoy_bytes[k] if which == "decoy" else self.bytes[k]

    def to_decoy(self):
        self._set("decoy")

    def to_real(self):
        self._set("real")

    def restore(self):
        for k in LATE:
            self.keep[k].copy_(self.staged[k], non_blocking=True)


# ------------------------------------------------------------------------------------------------ the calls and what they must leave

def blank(n_bytes):
    return np.full(n_bytes, SENT8, np.uint8)


def word(x, n=1):
    return np.asarray([x] * n if np.isscalar(x) else x, np.uint32).view(np.uint8).copy()


class Job:
    """One call (or a chain of calls) of the side libraries: sizes(route) -> {buffer: bytes}; enqueue(route, buf, stream) -> the code;
    expect(world) -> {buffer: the bytes it must hold afterwards, sentinels included} for every buffer but the scratch.
    same: outputs that the hand-made views leave equal in both states; reads: False for the n == 0 forms, which read no input."""

    def __init__(self, name, lib, sizes, enqueue, expect, same=(), reads=True):
        self.name, self.lib, self.sizes, self.enqueue, self.expect, self.same, self.reads = name, lib, sizes, enqueue, expect, same, reads


def planes_expected(want, n, ds, pre=""):
    out = {}
    for k in td.KINDS:
        e = blank(4 * want[k].shape[0] * ds)
        e.view(np.uint32).reshape(-1, ds)[:, :n] = want[k]
        out[pre + k] = e
    return out


def plane_sizes(ds, pre=""):
    return {pre + k: 4 * td.planes_of(k, L) * ds for k in td.KINDS}


def dense_job(sc):
    ds = N + PAD

    def enqueue(route, buf, stream):
        return route.dense.expand_raw(sc.v, K0, N, ds, stream=stream, **{k: route.ptr(buf[k]) for k in td.KINDS})
    return Job("dense", "dense", lambda route: plane_sizes(ds), enqueue, lambda w: planes_expected(td.want_planes(w.res, K0, N), N, ds), same=("fstat", "unavail"))


def panel_status(idx):
    idx = np.asarray(idx, np.int64)
    return (tp.OOR if ((idx < 0) | (idx >= P)).any() else 0) | (tp.DESC if (idx[1:] < idx[:-1]).any() else 0)


def panel_job(sc, form="list"):
    n = N_IDX if form == "list" else 0
    ds = n + PAD

    def enqueue(route, buf, stream):
        return route.panel.gather_raw(sc.v, route.ptr(sc.keep["idx"]), n, ds, status=route.ptr(buf["status"]), stream=stream, **{k: route.ptr(buf[k]) for k in td.KINDS})

    def expect(w):
        out = planes_expected(tp.want_at(w.res, w.idx[:n]), n, ds)
        out["status"] = word(panel_status(w.idx[:n]))
        return out
    return Job("panel " + form, "panel", lambda route: dict(plane_sizes(ds), status=4), enqueue, expect, same=("fstat", "unavail"), reads=n > 0)


def select_job(sc, form="list", role=SEL_ROLE, p=SEL_P, lib="select", pre=""):
    """form: "list" (cap = the real total), "counts" (the count alone), "empty" (n == 0)"""
    k0, n = (7, 0) if form == "empty" else (K0, N)
    cap = {"list": len(sc.real.h.want(role, p, K0, N)[0]), "counts": 0, "empty": 4}[form]
    lists = form != "counts"

    def sizes(route):
        s = {pre + "counts": 4, pre + "ws": getattr(route, lib).workspace(sc.v, sc.d, n)}
        if lists:
            s[pre + "idx"] = s[pre + "why"] = 4 * (cap + PAD)
        return s

    def enqueue(route, buf, stream):
        par, keep = capi.select_params(role, p["flags"], p["min_depth"], p["min_alt"], p["frac"], p["ctl_min_depth"], p["ctl_max_alt"], p["ctl_frac"])
        h = getattr(route, lib)
        rc = h.sites_raw(sc.v, sc.d, par, k0, n, cap=cap, idx=route.ptr(buf[pre + "idx"]) if lists else None, why=route.ptr(buf[pre + "why"]) if lists else None,
                         counts=route.ptr(buf[pre + "counts"]), workspace=route.ptr(buf[pre + "ws"]) if h.workspace(sc.v, sc.d, n) else None, stream=stream)
        del keep
        return rc

    def expect(w):
        widx, wwhy = w.h.want(role, p, k0, n)
        t = min(len(widx), cap)
        out = {pre + "counts": word(len(widx))}
        if lists:
            for k, x in (("idx", widx), ("why", wwhy)):
                e = blank(4 * (cap + PAD)); e.view(np.uint32)[:t] = x[:t].astype(np.int32).view(np.uint32); out[pre + k] = e
        return out
    j = Job("select " + form, lib, sizes, enqueue, expect, reads=n > 0)
    if form == "list":
        j.cap = cap
    return j


def runs_job(sc, form="list", cuts=RUNS_CUTS, combine=tr.MIN, keep=None, lib="runs", pre=""):
    """form: "list" (cap = the real total, every output), "counts" (counts and per_class alone: the call ends after k_runs_parts),
    "empty" (n == 0).  With BRC_RUNS_REF_N: the class of a position depends on the reference too."""
    k0, n = (7, 0) if form == "empty" else (K0, N)
    cap = {"list": len(tr.reference(sc.real.h, K0, N, cuts, combine, None, keep, True)[0]), "counts": 0, "empty": 4}[form]
    lists = form != "counts"
    nc = len(cuts) + 2

    def sizes(route):
        s = {pre + "counts": 4, pre + "per": 8 * (tr.MAXC + PAD), pre + "ws": getattr(route, lib).workspace(n)}
        if lists:
            s[pre + "start"] = s[pre + "end"] = s[pre + "cls"] = 4 * (cap + PAD)
        return s

    def enqueue(route, buf, stream):
        par, keepalive = capi.runs_params(cuts, combine, None, keep, capi.RUNS_REF_N)
        h = getattr(route, lib)
        at = lambda k: route.ptr(buf[pre + k]) if lists else None
        rc = h.find_raw(sc.v, sc.d, par, k0, n, cap=cap, start=at("start"), end=at("end"), cls=at("cls"), counts=route.ptr(buf[pre + "counts"]),
                        per_class=route.ptr(buf[pre + "per"]), workspace=route.ptr(buf[pre + "ws"]) if h.workspace(n) else None, stream=stream)
        del keepalive
        return rc

    def expect(w):
        w0, w1, wc, wp = tr.reference(w.h, k0, n, cuts, combine, None, keep, True)
        t = min(len(w0), cap)
        e = blank(8 * (tr.MAXC + PAD)); e.view(np.uint64)[:nc] = wp
        out = {pre + "counts": word(len(w0)), pre + "per": e}
        if lists:
            for k, x in (("start", w0), ("end", w1), ("cls", wc)):
                e = blank(4 * (cap + PAD)); e.view(np.uint32)[:t] = x[:t].astype(np.int32).view(np.uint32); out[pre + k] = e
        return out
    j = Job("runs " + form, lib, sizes, enqueue, expect, reads=n > 0)
    if form == "list":
        j.cap = cap
    return j


def bins_status(e, k0, n):
    e = np.asarray(e, np.int64)
    return (capi.BINS_DESCENDS if (e[1:] < e[:-1]).any() else 0) | (capi.BINS_OUTSIDE if ((e < k0) | (e > k0 + n)).any() else 0)


def bins_sizes(nb, n_hist, pre=""):
    ds = nb + PAD
    return {pre + "sums": 8 * L * tb.NSUM * ds, pre + "covered": 8 * L * len(THR) * ds, pre + "hist": 8 * L * n_hist, pre + "status": 4}


def bins_enqueue(route, sc, buf, stream, k0, n, edges_ptr, nb, n_hist, pre=""):
    par = capi.bins_params(0, edges_ptr, nb, list(THR), n_hist)
    return route.bins.reduce_raw(sc.v, sc.d, par, k0, n, nb + PAD, sums=route.ptr(buf[pre + "sums"]), covered=route.ptr(buf[pre + "covered"]),
                                 hist=route.ptr(buf[pre + "hist"]), status=route.ptr(buf[pre + "status"]), stream=stream)


def bins_expected(w, k0, n, edges, n_hist, pre=""):
    """the values of a list that does not descend: edges outside count as the window's ends (the header; test_bins' status test)"""
    st = bins_status(edges, k0, n)
    assert not st & capi.BINS_DESCENDS
    nb = len(edges) - 1
    ds = nb + PAD
    r = tb.reference(w.D, k0, n, 0, np.clip(np.asarray(edges, np.int64), k0, k0 + n), THR, n_hist)
    out = {pre + "status": word(st)}
    for k, rows in (("sums", tb.NSUM), ("covered", len(THR))):
        e = blank(8 * L * rows * ds); e.view(np.uint64).reshape(L, rows, ds)[:, :, :nb] = r[k]; out[pre + k] = e
    out[pre + "hist"] = np.ascontiguousarray(r["hist"]).view(np.uint8).reshape(-1).copy()
    return out


def bins_job(sc, form="list"):
    k0, n, key, n_hist = (K0, N, "edges", N_HIST) if form == "list" else (7, 0, "edges0", 4)
    nb = (len(EDGES) if form == "list" else 3) - 1
    return Job("bins " + form, "bins", lambda route: bins_sizes(nb, n_hist),
               lambda route, buf, stream: bins_enqueue(route, sc, buf, stream, k0, n, route.ptr(sc.keep[key]), nb, n_hist),
               lambda w: bins_expected(w, k0, n, w.edges if form == "list" else [7, 7, 7], n_hist), reads=n > 0)


def indels_job(sc, form="list"):
    """form: "list" (exact capacities of the real table, every destination), "counts" (the two totals alone), "empty" (n == 0)"""
    k0, n = (7, 0) if form == "empty" else (0, P)
    real = ti.table_of(ti.window_of(sc.real.res, 0, P))
    cap, acap = {"list": (real["pos"].shape[1], int(real["alleles"].size)), "counts": (0, 0), "empty": (4, 16)}[form]
    dests = () if form == "counts" else ti.DESTS

    def sizes(route):
        s = {k: 4 * (ti.PLANES[k] * cap + PAD) for k in ti.PLANES if k in dests}
        if dests:
            s["allele_off"] = 4 * (cap + 1 + PAD); s["alleles"] = acap + PAD
        s["counts"] = 8; s["ws"] = route.indels.workspace(sc.d, n)
        return s

    def enqueue(route, buf, stream):
        wsb = route.indels.workspace(sc.d, n)
        return route.indels.gather_raw(sc.d, k0, n, workspace=route.ptr(buf["ws"]) if wsb else None, workspace_bytes=wsb, counts=route.ptr(buf["counts"]),
                                       cap=cap, alleles_cap=acap, stream=stream, **{k: route.ptr(buf[k]) for k in dests})

    def expect(w):
        """test_indels.assert_table as bytes: the prefix the capacities allow, everything else the sentinel"""
        want = ti.table_of(ti.window_of(w.res, k0, n))
        m = want["pos"].shape[1]; t = min(m, cap)
        out = {"counts": word([m, int(want["alleles"].size)])}
        if not dests:
            return out
        for k, pl in ti.PLANES.items():
            e = blank(4 * (pl * cap + PAD)); e[:4 * pl * cap].view(np.uint32).reshape(pl, cap)[:, :t] = want[k][:, :t]; out[k] = e
        e = blank(4 * (cap + 1 + PAD)); e.view(np.uint32)[:t + 1] = want["allele_off"][:t + 1]; out["allele_off"] = e
        e = blank(acap + PAD)
        for r in range(t):
            a, b = int(want["allele_off"][r]), int(want["allele_off"][r + 1])
            if b <= acap:
                e[a:b] = want["alleles"][a:b]
        out["alleles"] = e
        return out
    return Job("indels " + form, "indels", sizes, enqueue, expect, reads=n > 0)


# ------------------------------------------------------------------------------------------------ the chains

def chain_select_panel(sc):
    """brc_select_sites -> brc_panel_gather over `cap` elements of the list where it lies: the count is read by nobody"""
    sel = select_job(sc)
    cap = sel.cap
    ds = cap + PAD

    def enqueue(route, buf, stream):
        rc = sel.enqueue(route, buf, stream)
        return rc or route.panel.gather_raw(sc.v, route.ptr(buf["idx"]), cap, ds, status=route.ptr(buf["p.status"]), stream=stream,
                                            **{k: route.ptr(buf["p." + k]) for k in td.KINDS})

    def expect(w):
        out = sel.expect(w)
        lst = out["idx"][:4 * cap].view(np.int32)               # (what the selection did not write is the sentinel: an index out of range)
        out.update(planes_expected(tp.want_at(w.res, lst), cap, ds, "p."))
        out["p.status"] = word(panel_status(lst))
        return out
    return Job("select -> panel", "panel", lambda route: dict(sel.sizes(route), **dict(plane_sizes(ds, "p."), **{"p.status": 4})), enqueue, expect,
               same=("p.fstat", "p.unavail"))


def interleaved(start, end):
    return np.stack([start, end], axis=1).reshape(-1)


def chain_runs_bins(sc):
    """brc_runs_find (one class kept) -> the start / end words interleaved by a torch op on the stream -> brc_bins_reduce with status:
    even bins are the runs, odd bins the gaps"""
    runs = runs_job(sc, keep=1 << 1)
    m = runs.cap
    nb = 2 * m - 1

    def enqueue(route, buf, stream):
        rc = runs.enqueue(route, buf, stream)
        if rc:
            return rc
        if route.name == "hip":
            i32 = route.torch.int32
            route.torch.stack([buf["start"].view(i32)[:m], buf["end"].view(i32)[:m]], dim=1, out=buf["edges"].view(i32)[:2 * m].view(m, 2))
        else:
            buf["edges"].view(np.int32)[:2 * m] = interleaved(buf["start"].view(np.int32)[:m], buf["end"].view(np.int32)[:m])
        return bins_enqueue(route, sc, buf, stream, K0, N, route.ptr(buf["edges"]), nb, N_HIST, "b.")

    def expect(w):
        out = runs.expect(w)
        e = interleaved(out["start"][:4 * m].view(np.int32), out["end"][:4 * m].view(np.int32))
        out["edges"] = e.view(np.uint8).copy()
        out.update(bins_expected(w, K0, N, e, N_HIST, "b."))
        return out
    return Job("runs -> bins", "bins", lambda route: dict(runs.sizes(route), edges=8 * m, **bins_sizes(nb, N_HIST, "b.")), enqueue, expect)


def inside_runs(start, end, idx):
    """1 where a listed position lies in one of the intervals; every index clamped to [0, P], so that no content is a wild address"""
    delta = np.zeros(P + 1, np.int64)
    np.add.at(delta, np.clip(start, 0, P), 1); np.add.at(delta, np.clip(end, 0, P), -1)
    return np.cumsum(delta)[np.clip(idx, 0, P)].astype(np.int32)


def chain_runs_select(sc):
    """brc_runs_find (the classes from the first cut up) and brc_select_sites over the same window, then torch ops on the stream that
    mark the selected positions inside the runs: the runs as a mask for the selection's list"""
    runs = runs_job(sc, keep=0b0110, pre="r.")
    sel = select_job(sc)
    mr, ms = runs.cap, sel.cap

    def enqueue(route, buf, stream):
        rc = runs.enqueue(route, buf, stream) or sel.enqueue(route, buf, stream)
        if rc:
            return rc
        if route.name == "hip":
            torch = route.torch
            i32 = torch.int32
            st, en, ix = (buf[k].view(i32)[:c].long().clamp(0, P) for k, c in (("r.start", mr), ("r.end", mr), ("idx", ms)))
            delta = torch.zeros(P + 1, dtype=torch.int64, device=st.device)
            delta.index_add_(0, st, torch.ones_like(st)); delta.index_add_(0, en, -torch.ones_like(en))
            buf["inside"].view(i32)[:ms].copy_(delta.cumsum(0)[ix])
        else:
            buf["inside"].view(np.int32)[:ms] = inside_runs(*(buf[k].view(np.int32)[:c].astype(np.int64) for k, c in (("r.start", mr), ("r.end", mr), ("idx", ms))))
        return 0

    def expect(w):
        out = dict(runs.expect(w), **sel.expect(w))
        st, en, ix = (out[k][:4 * c].view(np.int32).astype(np.int64) for k, c in (("r.start", mr), ("r.end", mr), ("idx", ms)))
        out["inside"] = inside_runs(st, en, ix).view(np.uint8).copy()
        return out
    return Job("runs -> select", "select", lambda route: dict(runs.sizes(route), inside=4 * ms, **sel.sizes(route)), enqueue, expect)


SINGLE = {"dense": dense_job, "panel": panel_job, "select": select_job, "bins": bins_job, "runs": runs_job, "indels": indels_job}
EARLY = {"panel n == 0": lambda sc: panel_job(sc, "empty"), "select n == 0": lambda sc: select_job(sc, "empty"), "select counts alone": lambda sc: select_job(sc, "counts"),
         "bins n == 0": lambda sc: bins_job(sc, "empty"), "runs n == 0": lambda sc: runs_job(sc, "empty"), "runs counts and per_class alone": lambda sc: runs_job(sc, "counts"),
         "indels n == 0": lambda sc: indels_job(sc, "empty"), "indels counts alone": lambda sc: indels_job(sc, "counts")}
CHAINS = {"select -> panel": chain_select_panel, "runs -> bins": chain_runs_bins, "runs -> select": chain_runs_select}
SECOND = {"select": lambda sc: select_job(sc, role=SEL2_ROLE, p=SEL2_P, lib="select2"), "runs": lambda sc: runs_job(sc, cuts=RUNS2_CUTS, combine=tr.SUM, lib="runs2")}
ALL_JOBS = dict(SINGLE, **EARLY, **CHAINS)


def run_plain(route, job, stream=None):
    """the job into 0xA5-filled buffers; returns (the code, {buffer: bytes}, the host's seconds inside the call)"""
    sizes = job.sizes(route)
    buf = {k: route.sentinel_bytes(max(n, 8)) for k, n in sizes.items()}
    t0 = time.perf_counter()
    rc = job.enqueue(route, buf, stream)
    dt = time.perf_counter() - t0
    return rc, {k: route.host(b)[:sizes[k]] for k, b in buf.items()}, dt


def compare(got, want, what):
    for k, e in want.items():
        g = got[k][:e.size]
        assert np.array_equal(g, e), "%s: %s differs from the reference at bytes %r (%d of %d differ)" % (what, k, np.nonzero(g != e)[0][:6].tolist(), int((g != e).sum()), e.size)


# ------------------------------------------------------------------------------------------------ the CPU suite

@pytest.fixture(scope="module")
def sim_route():
    return _route("sim")


def test_the_decoy_reference_differs_in_every_compared_output(sim_route):
    """Without this a launch that met the decoy could pass: for every job that reads its inputs, every compared buffer of the decoy's
    reference differs from the real one — but fstat and unavail, which build_views cannot fill; the forms with n == 0 read nothing
    and are protected by the order of the sentinel fill instead: what they clear must show over the sentinel."""
    for seed in (21, 22):
        sc = Scene(sim_route, seed)
        assert set(sc.real.idx[:-1].tolist()) & set(sc.records_at.tolist()), "the panel's list meets no third-allele record"
        widx, wwhy = sc.real.h.want(SEL_ROLE, SEL_P, K0, N)
        assert int(np.bitwise_or.reduce(wwhy)) & (capi.WHY_INS | capi.WHY_DEL) == capi.WHY_INS | capi.WHY_DEL and int(np.bitwise_or.reduce(wwhy)) & 15
        assert set(widx.tolist()) & set(sc.records_at.tolist()), "no selected position carries a third-allele record"
        jobs = dict({k: f(sc) for k, f in ALL_JOBS.items()}, **{k + " (second handle)": f(sc) for k, f in SECOND.items()})
        for name, job in jobs.items():
            real = job.expect(sc.real)
            if not job.reads:
                assert real == {} or any((e != SENT8).any() for e in real.values()), name
                continue
            decoy = job.expect(sc.decoy)
            assert sorted(real) == sorted(decoy), name
            for k in real:
                assert real[k].size == decoy[k].size, (name, k)
                if k in job.same:
                    assert np.array_equal(real[k], decoy[k]), (name, k)
                else:
                    assert not np.array_equal(real[k], decoy[k]), "%s: the decoy's %s equals the real one: a launch that met the decoy would pass" % (name, k)
            if hasattr(job, "cap"):
                assert job.cap >= 3, name
        # what the chains hand on is worth handing on
        assert jobs["runs -> bins"].expect(sc.real)["b.status"].view(np.uint32)[0] == 0
        inside = jobs["runs -> select"].expect(sc.real)["inside"].view(np.int32)
        assert 0 < inside.sum() < inside.size and set(inside.tolist()) == {0, 1}
        assert jobs["bins"].expect(sc.real)["status"].view(np.uint32)[0] == capi.BINS_OUTSIDE and jobs["panel"].expect(sc.real)["status"].view(np.uint32)[0] == tp.OOR


def test_the_expected_bytes_are_what_the_cpu_builds_give(sim_route):
    """every job of the GPU tests on the CPU builds, with the real contents and with the decoy in place: the expectations (HandRes, the
    sentinels, the chains' glue) are right before a GPU sees them, and the decoy is a valid view"""
    sc = Scene(sim_route, 21)
    jobs = dict({k: f(sc) for k, f in ALL_JOBS.items()}, **{k + " (second handle)": f(sc) for k, f in SECOND.items()})
    for state, world in (("decoy", sc.decoy), ("real", sc.real)):
        sc.to_decoy() if state == "decoy" else sc.to_real()
        for name, job in jobs.items():
            rc, got, _ = run_plain(sim_route, job)
            assert rc == 0, (name, state, getattr(sim_route, job.lib)._call("_last_error")(getattr(sim_route, job.lib).h))
            compare(got, job.expect(world), "%s [%s]" % (name, state))


NUMPY_ALONE = '''
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import numpy as np
import synth
from bam_readcount_amd import capi, tensors
from test_dense import computed
lib = %(libs)r
ref = synth.make_ref(np.random.default_rng(11), 1000)
arrs = synth.make_batch(77, ref, 50, read_len=(60, 120), style="indel", n_libs=2, mismatch=0.06)
eng = computed(capi.Library(lib["engine"]), arrs, 20, 980, ref, lib_names=["libA", "libB"], per_lib=True)
indels = capi.Indels(lib["indels"])
got = {"region": tensors.region(eng, capi.Dense(lib["dense"]), want=tensors.KINDS), "indels": tensors.indels(eng, indels)}
got["select"] = sel = tensors.select(eng, capi.Select(lib["select"]), case=["libA"], control=["libB"], min_depth=1, min_alt=1, ctl_max_frac=(1, 2))
got["sites"] = tensors.sites(eng, capi.Panel(lib["panel"]), positions=sel["pos"], want=tensors.KINDS, indels=indels)
got["windows"] = tensors.sites(eng, capi.Panel(lib["panel"]), windows=([100, 300], [110, 301]))
got["runs"] = runs = tensors.runs(eng, capi.Runs(lib["runs"]), cuts=(1, 3), libs=["libB", 0], ref_n=True)
got["bins"] = tensors.bins(eng, capi.Bins(lib["bins"]), width=64, thresholds=(1, 4), hist=8)
got["edges"] = tensors.bins(eng, capi.Bins(lib["bins"]), edges=np.stack([runs["start"], runs["end"]], axis=1).reshape(-1))
got["vet"] = tensors.vet(eng, capi.Vet(lib["vet"]), idx=sel["idx"], alt=sel["why"], libs=["libA"], min_depth=1, min_var_count=1)
n = got["region"]["n"]
assert 900 < n <= 961 and got["indels"]["m"] > 0 and sel["n"] > 0 and runs["n"] > 1 and got["windows"]["n"] == 11
assert got["sites"]["n"] == got["vet"]["n"] == sel["n"] and got["bins"]["n_bins"] == (n + 63) // 64 and got["edges"]["n_bins"] == 2 * runs["n"] - 1
for name, r in got.items():
    for k, a in dict(r, **r.get("indels", {})).items():
        assert isinstance(a, (int, dict, np.ndarray)), (name, k, type(a))
assert not [m for m in sys.modules if m.split(".")[0] == "torch"], "the CPU route imported torch"
print("NUMPY ALONE OK")
'''


def test_the_host_route_needs_numpy_alone(sim_route, tmp_path):
    """tensors' promise that importing the package, and the CPU route, need numpy alone: in a process of its own every entry point of
    bam_readcount_amd.tensors — region, indels, select, sites (a list, windows, indels=), runs, bins (width=, edges=) and vet — on a
    small region computed by the CPU builds, and torch is in sys.modules neither before nor after"""
    import sys
    from conftest import ROOT
    r = sim_route
    libs = dict(engine=r.engine_lib.path, **{k: getattr(r, k).path for k in ("dense", "indels", "select", "panel", "runs", "bins", "vet")})
    script = tmp_path / "numpy_alone.py"
    script.write_text(NUMPY_ALONE % dict(root=ROOT, libs=libs))
    p = subprocess.run([sys.executable, str(script)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0 and b"NUMPY ALONE OK" in p.stdout, p.stderr.decode()[-3000:]


# ------------------------------------------------------------------------------------------------ the GPU: holds

class Hold:
    """A bounded wait queued on torch's current stream: torch.cuda._sleep (a bounded torch workload where torch has none), never a
    kernel that waits for the host.  Calibrated once: `ticks` for `seconds`, measured with two events."""

    def __init__(self, torch, slowest_call):
        self.torch = torch
        self.sleep = getattr(torch.cuda, "_sleep", None)
        self.x = None if self.sleep else torch.ones(1024, 1024, device="cuda")
        self.target = min(HOLD_CAP, max(20.0 * slowest_call, HOLD_FLOOR))
        trial = 1_000_000 if self.sleep else 50
        self._queue(trial); torch.cuda.synchronize()                    # (loads the kernel)
        per = self._measure(trial) / trial
        assert per > 0, "the trial hold took no measurable time"
        self.ticks = max(int(self.target / per), 1)
        self.seconds = self._measure(self.ticks)
        if not 0.8 * self.target <= self.seconds <= min(1.2 * self.target, HOLD_CAP):       # (the trial was too short to scale from: once more)
            self.ticks = max(int(self.ticks * self.target / self.seconds), 1)
            self.seconds = self._measure(self.ticks)
        assert 0.5 * self.target <= self.seconds <= 1.2 * HOLD_CAP, "the hold cannot be calibrated: %d ticks took %.4f s, wanted %.4f s" % (self.ticks, self.seconds, self.target)

    def _queue(self, ticks):
        if self.sleep:
            self.sleep(int(ticks))
        else:
            for _ in range(int(ticks)):
                self.torch.mm(self.x, self.x)

    def _measure(self, ticks):
        a, b = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
        a.record(); self._queue(ticks); b.record(); b.synchronize()
        return a.elapsed_time(b) * 1e-3

    def queue(self, share=1.0):
        self._queue(max(int(self.ticks * share), 1))


def streams_beside_the_default(torch, hold, want=4, tries=16):
    """Streams on which a hold does not keep the default stream back.  The runtime spreads its streams over a few hardware queues,
    and a stream that shares the default stream's queue runs in order with it: there a launch that strayed to stream 0 would still
    come behind the hold and the late inputs, and the test could not see it.  Probed once: a short hold on the candidate, a small
    torch op and an event on the default stream — the stream qualifies when that event fires while the hold is still running.  (A
    bounded poll: it ends when either event has fired.)"""
    found = []
    x = torch.zeros(8, device="cuda")
    for _ in range(tries):
        s = torch.cuda.Stream()
        e_hold, e_null = torch.cuda.Event(), torch.cuda.Event()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            hold.queue(0.4)
            e_hold.record(s)
        x.add_(1)
        e_null.record()
        while not e_hold.query() and not e_null.query():
            pass
        held_still = not e_hold.query()
        if held_still and e_null.query():
            found.append(s)
        torch.cuda.synchronize()
        if len(found) == want:
            break
    return found


class Gpu:
    def stream(self):
        """the next of the probed streams, in turn"""
        self.turn = getattr(self, "turn", -1) + 1
        return self.streams[self.turn % len(self.streams)]


@pytest.fixture(scope="module")
def gpu():
    """The hip route, two scenes, every job run once on the default stream (code objects and torch's kernels loaded, the values
    checked there too, the six calls' warm host times and byte counts taken), and the hold sized against them."""
    g = Gpu()
    g.route = route = _route("hip")
    g.torch = torch = route.torch
    g.scenes = [Scene(route, 21), Scene(route, 22)]
    g.call_s, g.bytes = {}, {}
    for sc in g.scenes:
        for name, f in dict(ALL_JOBS, **{k + " (second handle)": f for k, f in SECOND.items()}).items():
            job = f(sc)
            rc, got, dt = run_plain(route, job)
            assert rc == 0, (name, getattr(route, job.lib)._call("_last_error")(getattr(route, job.lib).h))
            compare(got, job.expect(sc.real), name + " [default stream]")
            if name in SINGLE and sc is g.scenes[0]:                   # (the byte counts depend on the view: the timing test uses this one)
                torch.cuda.synchronize()
                _, _, dt = run_plain(route, job)                        # warm
                g.call_s[name] = min(dt, g.call_s.get(name, dt))
                t = getattr(route, job.lib).last_timing()
                g.bytes[name] = (t["bytes_read"], t["bytes_written"])
    torch.cuda.synchronize()
    g.hold = Hold(torch, max(g.call_s.values()))
    g.streams = streams_beside_the_default(torch, g.hold)
    assert len(g.streams) >= 2, "INCONCLUSIVE: fewer than two streams run beside the default stream on this machine: a launch on stream 0 could not be told from one on the caller's"
    print("\nhold: %d ticks of %s = %.4f s (wanted %.4f s); warm host-side call times: %s" %
          (g.hold.ticks, "torch.cuda._sleep" if g.hold.sleep else "torch.mm", g.hold.seconds, g.hold.target,
           ", ".join("%s %.1f us" % (k, 1e6 * v) for k, v in g.call_s.items())))
    return g


def held(g, lanes):
    """lanes: [(scene, job, share of the hold)], one stream each (torch.cuda.Stream()s, probed by the `gpu` fixture), all queued before any is waited for.  Returns per lane the
    host's seconds from the call to the end of the stream's synchronisation.  Nothing here touches the default stream between the
    synchronisation that settles the decoy and the streams' own."""
    torch, route = g.torch, g.route
    for sc, _, _ in lanes:
        sc.to_decoy()
    sizes = [job.sizes(route) for _, job, _ in lanes]
    bufs = [{k: torch.zeros(max(n, 8), dtype=torch.uint8, device="cuda") for k, n in s.items()} for s in sizes]
    outs = [{k: torch.zeros_like(b) for k, b in buf.items()} for buf in bufs]
    streams = [g.stream() for _ in lanes]
    e_in = [torch.cuda.Event() for _ in lanes]
    torch.cuda.synchronize()
    rcs, t_call = [], []
    for (sc, job, share), s, e, buf, out in zip(lanes, streams, e_in, bufs, outs):
        with torch.cuda.stream(s):
            g.hold.queue(share)
            sc.restore()
            for b in buf.values():
                b.fill_(SENT8)
            e.record(s)
            t_call.append(time.perf_counter())
            rcs.append(job.enqueue(route, buf, s.cuda_stream))
            for k in buf:
                out[k].copy_(buf[k], non_blocking=True)
    pending = [not e.query() for e in e_in]
    wall = []
    for s, t0 in zip(streams, t_call):
        s.synchronize()
        wall.append(time.perf_counter() - t0)
    for (sc, job, _), rc in zip(lanes, rcs):
        assert rc == 0, (job.name, getattr(route, job.lib)._call("_last_error")(getattr(route, job.lib).h))
    assert all(pending), ("INCONCLUSIVE: when the call returned, the inputs' event on its stream had fired — the call waited for its stream, or the hold "
                          "of %.1f ms did not outlast the host's queueing: nothing is proved about order (%r)" % (1e3 * g.hold.seconds, pending))
    for (sc, job, _), s, out in zip(lanes, sizes, outs):
        compare({k: b.cpu().numpy()[:s[k]] for k, b in out.items()}, job.expect(sc.real), job.name + " [held stream]")
    return wall


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SINGLE) + list(EARLY))
def test_each_entry_point_on_a_held_stream(gpu, name):
    """the six calls with every output, and their early-return forms (n == 0: the clears; counts alone): the call returns while the
    hold runs, and what the stream's later copies see is the reference of the real, late contents"""
    held(gpu, [(gpu.scenes[0], ALL_JOBS[name](gpu.scenes[0]), 1.0)])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CHAINS))
def test_chains_on_one_held_stream(gpu, name):
    """select -> panel, runs -> edges -> bins, runs -> select's list: late inputs, one stream, no host synchronisation between the links"""
    held(gpu, [(gpu.scenes[0], CHAINS[name](gpu.scenes[0]), 1.0)])


@pytest.mark.gpu
@pytest.mark.parametrize("first_released", [0, 1])
@pytest.mark.parametrize("lib", list(SECOND))
def test_two_streams_two_handles(gpu, lib, first_released):
    """two handles of one library, two views, two parameter sets, two workspaces, two held streams released in either order: each
    result is its own reference"""
    a, b = gpu.scenes
    shares = (0.5, 1.0) if first_released == 0 else (1.0, 0.5)
    held(gpu, [(a, SINGLE[lib](a), shares[0]), (b, SECOND[lib](b), shares[1])])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SINGLE))
def test_last_timing_after_a_call_on_a_held_stream(gpu, name):
    """the two events lie on the caller's stream, around the launches: kernel_s is positive, below the host's time from the call to the
    end of the stream's synchronisation and below the hold in front of the call; the byte counts are the default stream's"""
    job = SINGLE[name](gpu.scenes[0])
    wall, = held(gpu, [(gpu.scenes[0], job, 1.0)])
    t = getattr(gpu.route, job.lib).last_timing()
    print("%s: kernel_s %.6f, call to synchronised %.6f, hold %.6f" % (name, t["kernel_s"], wall, gpu.hold.seconds))
    assert 0 < t["kernel_s"] < wall, (name, t, wall)
    assert t["kernel_s"] < gpu.hold.seconds, "%s: kernel_s %.6f includes the hold of %.6f s: an event lies on another stream" % (name, t["kernel_s"], gpu.hold.seconds)
    assert (t["bytes_read"], t["bytes_written"]) == gpu.bytes[name], name


# ------------------------------------------------------------------------------------------------ the GPU: tensors.* under torch.cuda.stream(s)

@pytest.fixture(scope="module")
def low_region(oracle_lib):
    """test_select's synthetic low-depth region of two libraries and the oracle's result of it"""
    rng = np.random.default_rng(11)
    ref = synth.make_ref(rng, 3000, weird=0.01)
    arrs = synth.make_batch(77, ref, 260, read_len=(60, 120), style="indel", n_libs=2, mismatch=0.06)
    res, _ = td.oracle_result(oracle_lib, arrs, 50, 2950, ref, **ts.PER_LIB)
    return ref, arrs, res


@pytest.mark.gpu
def test_tensors_functions_under_a_held_stream(gpu, low_region):
    """tensors.region / indels / sites / select / bins / runs / vet on an engine-computed region inside `with torch.cuda.stream(s)`,
    behind a hold, with a torch op of the caller's queued behind each: the results are the references.  region, bins(width=) and vet
    on device lists (a select result from outside the held window) must return while the hold runs; the others read a count (or
    upload a host list) and may wait — see the module's text."""
    from bam_readcount_amd import tensors
    torch, route = gpu.torch, gpu.route
    ref, arrs, res = low_region
    eng = td.computed(route.engine_lib, arrs, 50, 2950, ref, **ts.PER_LIB)
    dense, D = ts.Dense.of(res), tb.Dense.of(res)
    P_, p0 = res.n_pos, res.pos0
    p = ts.TWOLIB_PARAMS[2][1]
    pos = (p0 + np.array([0, 1, 63, 64, 65, 200, 200, 1000, P_ - 1])).tolist()
    cuts = (2, 5)
    VD = tv.Dense.of(res)
    vidx, vwhy = tv.select_list(VD, 1)
    sel = tensors.select(eng, route.select, indel=False, min_depth=0, min_alt=1)          # vet's device lists: made outside the held window
    assert sel["n"] == len(vidx) > 20 and sel["idx"].is_cuda and sel["why"].is_cuda
    calls = {"region": lambda: tensors.region(eng, route.dense, want=tensors.KINDS),
             "bins": lambda: tensors.bins(eng, route.bins, width=64, thresholds=(1, 4), hist=8),
             "indels": lambda: tensors.indels(eng, route.indels),
             "sites": lambda: tensors.sites(eng, route.panel, positions=pos, want=tensors.KINDS),
             "select": lambda: tensors.select(eng, route.select, role=[1, 2], min_depth=p["min_depth"], min_alt=p["min_alt"], min_frac=p["frac"], ctl_max_frac=p["ctl_frac"]),
             "runs": lambda: tensors.runs(eng, route.runs, cuts=cuts, combine="max", ref_n=True),
             "vet": lambda: tensors.vet(eng, route.vet, idx=sel["idx"], alt=sel["why"], **tv.EASY_LOW)}
    first = {"region": "depth", "bins": "sums", "indels": "pos", "sites": "depth", "select": "idx", "runs": "k0", "vet": "keep"}
    for f in calls.values():                                             # (torch's own kernels of these paths, loaded outside the held window)
        f()
    torch.cuda.synchronize()
    got, seen = {}, {}
    for name, f in calls.items():
        s = gpu.stream()
        e = torch.cuda.Event()
        with torch.cuda.stream(s):
            gpu.hold.queue()
            e.record(s)
            got[name] = r = f()
            pending = not e.query()
            seen[name] = r[first[name]].view(torch.int32).clone()        # the caller's own op, queued behind the call
        if name in ("region", "bins", "vet"):
            assert pending, "INCONCLUSIVE or a wait: tensors.%s returned after the hold of %.1f ms on its stream had run out" % (name, 1e3 * gpu.hold.seconds)
        s.synchronize()
        assert np.array_equal(seen[name].cpu().numpy(), r[first[name]].view(torch.int32).cpu().numpy()), name
    want = td.want_planes(res, 0, P_)
    for k in tensors.KINDS:
        assert np.array_equal(tp.host_words(route, got["region"][k]).reshape(want[k].shape), want[k]), k
    tb.check_bins(route, got["bins"], D, 0, P_, 64, None, (1, 4), 8, "bins on a stream")
    table = ti.table_of(res.indels)
    assert got["indels"]["m"] == len(res.indels) > 0
    for k in tensors.INDEL_KINDS:
        a = got["indels"][k].cpu().numpy()
        assert np.array_equal(a.view(np.uint8 if k == "alleles" else np.uint32).reshape(table[k].shape), table[k]), k
    tp.check_sites(route, got["sites"], res, pos, np.arange(len(pos)), "sites on a stream")
    ts.check_select(route, got["select"], dense, [1, 2], p, "select on a stream")
    tr.check_runs(route, got["runs"], dense, 0, P_, cuts, "runs on a stream", combine=tr.MAX, ref_n=True)
    tv.check_vet(route, got["vet"], VD, vidx, vwhy, "vet on a stream", **tv.EASY_LOW)
    eng.close()
