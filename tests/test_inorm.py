"""Device-side indel normalisation (include/brc_inorm.h): brc_inorm_table and bam_readcount_amd.tensors.normalize_indels against a
PLAIN-PYTHON restatement of the header's definition — lists, bytes, the text rewritten step by step, numpy.float32 additions one at a
time — every output equal as bit patterns, no tolerance, no cell left out.

Every body runs twice (the `route` fixture): [sim] = tests/sim_inorm/libbrc_inorm_sim.so, host memory, in the CPU suite; [hip] = the
product's library on the GPU (gpu-marked), view, table, scratch and destinations in device memory allocated through torch.
Destinations are filled with 0xA5 first and are PAD elements wider than the caps: everything behind the contract's sizes and every
destination that was not asked for must keep it.  The scratch has exactly brc_inorm_workspace bytes.

Beside the reference, two properties that do not restate the rule are asserted on every case's REFERENCE-side result first (`props`):
the case-folded haplotype of every judged record is unchanged, and a second normalisation of the output shifts nothing and merges
nothing (a case in which a walk stopped at max_shift is exempt from the second: the limit is what stopped it).

Sizes that matter to the kernels (brc_inorm.hip): a wave is 64 consecutive records, a workgroup 256, a scan's second round of partials
begins behind 65 536 elements."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from bam_readcount_amd import capi
import abi_side as side
from route import Route, SENT, SENT8
import test_dense as td
import test_indels as ti
import test_ivet as tiv
import test_select as ts
import test_vet as tv

LIBS = tiv.LIBS + ("inorm",)
PAD = 3
F32 = np.float32
NJ, LIMIT, EDGE = capi.INORM_NOT_JUDGED, capi.INORM_LIMIT, capi.INORM_EDGE
PER_IN = ("npos", "shift", "flags", "group")
PER_OUT = ("pos", "lib", "len", "rep_read", "rep_qpos", "members")
PLANES = (("istat", 9), ("fstat", 4), ("metrics", 13))
EVERY = ("counts", "status") + PER_IN + PER_OUT + ("istat", "fstat", "metrics", "allele_off", "alleles")
CASE, CTL = capi.ROLE_CASE, capi.ROLE_CONTROL
Tab, sums = tiv.Tab, tiv.sums


@pytest.fixture(scope="module", params=["sim", pytest.param("hip", marks=pytest.mark.gpu)])
def route(request):
    return Route(request.param, LIBS, engine=True)


@pytest.fixture(scope="module")
def sim_route():
    return Route("sim", LIBS, engine=True)


# ------------------------------------------------------------------------------------------------ the view

class View:
    """the plain-data form of the brc_device_indels view the library reads: the reference slice, pos0, n_pos, n_lib"""

    def __init__(self, ref, pos0=0, n_pos=None, n_lib=1, ref_lo=None, ref_len=None):
        self.ref = None if ref is None else bytes(ref)
        self.pos0, self.n_lib = pos0, n_lib
        self.ref_lo = pos0 if ref_lo is None else ref_lo
        self.ref_hi = self.ref_lo + (len(self.ref) if self.ref is not None else 0)
        self.ref_len = self.ref_hi if ref_len is None else ref_len
        self.n_pos = (len(self.ref) if self.ref is not None else 0) if n_pos is None else n_pos

    @classmethod
    def of_engine(cls, d, ref):
        """the view an engine hands out, with the slice of the whole-contig `ref` it uploaded"""
        ref = bytes(ref)
        return cls(ref[d.ref_lo:d.ref_hi], int(d.pos0), int(d.n_pos), int(d.n_lib), int(d.ref_lo), int(d.ref_len))

    def make(self, route):
        """-> (capi.DeviceIndels, keep-alive): the slice has exactly its own bytes; no record array is given (the library reads none)"""
        keep = route.put(np.frombuffer(self.ref, np.uint8)) if self.ref is not None else None
        return capi.DeviceIndels(route.mem, 0, self.n_lib, self.pos0, self.n_pos, None, 0, None, None, None, 0, route.ptr(keep) if keep is not None else None,
                                 self.ref_lo, self.ref_hi, self.ref_len), keep

    def R(self, p):
        if self.ref is None or not self.ref_lo <= p < self.ref_hi or p >= self.ref_len or p < 0:
            return None
        c = self.ref[p - self.ref_lo]
        return c if c else None


def base(c):
    if c is None:
        return None
    if 97 <= c <= 122:
        c -= 32
    return c if c in b"ACGT" else None


def match(a, b):
    return base(a) is not None and base(a) == base(b)


# ------------------------------------------------------------------------------------------------ the reference, in plain Python

def norm_reference(V, T, k0=0, n=None, max_shift=1024, rep=None):
    """The header's definition, operation by operation.  -> dict(npos, shift, flags, group: lists over the input records; status; merged:
    list of dict(pos, lib, len, text (sign first), i [9 ints], f [4 numpy.float32], rep_read, rep_qpos, members, of: input indices))"""
    n = V.n_pos - k0 if n is None else n
    first = V.pos0 + k0
    floor = max(first, V.ref_lo)
    text = T.texts()
    npos, shift, flags, final = [], [], [], []
    for r in range(T.m):
        p, l, ln = int(T.pos[r]), int(T.lib[r]), int(T.len[r])
        L = abs(ln)
        judged = ln != 0 and first <= p < first + n and 0 <= l < V.n_lib and len(text[r]) == L + 1 and text[r][:1] == (b"+" if ln > 0 else b"-")
        if not judged:
            npos.append(p); shift.append(0); flags.append(NJ); final.append(None)
            continue
        t, s, fl = text[r][1:], 0, 0
        while True:
            if not match(V.R(p), t[L - 1]):
                break
            if s == max_shift:
                fl = LIMIT
                break
            if p - 1 < floor:
                fl = EDGE
                break
            c = t[L - 1] if ln > 0 else V.R(p)
            t = bytes([c]) + t[:L - 1]
            p -= 1; s += 1
        npos.append(p); shift.append(s); flags.append(fl); final.append(text[r][:1] + t)
    classes = {}
    for r in range(T.m):
        if final[r] is not None:
            classes.setdefault((npos[r], int(T.lib[r]), final[r], int(T.len[r])), []).append(r)       # (ascending input index)
    merged, group = [], [-1] * T.m
    for key in sorted(classes):                                   # (pos, lib, text bytewise with its sign; len follows from the text)
        of = classes[key]
        i = [0] * 9
        f = [F32(T.fstat[c, of[0]]) for c in range(4)]
        for x, r in enumerate(of):
            for c in range(9):
                i[c] = (i[c] + int(T.istat[c, r])) % 2 ** 32
            if x:
                with np.errstate(over="ignore", invalid="ignore"):
                    for c in range(4):
                        f[c] = F32(f[c] + F32(T.fstat[c, r]))     # one rounding per addition, in input order
            group[r] = len(merged)
        merged.append(dict(pos=key[0], lib=key[1], len=key[3], text=key[2], i=i, f=f, members=len(of), of=of,
                           rep_read=int(rep[0][of[0]]) if rep else 0, rep_qpos=int(rep[1][of[0]]) if rep else 0))
    status = 0
    for fl in flags:
        status |= fl                                              # (NOT_JUDGED / LIMIT / EDGE are TABLE_BAD / ANY_LIMIT / ANY_EDGE)
    if T.m == 0 or n == 0:
        status = 0
    return dict(npos=npos, shift=shift, flags=flags, group=group, status=status, merged=merged, k0=k0, n=n)


def merged_tab(W):
    """the reference's merged table as a Tab (the input of a second normalisation, and of test_ivet.reference)"""
    M = W["merged"]
    return Tab.of([(g["pos"], g["lib"], g["text"], (g["i"], [float(x) for x in g["f"]]), g["len"]) for g in M])


def haplotype(V, p, ln, text, lo, hi):
    """the stretch [lo, hi) of the reference slice with the allele applied behind position p (lo <= p + 1, p + 1 + |ln| <= hi), case-folded"""
    a, lo, hi = p + 1 - V.ref_lo, lo - V.ref_lo, hi - V.ref_lo
    if ln > 0:
        return (V.ref[lo:a] + text + V.ref[a:hi]).upper()
    return (V.ref[lo:a] + V.ref[a - ln:hi]).upper()


def props(V, T, W, max_shift):
    """the two properties that do not restate the rule, on the reference's own result"""
    text = T.texts()
    for r in range(T.m):
        if W["group"][r] < 0 or W["shift"][r] == 0:
            continue
        g = W["merged"][W["group"][r]]
        ln = int(T.len[r])
        lo, hi = g["pos"], min(int(T.pos[r]) + 1 + abs(ln), V.ref_hi)        # (the stretch both placements touch)
        assert haplotype(V, int(T.pos[r]), ln, text[r][1:], lo, hi) == haplotype(V, g["pos"], ln, g["text"][1:], lo, hi), ("haplotype", r)
        assert g["pos"] == int(T.pos[r]) - W["shift"][r] and len(g["text"]) == len(text[r])
    if not W["status"] & LIMIT and W["n"]:
        W2 = norm_reference(V, merged_tab(W), W["k0"], W["n"], max_shift)
        assert not any(W2["shift"]) and len(W2["merged"]) == len(W["merged"]) and not W2["status"] & NJ, "a second normalisation does more"


def expected(W, T, cap, acap, want=EVERY):
    """every destination as the contract leaves it: {name: uint32 words, or uint8 bytes for alleles}, PAD elements wider than its size,
    SENT where nothing may be written"""
    M = W["merged"]
    m, mm = T.m, len(M)
    empty = m == 0 or W["n"] == 0
    e = {"counts": np.full(2 + PAD, SENT, np.uint32), "status": np.full(1 + PAD, SENT, np.uint32)}
    e["counts"][:2] = [mm, sum(len(g["text"]) for g in M)]
    e["status"][0] = W["status"]
    for k in PER_IN:
        e[k] = np.full(m + PAD, SENT, np.uint32)
        if not empty:
            e[k][:m] = np.array(W[k], np.int64).astype(np.uint32)
    w = min(mm, cap)
    for k in PER_OUT:
        e[k] = np.full(cap + PAD, SENT, np.uint32)
        e[k][:w] = np.array([g[k] for g in M[:w]], np.int64).astype(np.uint32)
    ist = np.array([g["i"] for g in M], np.uint32).reshape(mm, 9).T
    fst = np.array([g["f"] for g in M], np.float32).reshape(mm, 4).T
    for k, a in (("istat", ist), ("fstat", fst.view(np.uint32)), ("metrics", ti.metrics_of(ist, fst).view(np.uint32))):
        e[k] = np.full(a.shape[0] * cap + PAD, SENT, np.uint32)
        for c in range(a.shape[0]):
            e[k][c * cap:c * cap + w] = a[c, :w]
    off = np.concatenate([[0], np.cumsum([len(g["text"]) for g in M])]).astype(np.int64)
    e["allele_off"] = np.full(cap + 1 + PAD, SENT, np.uint32)
    e["allele_off"][:w + 1] = off[:w + 1]
    e["alleles"] = np.full(acap + PAD, SENT8, np.uint8)
    for g in range(w):
        if off[g + 1] <= acap:
            e["alleles"][off[g]:off[g + 1]] = np.frombuffer(M[g]["text"], np.uint8)
    for k in e:
        if k not in want:
            e[k][:] = SENT8 if k == "alleles" else SENT
    return e


# ------------------------------------------------------------------------------------------------ calling the library

def call(route, V, T, k0=0, n=None, max_shift=1024, cap=0, acap=0, want=EVERY, rep=None, stride=None, handle=True, view=True, params=True, source=True,
         ws=True, wsb=None, reserved=(0, 0, 0), dview=None, sfields=None, ws_zero=False):
    """brc_inorm_table into sentinel-filled buffers PAD elements wider than the caps and a scratch of exactly brc_inorm_workspace bytes;
    view, table and destinations in the route's memory.  -> (rc, {name: words})"""
    n = V.n_pos - k0 if n is None else n
    m = T.m
    stride = m if stride is None else stride
    ist = np.full((9, max(stride, m)), 0xDEADBEEF, np.uint32); ist[:, :m] = T.istat
    fst = np.full((4, max(stride, m)), np.nan, np.float32); fst[:, :m] = T.fstat
    src = [T.pos.astype(np.int32), T.lib.astype(np.int32), T.len.astype(np.int32)] + ([np.asarray(rep[0], np.uint32), np.asarray(rep[1], np.int32)] if rep else []) + \
        [ist, fst, T.off, T.alleles]
    keep = [route.put(x) for x in src]
    p = [route.ptr(b) for b in keep]
    if not rep:
        p[3:3] = [None, None]
    S = capi.INormSource(m, stride, *p, T.alleles.size)
    for k, x in (sfields or {}).items():
        setattr(S, k, x)
    par = capi.INormParams(max_shift, (C.c_uint32 * 3)(*reserved))
    d, dkeep = V.make(route)
    if dview is not None:
        d = dview(d)
    sizes = {"counts": 2, "status": 1, "allele_off": max(cap, 0) + 1}
    sizes.update({k: m for k in PER_IN}); sizes.update({k: max(cap, 0) for k in PER_OUT}); sizes.update({k: f * max(cap, 0) for k, f in PLANES})
    buf = {k: route.sentinel_words(sz + PAD) for k, sz in sizes.items()}
    buf["alleles"] = route.sentinel_words((max(acap, 0) + PAD + 3) // 4 + 1)
    need = route.inorm.workspace(n, m)
    assert need % 4 == 0
    wsb = need if wsb is None else wsb
    bw = route.sentinel_words(max(wsb, 0) // 4)
    if ws_zero:                                             # (a caller's scratch may hold anything: zeros instead of 0xA5)
        bw[:] = 0
    a = {k: (route.ptr(b) if k in want else None) for k, b in buf.items()}
    rc = route.inorm.lib.brc_inorm_table(route.inorm.h if handle else None, C.byref(d) if view else None, C.byref(par) if params else None,
                                         C.byref(S) if source else None, k0, n, route.ptr(bw) if ws else None, max(wsb, 0), a["counts"], a["npos"], a["shift"],
                                         a["flags"], a["group"], cap, acap, a["pos"], a["lib"], a["len"], a["rep_read"], a["rep_qpos"], a["members"], a["istat"],
                                         a["fstat"], a["metrics"], a["allele_off"], a["alleles"], a["status"], None)
    got = {k: route.words(b)[:sizes[k] + PAD].copy() for k, b in buf.items() if k != "alleles"}
    got["alleles"] = route.words(buf["alleles"]).view(np.uint8)[:max(acap, 0) + PAD].copy()
    del keep, dkeep
    return rc, got


def untouched(got):
    return all((g == (SENT8 if k == "alleles" else SENT)).all() for k, g in got.items())


def check(route, V, T, k0=0, n=None, max_shift=1024, what="", want=EVERY, short=(0, 0), rep=None, stride=None, W=None, ws_zero=False):
    """one call against the reference, bit for bit, sentinels included; the properties first.  short: how far cap / alleles_cap stay
    below the counts.  Returns the reference's result."""
    if W is None:
        W = norm_reference(V, T, k0, n, max_shift, rep)
        props(V, T, W, max_shift)
    mm, nb = len(W["merged"]), sum(len(g["text"]) for g in W["merged"])
    cap, acap = max(mm + PAD - short[0] * (PAD + 1), 0), max(nb + PAD - short[1] * (PAD + 1), 0)
    rc, got = call(route, V, T, k0, n, max_shift, cap, acap, want, rep, stride, ws_zero=ws_zero)
    assert rc == 0, (what, route.inorm.lib.brc_inorm_last_error(route.inorm.h))
    e = expected(W, T, cap, acap, want)
    for k in e:
        assert np.array_equal(got[k], e[k]), (what, k, np.argwhere(got[k] != e[k])[:4].ravel().tolist(), got[k][:8], e[k][:8])
    return W


# ------------------------------------------------------------------------------------------------ 1. the walk

UNIT = {1: b"A", 2: b"AC", 3: b"ACG", 7: b"ACGTTGA"}


def walk_case(lower=False):
    """One reference with a stretch per (kind, L, free shift): an insertion of L bases behind a stretch whose last s characters continue
    its text cyclically, and a deletion of the last L characters of a stretch of period L and length s + L — both behind a character
    that stops the walk.  -> (View, Tab, {record: its free shift})"""
    ref, recs, free = bytearray(b"GNNNN"), [], {}
    for L, u in UNIT.items():
        for s in (0, 1, L - 1, L, L + 1, 3 * L + 1):
            seg = (u * 8)[len(u) * 8 - s:]
            ref += seg
            free[len(recs)] = s
            recs.append((len(ref) - 1, 0, b"+" + u, sums(3 + len(recs))))
            ref += b"NN"
            per = (u * 8)[:s + L]
            ref += per
            free[len(recs)] = s
            recs.append((len(ref) - 1 - L, 0, b"-" + per[s:], sums(3 + len(recs))))
            ref += b"NTN"
    if lower:
        ref = bytearray(bytes(ref).lower().replace(b"n", b"N"))
        recs = [(p, l, (t[:1] + t[1:].lower()) if t[:1] == b"-" else t, s) for p, l, t, s in recs]
    return View(ref, pos0=0), Tab.of(recs), free


def test_shifts_of_every_length_for_both_kinds(route):
    """shifts of 0, 1, L - 1, L, L + 1 and 3L + 1 for L = 1, 2, 3, 7: an insertion's text rotates, a deletion's walk crosses from its own
    text into the reference at s = L"""
    V, T, free = walk_case()
    W = check(route, V, T, what="walk")
    assert W["shift"] == [free[r] for r in range(T.m)] and not any(W["flags"]) and W["status"] == 0
    assert {(abs(int(T.len[r])), W["shift"][r] - abs(int(T.len[r]))) for r in range(T.m) if T.len[r] < 0} >= {(L, x) for L in (2, 3, 7) for x in (-1, 0, 1)}


def test_a_soft_masked_repeat_keeps_the_references_raw_case(route):
    V, T, free = walk_case(lower=True)
    W = check(route, V, T, what="soft-masked")
    assert W["shift"] == [free[r] for r in range(T.m)]
    dels = [g for g in W["merged"] if g["len"] < 0 and len(g["of"]) == 1 and W["shift"][g["of"][0]] > 0]
    assert dels and all(g["text"][1:].islower() and g["text"][1:] == V.ref[g["pos"] + 1:g["pos"] + 1 - g["len"]] for g in dels)
    ins = [g for g in W["merged"] if g["len"] > 0]
    assert all(g["text"][1:].isupper() for g in ins)          # (an insertion's bytes are its own, rotated)


def test_characters_that_stop_a_walk(route):
    """N, n, R and NUL in the reference; '=' and N in inserted text; a lower-case reference under an upper-case text matches"""
    ref = b"G" + b"AANAA" + b"G" + b"AAnAA" + b"G" + b"AARAA" + b"G" + b"AA\0AA" + b"G" + b"aaaa" + b"G" + b"A=A=A=" + b"G" + b"ANANAN" + b"GNNNN" + b"GG"
    V = View(ref)
    recs = [(5, 0, "+A", sums(4)), (11, 0, "+A", sums(5)), (17, 0, "+A", sums(6)), (23, 0, "+A", sums(7)), (28, 0, "+A", sums(8)),
            (29 + 5, 0, "+A=", sums(9)), (36 + 5, 0, "+AN", sums(10)), (36 + 5, 0, "+NA", sums(11)), (len(ref) - 3, 0, "+N", sums(12)),
            (len(ref) - 1, 0, "+g", sums(13))]
    T = Tab.of(recs)
    W = check(route, V, T, what="stoppers")
    assert W["shift"][:5] == [2, 2, 2, 2, 4]
    assert W["shift"][5:9] == [0, 0, 1, 0] and W["shift"][9] == 2      # "+NA" steps once over its A and stops at its N; "+g" folds


def free_shift_view():
    ref = b"GT" + b"A" * 10 + b"CGT"
    return View(ref, pos0=100), ref


def test_max_shift_around_a_records_free_shift(route):
    V, ref = free_shift_view()
    T = Tab.of([(111, 0, "+A", sums(5)), (111, 0, "-C", sums(6))])         # the insertion is free to go 10 steps, the deletion none
    for ms, want_s, want_f in ((9, 9, LIMIT), (10, 10, 0), (11, 10, 0), (0, 0, LIMIT), (capi.INORM_MAX_SHIFT, 10, 0)):
        W = check(route, V, T, max_shift=ms, what="max_shift %d" % ms)
        assert (W["shift"], W["flags"]) == ([want_s, 0], [want_f, 0]) and W["status"] == want_f, ms


def test_the_floor(route):
    """`first` above ref_lo and below it, a record at the floor itself, a view without a reference: EDGE only when a step was possible"""
    ref = b"A" * 12 + b"CGT"
    rec = [(8, 0, "+A", sums(5)), (8, 0, "+C", sums(6)), (11, 0, "+A", sums(7))]
    # the window begins inside the slice: the floor is `first`
    V = View(ref, pos0=0)
    W = check(route, V, Tab.of(rec), k0=5, n=10, what="first above ref_lo")
    assert (W["npos"], W["flags"], W["status"]) == ([5, 8, 5], [EDGE, 0, EDGE], EDGE)
    W = check(route, V, Tab.of([(5, 0, "+A", sums(5)), (5, 0, "+C", sums(6))]), k0=5, n=10, what="a record at the floor")
    assert (W["shift"], W["flags"]) == ([0, 0], [EDGE, 0])
    # the slice begins inside the window: the floor is ref_lo, and a record left of it has no reference character
    V = View(ref[4:], pos0=0, n_pos=15, ref_lo=4)
    W = check(route, V, Tab.of([(2, 0, "+A", sums(4))] + rec), what="first below ref_lo")
    assert (W["npos"], W["flags"]) == ([2, 4, 8, 4], [0, EDGE, 0, EDGE])
    # the slice ends at ref_len, whatever lies behind it
    V = View(ref, pos0=0, ref_len=10)
    W = check(route, V, Tab.of(rec), what="ref_len inside the slice")
    assert W["shift"] == [8, 0, 0]
    V = View(None, pos0=0, n_pos=15)
    W = check(route, V, Tab.of(rec), what="no reference")
    assert W["shift"] == [0, 0, 0] and W["status"] == 0 and len(W["merged"]) == 3


# ------------------------------------------------------------------------------------------------ 2. records that are not judged

def test_records_that_are_not_judged(route):
    ref = b"G" + b"A" * 8 + b"CGTTTTG"
    V = View(ref, pos0=50, n_lib=2)
    s = sums(6)
    good = [(55, 0, "+A", s), (58, 1, "+A", s), (63, 1, "-T", s)]
    bad = [(52, 0, "", s, 0), (49, 0, "+A", s), (50 + len(ref), 0, "+A", s), (56, -1, "+A", s), (56, 2, "+A", s), (57, 0, "+A", s, 2), (57, 0, "+AAA", s, 2),
           (57, 0, "-A", s, 1), (57, 0, "+A", s, -1)]
    for i, b in enumerate(bad):
        recs = sorted(good + [b], key=lambda r: r[0])
        T = Tab.of(recs)
        W = check(route, V, T, what="not judged %d" % i)
        x = recs.index(b)
        assert W["flags"][x] == NJ and W["group"][x] == -1 and W["npos"][x] == b[0] and W["status"] & NJ and len(W["merged"]) == 3
        assert sorted(g for g in W["group"] if g >= 0) == [0, 1, 2]
    # a window that leaves records out
    W = check(route, V, Tab.of(good), k0=6, n=4, what="a window inside the table")
    assert W["flags"] == [NJ, EDGE, NJ]
    # offsets above alleles_len and descending: no read leaves `alleles`
    T = Tab.of(good + [(64, 0, "-G", s), (65, 1, "+GG", s)])
    for x, val in ((1, T.alleles.size + 1000), (2, 0xFFFFFFFF), (3, 0), (5, 0xFFFFFFF0), (5, 1)):
        B = Tab(T.pos, T.lib, T.len, T.istat, T.fstat, T.off.copy(), T.alleles)
        B.off[x] = val
        W = check(route, V, B, what="offsets %d" % x)
        assert (W["status"] & NJ) == (0 if (x, val) == (5, 0xFFFFFFF0) else NJ)      # (the last offset clamps to alleles_len: the true one)


def test_records_of_libraries_that_do_not_exist(route):
    """table records whose library is n_lib, n_lib + 1 or -1 beside a valid record of the same position and allele, with 2 libraries
    and with 254 (the most a view holds): not judged, group -1, BRC_INORM_TABLE_BAD in the status word, and they join no merged record"""
    ref = b"G" + b"A" * 8 + b"CGTTTTG"
    s = sums(6)
    for L in (2, 254):
        V = View(ref, pos0=50, n_lib=L)
        recs = [(55, L - 1, "+A", s), (55, L, "+A", s), (55, L + 1, "+A", s), (55, -1, "+A", s), (58, L - 1, "+A", s), (58, L, "+A", s), (63, L, "-T", s),
                (63, 0, "-T", s)]
        W = check(route, V, Tab.of(recs), what="bad libraries of %d" % L)
        assert W["flags"] == [0, NJ, NJ, NJ, 0, NJ, NJ, 0] and W["group"] == [0, -1, -1, -1, 0, -1, -1, 1] and W["status"] == capi.INORM_TABLE_BAD
        assert [g["members"] for g in W["merged"]] == [2, 1] and W["merged"][0]["lib"] == L - 1


def test_a_deletion_whose_text_is_not_the_reference(route):
    """a hand-made table may spell a deletion otherwise than the reference does: the walk compares the record's OWN bytes for its first
    L steps.  -CA behind the fourth of six As: the A matches, the C does not — one step, whatever the reference holds L positions on"""
    V = View(b"G" + b"A" * 6 + b"TG", pos0=0)
    for text, shift in ((b"-CA", 1), (b"-CAA", 2), (b"-AA", 4), (b"-TCA", 1)):
        T = Tab.of([(4, 0, text, sums(5))])
        W = check(route, V, T, what="deletion %r" % text, W=norm_reference(V, T))      # (no haplotype property: the text is not the reference's)
        assert W["shift"] == [shift] and W["flags"] == [0], (text, W["shift"])


def test_a_scratch_of_zeros(route):
    """the workspace holds whatever the caller left in it: zeros give what 0xA5 gives, with records that are not judged among the others
    (the words behind the judged records' entries are then never written) and a class of several members at the end"""
    ref = b"G" + b"A" * 8 + b"CGTTTTG"
    V = View(ref, pos0=50, n_lib=2)
    s = sums(6)
    for recs in ([(55, 0, "+A", s), (56, 5, "+A", s), (58, 0, "+A", s), (62, 1, "-T", s), (63, 1, "-T", s)],
                 [(52, 0, "", s, 0), (55, 0, "+A", s), (58, 0, "+A", s)], [(55, 0, "+A", s), (58, 0, "+A", s)]):
        T = Tab.of(recs)
        W = check(route, V, T, what="zeros")
        W0 = check(route, V, T, what="zeros", ws_zero=True, W=W)
        assert W["merged"][-1]["members"] == 2


LONG_SHIFTS = (255, 256, 257, 65535, 65536, 65537)


def long_walk_case(u):
    """One repeat of unit u behind a stopper, 65 537 + 16 characters long.  Per free shift s of LONG_SHIFTS an insertion of one unit
    behind the repeat's s-th character (its text: the unit as it ends there) and a deletion of the L characters that follow; and one
    record of either kind placed at the target, the repeat's start, already.  Every record of a kind is the same event: seven records
    become one.  -> (View, Tab, the index of the repeat's first character)"""
    L, start = len(u), 5
    size = max(LONG_SHIFTS) + 16
    rep = (u * (size // L + 1))[:size]
    ref = b"GNNNN" + rep + b"NTN"
    recs = [(start - 1, 0, b"+" + rep[:L], sums(2)), (start - 1, 0, b"-" + rep[:L], sums(3))]
    for s in LONG_SHIFTS:
        p = start + s - 1
        recs.append((p, 0, b"+" + bytes(rep[(s - L + i) % L] for i in range(L)), sums(4 + s % 5)))
        recs.append((p, 0, b"-" + rep[s:s + L], sums(5 + s % 3)))
    return View(ref, pos0=0), Tab.of(recs), start


def shift_by_comparisons(V, T, r, max_shift):
    """a second statement of a record's walk that rewrites no text: still one comparison per step, against the text character the
    step's rotation brings to the end (an insertion) or, behind the deletion's own bytes, the reference's.  test_walks_of_255_to_65537_steps
    holds it against norm_reference's rewriting walk on walk_case's small shifts and on the long ones."""
    p, ln = int(T.pos[r]), int(T.len[r])
    L, t = abs(ln), T.texts()[r][1:]
    s = 0
    while s < max_shift and match(V.R(p - s), t[(L - 1 - s) % L] if ln > 0 else (t[L - 1 - s] if s < L else V.R(p - s + L))):
        s += 1
    return s


@pytest.mark.parametrize("u", [b"AC", b"ACG", b"ACGTTGA"], ids=["L2", "L3", "L7"])
def test_walks_of_255_to_65537_steps(route, u):
    """free shifts of 255, 256, 257, 65 535, 65 536 and 65 537 in a window of about 65 560 positions over one repeat, unit length 2, 3
    and 7, insertions and deletions; max_shift at 2^20 and at exactly the longest free shift (no record stops at the limit: the walk
    asks for the limit only when another step is possible).  The records that walked merge with the one placed at the target."""
    Vs, Ts, free = walk_case()
    assert [shift_by_comparisons(Vs, Ts, r, 1024) for r in range(Ts.m)] == norm_reference(Vs, Ts)["shift"] == [free[r] for r in range(Ts.m)]
    V, T, start = long_walk_case(u)
    L = len(u)
    assert [shift_by_comparisons(V, T, r, capi.INORM_MAX_SHIFT) for r in range(T.m)] == [0, 0] + [s for s in LONG_SHIFTS for _ in (0, 1)]
    for max_shift in (capi.INORM_MAX_SHIFT, max(LONG_SHIFTS)):
        W = check(route, V, T, max_shift=max_shift, what="long walks, max_shift %d" % max_shift)
        assert W["shift"] == [0, 0] + [s for s in LONG_SHIFTS for _ in (0, 1)] and W["status"] == 0 and not any(W["flags"])
        assert all(x == start - 1 for x in W["npos"]) and [g["members"] for g in W["merged"]] == [7, 7]
        assert [g["text"] for g in W["merged"]] == [b"+" + u, b"-" + u] and W["merged"][0]["of"][0] == 0 and W["merged"][0]["of"][-1] == 12
    # the rotation of an insertion's text is by s mod L, with s beyond 2^16 and beyond 2^8: other residues than s mod 2^16 and s mod 2^8 give
    assert L == 2 or any((s & 0xffff) % L != s % L for s in LONG_SHIFTS) and any((s & 0xff) % L != s % L for s in LONG_SHIFTS)
    # one step short of the longest walk: that record alone stops at the limit and stays apart
    W = check(route, V, T, max_shift=max(LONG_SHIFTS) - 1, what="long walks, one step short")
    assert W["flags"][-2:] == [LIMIT, LIMIT] and not any(W["flags"][:-2]) and [g["members"] for g in W["merged"]] == [6, 6, 1, 1]


# ------------------------------------------------------------------------------------------------ 3. merging and order

def fsums(n, f, **kw):
    return sums(n, f=f, **kw)


def test_records_of_different_positions_become_one(route):
    ref = b"G" + b"AC" * 4 + b"T" + b"C" + b"A" * 6 + b"G"
    V = View(ref, pos0=10, n_lib=2)
    rep = (np.arange(100, 110), np.arange(-3, 7))
    recs = [(10, 1, "+AC", sums(3)), (14, 0, "+AC", sums(2)), (15, 0, "+CA", sums(1)), (18, 0, "+AC", sums(1)), (18, 1, "+AC", sums(5)),
            (20, 1, "-A", sums(3)), (23, 0, "-A", sums(2)), (23, 0, "+A", sums(9)), (25, 0, "-A", sums(2))]
    T = Tab.of(recs)
    for r in (rep, None):
        W = check(route, V, T, rep=r, what="merge")
        M = W["merged"]
        assert [(g["pos"], g["lib"], g["text"], g["members"]) for g in M] == [(10, 0, b"+AC", 3), (10, 1, b"+AC", 2), (20, 0, b"+A", 1), (20, 0, b"-A", 2), (20, 1, b"-A", 1)]
        assert M[0]["i"][0] == 4 and M[1]["i"][0] == 8 and W["group"] == [1, 0, 0, 0, 1, 4, 3, 2, 3]
        assert (M[0]["rep_read"], M[0]["rep_qpos"]) == ((101, -2) if r else (0, 0))
    # two insertions that become equal in position but not in text; one that shifts PAST another position's record
    ref = b"G" + b"ACAC" + b"TTT"
    V = View(ref, pos0=0)
    T = Tab.of([(1, 0, "+TA", sums(7)), (2, 0, "+GG", sums(4)), (3, 0, "+CA", sums(2)), (4, 0, "+AC", sums(3)), (4, 0, "+CC", sums(6))])
    W = check(route, V, T, what="order")
    assert [(g["pos"], g["text"]) for g in W["merged"]] == [(0, b"+AC"), (0, b"+AT"), (2, b"+GG"), (3, b"+CC")] and W["group"] == [1, 2, 0, 0, 3]


def test_fp32_sums_follow_the_input_order_and_integer_sums_wrap(route):
    ref = b"G" + b"A" * 6 + b"T"
    V = View(ref, pos0=0)
    # Members a, b, -a in the three input orders that group them differently: (a + b) - a, (a - a) + b, (b - a) + a.  Column 0 carries
    # 1e8, 1, -1e8: in fp32 its first and third order both give 0 (the spacing at 1e8 is 8 on either side), the second gives 1.  Column 1
    # carries 2^27, 5, -2^27: the spacing is 16 above 2^27 and 8 below it, so the three orders give 0, 5 and 8 — all different, asserted
    # on the reference's own results: a sum in any other order fails at least one of the three tables.
    members = [(1e8, 2.0 ** 27), (1.0, 5.0), (-1e8, -2.0 ** 27)]
    got = []
    for order in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
        recs = [(2 * x + 1, 0, "+A", fsums(0xC0000000, (members[o][0], members[o][1], 0.25, 0.5), smq=5, sclip=7)) for x, o in enumerate(order)]
        W = check(route, V, Tab.of(recs), what="fp32 %r" % (order,))
        assert len(W["merged"]) == 1 and W["merged"][0]["members"] == 3
        got.append((float(W["merged"][0]["f"][0]), float(W["merged"][0]["f"][1])))
        assert W["merged"][0]["i"][0] == (3 * 0xC0000000) % 2 ** 32 == 0x40000000
    assert [g[0] for g in got] == [0.0, 1.0, 0.0] and [g[1] for g in got] == [0.0, 5.0, 8.0], got
    # metrics of the merged sums, a count above 2^24
    recs = [(1, 0, "+A", sums((1 << 24) - 1, smq=0xFFFFFFF0, f=(3.0, 5.0, 7.0, 9.0))), (3, 0, "+A", sums(5, smq=77, nq2=3, f=(1.5, 2.5, 3.5, 4.5)))]
    W = check(route, V, Tab.of(recs), what="metrics")
    assert W["merged"][0]["i"][0] == (1 << 24) + 4


# ------------------------------------------------------------------------------------------------ 4. launch boundaries

def homopolymer_table(m, L=2, spread=4, seed=3):
    """m records over a reference of homopolymer runs: insertions and deletions of the run's base placed anywhere in it, two libraries"""
    rng = np.random.default_rng(seed)
    runs = max(m // spread, 1)
    ref = bytearray()
    starts = []
    for x in range(runs):
        ref += b"G" if x & 1 else b"C"
        starts.append(len(ref))
        ref += b"AT"[x % 2:x % 2 + 1] * 6
    ref += b"G"
    recs = []
    for x in range(m):
        q = x * runs // m
        b = b"AT"[q % 2:q % 2 + 1]
        p = 7 + starts[q] + int(rng.integers(0, 5))
        kind = rng.integers(0, 3)
        recs.append((p, int(rng.integers(0, L)), (b"+" + b * (1 + kind)) if kind < 2 else b"-" + b, sums(int(rng.integers(1, 9)), f=tuple(rng.random(4).astype(np.float32)))))
    recs.sort(key=lambda r: r[0])
    return View(bytes(ref), pos0=7, n_lib=L), Tab.of(recs)


@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 255, 256, 257])
def test_table_lengths(route, m):
    V, T = homopolymer_table(m)
    W = check(route, V, T, what="m %d" % m)
    if m > 1:
        assert len(W["merged"]) < m
    W = check(route, V, T, stride=m + 5, what="stride wider than m", W=W)


def test_classes_across_a_wave_edge_a_block_edge_and_a_long_run(route):
    ref = bytearray(b"GT" * 200)
    ref[100:106] = b"CAAAAA"; ref[300:306] = b"CAAAAA"
    recs = [(x if x < 62 else 101 + (x - 62), 0, "+A" if 62 <= x <= 66 else "+C", sums(1 + x % 5)) for x in range(254)]
    recs += [(301 + x, 0, "+A", sums(2 + x)) for x in range(5)] + [(330 + x, 0, "+C", sums(1)) for x in range(20)]
    T = Tab.of(recs)
    V = View(bytes(ref))
    W = check(route, V, T, what="edges")
    big = sorted(g["of"] for g in W["merged"] if g["members"] == 5)
    assert big == [[62, 63, 64, 65, 66], [254, 255, 256, 257, 258]]
    # 65 records at one normalised position: 13 texts x 5 placements
    ref = b"G" + b"A" * 11 + b"T"
    texts = ["+" + "A" * k for k in range(1, 8)] + ["-" + "A" * k for k in range(1, 7)]
    recs = sorted([(p, 0, t, sums(1 + p)) for t in texts for p in range(1, 6)], key=lambda r: r[0])
    assert len(recs) == 65
    W = check(route, View(ref), Tab.of(recs), what="a long run")
    assert {g["pos"] for g in W["merged"]} == {0} and len(W["merged"]) == 13


def test_a_window_of_65537_positions(route):
    """records only in the first and the last tile of the window: the scan's second round of partials carries nothing in between"""
    n = 65537
    ref = bytearray(b"G" * n)
    ref[1:6] = b"AAAAA"; ref[n - 8:n - 2] = b"CCCCCT"
    T = Tab.of([(3, 0, "+A", sums(2)), (5, 0, "+A", sums(3)), (n - 6, 0, "+C", sums(4)), (n - 4, 0, "+C", sums(5)), (n - 1, 0, "+T", sums(1))])
    W = check(route, View(bytes(ref)), T, what="65537 positions")
    assert [(g["pos"], g["members"]) for g in W["merged"]] == [(0, 2), (n - 9, 2), (n - 1, 1)]


def test_65537_records_of_which_every_second_merges(route):
    m = 65537
    ref = (b"GAAT" * (m // 2 + 1))
    pos = np.repeat(np.arange(m // 2 + 1) * 4, 2)[:m] + 1 + (np.arange(m) & 1)          # ...GAAT: records behind the first and the second A
    f = np.zeros((4, m), np.float32); f[0] = np.arange(m) * 0.25
    i = np.zeros((9, m), np.uint32); i[0] = 1 + (np.arange(m) % 7); i[3] = i[0]
    T = Tab(pos, np.zeros(m), np.ones(m), i, f, np.arange(m + 1) * 2, b"+A" * m)
    W = check(route, View(ref), T, what="65537 records")
    assert len(W["merged"]) == m // 2 + 1 and W["merged"][-1]["members"] == 1 and W["merged"][0]["members"] == 2


def test_caps_one_short_counts_alone_each_destination_alone_and_two_calls(route):
    V, T = homopolymer_table(70)
    W = check(route, V, T, what="all")
    check(route, V, T, short=(1, 0), what="cap short", W=W)
    check(route, V, T, short=(0, 1), what="alleles_cap short", W=W)
    check(route, V, T, short=(1, 1), what="both short", W=W)
    for k in EVERY:
        check(route, V, T, want=(k,), what="alone: " + k, W=W)
    check(route, V, T, want=(), what="nothing wanted", W=W)
    mm, nb = len(W["merged"]), sum(len(g["text"]) for g in W["merged"])
    a = call(route, V, T, cap=mm, acap=nb)
    b = call(route, V, T, cap=mm, acap=nb)
    assert a[0] == b[0] == 0 and all(np.array_equal(a[1][k], b[1][k]) for k in a[1])
    rc, got = call(route, V, T, cap=0, acap=0)                # cap 0: the counts, the per-input arrays and allele_off[0]
    e = expected(W, T, 0, 0)
    assert rc == 0 and all(np.array_equal(got[k], e[k]) for k in e)


# ------------------------------------------------------------------------------------------------ 5. refusals

def test_refused_calls_write_nothing(route):
    V, T = homopolymer_table(20)
    W = norm_reference(V, T)
    mm, nb = len(W["merged"]), sum(len(g["text"]) for g in W["merged"])
    other = capi.MEM_HOST if route.mem == capi.MEM_DEVICE else capi.MEM_DEVICE

    def altered(**kw):
        def f(d):
            for k, x in kw.items():
                setattr(d, k, x)
            return d
        return f
    need = route.inorm.workspace(V.n_pos, T.m)
    assert need > 0 and route.inorm.workspace(0, 5) == 0 and route.inorm.workspace(5, 0) == 0 and route.inorm.workspace(V.n_pos, T.m + 1) > need
    cases = [("no handle", dict(handle=False)), ("no view", dict(view=False)), ("no params", dict(params=False)), ("no source", dict(source=False)),
             ("k0 < 0", dict(k0=-1, n=3)), ("n < 0", dict(n=-1)), ("k0 + n > n_pos", dict(k0=2, n=V.n_pos - 1)), ("cap < 0", dict(cap=-1)),
             ("alleles_cap < 0", dict(acap=-1)), ("memory of the other kind", dict(dview=altered(memory=other))), ("memory 0", dict(dview=altered(memory=0))),
             ("another device", dict(dview=altered(device=1))), ("no workspace", dict(ws=False)), ("workspace one word short", dict(wsb=need - 4)),
             ("max_shift out of range", dict(max_shift=capi.INORM_MAX_SHIFT + 1)), ("a reserved word", dict(reserved=(0, 0, 1))),
             ("a reserved word", dict(reserved=(7, 0, 0))), ("m < 0", dict(sfields=dict(m=-1))), ("stride < m", dict(stride=T.m - 1)),
             ("alleles_len < 0", dict(sfields=dict(alleles_len=-1))), ("not a computed region", dict(dview=altered(n_lib=0)))]
    cases += [("no " + k, dict(sfields={k: None})) for k in ("pos", "lib", "len", "istat", "fstat", "allele_off", "alleles")]
    for what, kw in cases:
        kw = dict(dict(cap=mm, acap=nb), **kw)
        rc, got = call(route, V, T, **kw)
        assert rc == capi.E_ARG and untouched(got), what
        if what != "no handle":
            assert route.inorm.lib.brc_inorm_last_error(route.inorm.h) != b"", what
    # m == 0 and n == 0 are fine: counts = {0, 0}, allele_off[0] = 0, status = 0, nothing else
    for what, kw, TT in (("m == 0", {}, Tab.of([])), ("n == 0", dict(k0=3, n=0), T)):
        rc, got = call(route, V, TT, cap=4, acap=4, ws=False, **kw)
        assert rc == 0 and list(got["counts"][:2]) == [0, 0] and got["allele_off"][0] == 0 and got["status"][0] == 0, what
        got["counts"][:2] = SENT; got["allele_off"][0] = SENT; got["status"][0] = SENT
        assert untouched(got) and route.inorm.lib.brc_inorm_last_error(route.inorm.h) == b"", what


# ------------------------------------------------------------------------------------------------ 6. an engine's table

X_REP, X_HOMO = 500, 800
N_CTL = 3


@pytest.fixture(scope="module")
def repeats(oracle_lib):
    """A synthetic two-library batch in the manner of test_ivet.two_libs, over a reference with a hand-written G ACACAC T repeat and a
    C AAAAAA G run: case reads carry +AC behind the last unit (two reads), the same event one base and one unit to the left (one read
    each, the first with the rotated text), control reads at the leftmost placement; a 1-base deletion at the right end (two case
    reads), in the middle (two) and at the left end (control) of the run."""
    import synth
    rng = np.random.default_rng(33)
    ref = bytearray(synth.make_ref(rng, 3000))
    ref[X_REP - 25:X_REP + 30] = bytes(ref[X_REP - 25:X_REP + 30]).upper().replace(b"A", b"T").replace(b"C", b"G")
    ref[X_REP:X_REP + 8] = b"GACACACT"
    ref[X_HOMO - 25:X_HOMO + 30] = bytes(ref[X_HOMO - 25:X_HOMO + 30]).upper().replace(b"A", b"T")
    ref[X_HOMO:X_HOMO + 8] = b"CAAAAAAG"
    main = synth.make_batch(92, bytes(ref), 700, read_len=(60, 120), style="indel", n_libs=2)
    rows = [ti.ins_read(X_REP + 6, "AC", 0)] * 2 + [ti.ins_read(X_REP + 5, "CA", 0), ti.ins_read(X_REP + 4, "AC", 0)] + [ti.ins_read(X_REP, "AC", 1)] * N_CTL
    rows += [ti.del_read(X_HOMO + 5, 1, 0)] * 2 + [ti.del_read(X_HOMO + 3, 1, 0)] * 2 + [ti.del_read(X_HOMO, 1, 1)] * N_CTL
    arrs = ti.merged([main, ti.hand_reads(bytes(ref), rows)])
    res, _ = td.oracle_result(oracle_lib, arrs, 50, 2950, bytes(ref), **ts.PER_LIB)
    return bytes(ref), arrs, res


def raw_records(T, text, lib):
    """{position: count} of the records of one text and library within the hand-written stretches"""
    texts = T.texts()
    return {int(T.pos[x]): int(T.istat[0, x]) for x in range(T.m) if texts[x] == text and T.lib[x] == lib and min(abs(int(T.pos[x]) - X_REP), abs(int(T.pos[x]) - X_HOMO)) < 20}


def check_table(route, norm, W, T, what):
    """tensors.normalize_indels' dict against the reference"""
    M = W["merged"]
    assert norm["m"] == len(M) and (norm["first"], norm["n"]) == (W["first"], W["n"]), what
    e = expected(W, T, len(M), sum(len(g["text"]) for g in M))
    for k in PER_OUT + ("istat", "fstat", "metrics", "allele_off"):
        if k in norm:
            g = tv.host_words(route, norm[k]).ravel()
            assert np.array_equal(g, e[k][:g.size]) and (e[k][g.size:] == SENT).all(), (what, k)
    if "alleles" in norm:
        assert bytes(np.asarray(route.host(norm["alleles"]))) == b"".join(g["text"] for g in M), what
    for k in PER_IN:
        assert np.array_equal(tv.host_words(route, norm["src"][k]), e[k][:T.m]), (what, k)
    assert int(tv.host_words(route, norm["status"])[0]) == W["status"], what
    for a in [norm[k] for k in PER_OUT if k in norm] + list(norm["src"].values()):
        assert isinstance(a, np.ndarray) if route.name == "sim" else a.is_cuda, what


def engine_reference(d, ref, T, t, rep, max_shift=1024):
    V = View.of_engine(d, ref)
    W = norm_reference(V, T, t["first"] - V.pos0, t["n"], max_shift, rep)
    props(V, T, W, max_shift)
    W["first"] = t["first"]
    return V, W


def oracle_rep(res):
    return ([d["rep_read"] for d in res.indels], [d["rep_qpos"] for d in res.indels])


def test_an_engines_table_test_bam(route, oracle_lib, test_bam):
    from bam_readcount_amd import tensors
    beg0, end = 10402736, 10405248
    res, _ = td.oracle_result(oracle_lib, test_bam, beg0, end, test_bam["ref"], tid=20)
    eng = td.computed(route.engine_lib, test_bam, beg0, end, test_bam["ref"], tid=20)
    t, T = tiv.gathered_table(route, eng, res, "test_bam")
    d = eng.device_indels()
    V, W = engine_reference(d, test_bam["ref"], T, t, oracle_rep(res))
    assert T.m > 3 and len(W["merged"]) <= T.m
    check_table(route, tensors.normalize_indels(eng, route.inorm, t), W, T, "test_bam")
    check(route, V, T, t["first"] - V.pos0, t["n"], rep=oracle_rep(res), what="test_bam, raw", W=W)
    eng.close()


def test_an_engines_table_and_the_chain_over_repeats(route, repeats):
    """THE TEST THAT FAILS WITHOUT THE FEATURE: over the raw table the control's record of the same event, placed elsewhere in the repeat,
    does not veto, and the split case-side records each fail min_var_count; over the normalised table the merged record passes it and
    carries CTL_ALLELE with the control's read count"""
    from bam_readcount_amd import tensors
    ref, arrs, res = repeats
    D = tv.Dense.of(res)
    T = Tab.of_oracle(res.indels)
    # the oracle's list holds the placements as separate records
    assert raw_records(T, b"+AC", 0).items() >= {X_REP + 6: 2, X_REP + 4: 1}.items() and raw_records(T, b"+CA", 0) == {X_REP + 5: 1}
    assert raw_records(T, b"+AC", 1) .get(X_REP) == N_CTL
    assert raw_records(T, b"-A", 0).items() >= {X_HOMO + 5: 2, X_HOMO + 3: 2}.items() and raw_records(T, b"-A", 1).get(X_HOMO) == N_CTL
    eng = td.computed(route.engine_lib, arrs, 50, 2950, ref, **ts.PER_LIB)
    v, d = ts.views_of(eng)
    t, _ = tiv.gathered_table(route, eng, res, "repeats")
    V, W = engine_reference(d, ref, T, t, oracle_rep(res))
    norm = tensors.normalize_indels(eng, route.inorm, t)
    check_table(route, norm, W, T, "repeats")
    by = {(g["pos"], g["lib"], g["text"]): g for g in W["merged"]}
    assert by[(X_REP, 0, b"+AC")]["i"][0] == 4 and by[(X_REP, 0, b"+AC")]["members"] == 3 and by[(X_REP, 1, b"+AC")]["i"][0] == N_CTL
    assert by[(X_HOMO, 0, b"-A")]["i"][0] == 4 and by[(X_HOMO, 0, b"-A")]["members"] == 2 and by[(X_HOMO, 1, b"-A")]["i"][0] == N_CTL
    thr = tiv.T_(min_var_count=3, ctl_max_count=1, ctl_frac_num=1, ctl_frac_den=2)
    role = [CASE, CTL]
    BIT = tiv.BIT
    # over the raw table: no veto, and every part fails min_var_count
    raw = tensors.vet_indels(eng, route.ivet, t, role=role, **thr)
    wraw = tiv.reference(D, T, role=role, **thr)
    tiv.check_tensors(route, dict(raw, keep=raw["keep"]), wraw, "raw")
    parts = [x for x in range(T.m) if T.lib[x] == 0 and W["group"][x] in (W["merged"].index(by[(X_REP, 0, b"+AC")]), W["merged"].index(by[(X_HOMO, 0, b"-A")]))]
    assert len(parts) == 5
    for x in parts:
        assert not wraw[0][x] & BIT["CTL_ALLELE"] and wraw[2][x] == 0 and wraw[0][x] & BIT["VAR_COUNT"], x
    # over the normalised table
    NT = merged_tab(W)
    r = tensors.vet_indels(eng, route.ivet, norm, role=role, **thr)
    wn = tiv.reference(D, NT, role=role, **thr)
    tiv.check_tensors(route, r, wn, "normalised")
    for key in ((X_REP, 0, b"+AC"), (X_HOMO, 0, b"-A")):
        g = W["merged"].index(by[key])
        assert wn[0][g] & BIT["CTL_ALLELE"] and wn[2][g] == N_CTL and not wn[0][g] & BIT["VAR_COUNT"], key
    # the verdicts back on the raw records
    grp = norm["src"]["group"]
    fail = r["fail"].view(np.int32 if route.name == "sim" else route.torch.int32)
    back = tv.host_words(route, fail[grp if route.name == "sim" else grp.long()])
    assert np.array_equal(back, wn[0][np.array(W["group"])]) and min(W["group"]) >= 0
    assert all(back[x] & BIT["CTL_ALLELE"] for x in parts)
    eng.close()


# ------------------------------------------------------------------------------------------------ 7. tensors.normalize_indels

def test_tensors_normalize_indels_on_text_only_engines_a_site_lists_table_and_its_errors(route, oracle_lib, test_bam, repeats):
    from bam_readcount_amd import tensors
    import test_panel as tp
    beg0, end = 10402736, 10405248
    res, text = td.oracle_result(oracle_lib, test_bam, beg0, end, test_bam["ref"], tid=20, chrom="21")
    T = Tab.of_oracle(res.indels)
    for opts in (dict(text_only=True), dict(device_text="21")):
        eng = td.computed(route.engine_lib, test_bam, beg0, end, test_bam["ref"], tid=20, **opts)
        t = tensors.indels(eng, route.indels)
        V, W = engine_reference(eng.device_indels(), test_bam["ref"], T, t, oracle_rep(res), max_shift=3)
        check_table(route, tensors.normalize_indels(eng, route.inorm, t, max_shift=3), W, T, "before fetch %r" % opts)
        eng.fetch_result()
        assert eng.format_region("21") == text
        r = tensors.normalize_indels(eng, route.inorm, t, max_shift=3, want=("pos", "members"))
        assert sorted(r) == ["first", "m", "members", "n", "pos", "src", "status"]
        check_table(route, r, W, T, "after fetch %r" % opts)
        r = tensors.normalize_indels(eng, route.inorm, {k: x for k, x in t.items() if not k.startswith("rep_")}, max_shift=3, want=())
        assert np.array_equal(tv.host_words(route, r["src"]["group"]), np.array(W["group"]).astype(np.uint32)) and r["m"] == len(W["merged"])
        wrong = (lambda a, dt: a.astype(dt)) if route.name == "sim" else (lambda a, dt: a.to(getattr(route.torch, dt)))
        bad = [dict(max_shift=-1), dict(max_shift=capi.INORM_MAX_SHIFT + 1), dict(max_shift=1.5), dict(max_shift=True), dict(want=("nothing",)), dict(table=None),
               dict(table=dict(m=3)), dict(table={k: x for k, x in t.items() if k != "alleles"}), dict(table={k: x for k, x in t.items() if k != "first"}),
               dict(table=dict(t, m=T.m + 1)), dict(table=dict(t, pos=wrong(t["pos"], "int64"))), dict(table=dict(t, fstat=t["istat"])),
               dict(table=dict(t, istat=t["istat"][:4])), dict(table=dict(t, alleles=wrong(t["alleles"], "int32"))), dict(table=dict(t, first=beg0 - 100)),
               dict(table=dict(t, n=res.n_pos + 1)), dict(table=dict(t, rep_read=wrong(t["rep_read"].view(t["pos"].dtype), "int16")))]
        for b in bad:
            with pytest.raises(ValueError):
                tensors.normalize_indels(eng, route.inorm, b.pop("table", t), **b)
        eng.close()
    # the table of a site list (strided on the host route)
    panel = route.another("panel")
    ref, arrs, res = repeats
    T = Tab.of_oracle(res.indels)
    eng = td.computed(route.engine_lib, arrs, 50, 2950, ref, **ts.PER_LIB)
    listed = [X_REP, X_REP + 4, X_REP + 5, X_REP + 6, X_HOMO, X_HOMO + 5]
    ps = tensors.sites(eng, panel, positions=listed, want=("depth",), indels=route.indels)
    sel = [x for x in range(T.m) if T.pos[x] in listed]
    sub = T.take(sel)
    rep = oracle_rep(res)
    V, W = engine_reference(eng.device_indels(), ref, sub, ps["indels"], ([rep[0][x] for x in sel], [rep[1][x] for x in sel]))
    assert (W["merged"][0]["pos"], W["merged"][0]["lib"], W["merged"][0]["members"]) == (X_REP, 0, 3)
    check_table(route, tensors.normalize_indels(eng, route.inorm, ps["indels"]), W, sub, "the table of a site list")
    eng.close()


# ------------------------------------------------------------------------------------------------ 8. the host sanitizers

def _serialize(V, calls):
    """the view and the calls as inorm_check.cpp reads them"""
    ref = V.ref or b""
    b = struct.pack("<iiqiqqqq", V.n_lib, V.pos0, V.n_pos, 0 if V.ref is None else 1, V.ref_lo, V.ref_hi, V.ref_len, len(ref)) + ref + struct.pack("<i", len(calls))
    for T, k0, n, ms, cap, acap, rep, want in calls:
        b += struct.pack("<qqqqqqIii", k0, n, T.m, T.alleles.size, cap, acap, ms, 1 if rep else 0, want)
        b += T.pos.astype(np.int32).tobytes() + T.lib.astype(np.int32).tobytes() + T.len.astype(np.int32).tobytes()
        if rep:
            b += np.asarray(rep[0], np.uint32).tobytes() + np.asarray(rep[1], np.int32).tobytes()
        b += T.istat.tobytes() + T.fstat.tobytes() + T.off.tobytes() + T.alleles.tobytes()
    return b


def _sanitized(tmp_path, name, V, calls):
    """inorm_check_asan over one view: every call must return 0 without a report and give the reference's words, every destination that
    was not wanted as it was filled; returns the number of records compared"""
    full = []
    for T, k0, n, ms, short, rep, want in calls:
        W = norm_reference(V, T, k0, n, ms, rep)
        props(V, T, W, ms)
        mm, nb = len(W["merged"]), sum(len(g["text"]) for g in W["merged"])
        full.append((T, k0, W["n"], ms, max(mm - short, 0), max(nb - short, 0), rep, want, W))
    case, out = str(tmp_path / (name + ".bin")), str(tmp_path / (name + ".res"))
    open(case, "wb").write(_serialize(V, [c[:8] for c in full]))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    pr = subprocess.run([side.sim_checker(side.SIDE["inorm"]), case, out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert pr.returncode == 0, (name, pr.stderr.decode()[-3000:])
    assert pr.stdout.decode().strip() == "%d calls" % len(calls), name
    raw = np.fromfile(out, np.uint8); o = 0
    some = 0
    for T, k0, n, ms, cap, acap, rep, want, W in full:
        names = (("counts",) if want & 1 else ()) + (PER_IN if want & 2 else ()) + (PER_OUT + ("istat", "fstat", "metrics", "allele_off", "alleles") if want & 4 else ()) + \
            (("status",) if want & 8 else ())
        e = expected(W, T, cap, acap, names)
        assert raw[o:o + 4].view(np.int32)[0] == 0, (name, T.m)
        o += 4
        for k, size in [("status", 1), ("counts", 2)] + [(k, T.m) for k in PER_IN] + [(k, cap) for k in PER_OUT] + [(k, f * cap) for k, f in PLANES] + [("allele_off", cap + 1)]:
            g = raw[o:o + 4 * size].view(np.uint32); o += 4 * size
            assert np.array_equal(g, e[k][:size]), (name, T.m, k)
        assert np.array_equal(raw[o:o + acap], e["alleles"][:acap]), (name, T.m, "alleles")
        o += acap
        some += T.m
    assert o == raw.size, name
    return some


def test_calls_under_the_host_sanitizers(sim_route, tmp_path):
    """A subset of the hand-made cases above on the CPU build with -fsanitize=address,undefined, a stand-alone program: the reference slice
    and the table of exactly their sizes, a scratch of exactly brc_inorm_workspace bytes, destinations of exactly the caps — a load or
    store outside them is a report — and the results are the reference's.  Never under the gpu mark; nothing is loaded into python with
    a sanitizer."""
    some = 0
    V, T, _ = walk_case()
    some += _sanitized(tmp_path, "walk", V, [(T, 0, None, 1024, 0, None, 15), (T, 0, None, 2, 0, None, 15), (T, 0, None, 0, 1, None, 15), (T, 7, V.n_pos - 20, 1024, 0, None, 15)])
    V, T, _ = walk_case(lower=True)
    some += _sanitized(tmp_path, "lower", V, [(T, 0, None, 1024, 0, None, w) for w in (15, 1, 2, 4, 8, 0)])
    for m in (0, 1, 63, 64, 65, 256, 257):
        V, T = homopolymer_table(m)
        rep = (np.arange(m), -np.arange(m))
        some += _sanitized(tmp_path, "m%d" % m, V, [(T, 0, None, 1024, 0, rep, 15), (T, 0, None, 1024, 1, None, 15), (T, 3, max(V.n_pos - 9, 0), 1, 0, None, 15)])
    # not-judged records and broken offsets
    ref = b"G" + b"A" * 8 + b"CGTTTTG"
    V = View(ref, pos0=50, n_lib=2)
    s = sums(6)
    T = Tab.of([(49, 0, "+A", s), (52, 0, "", s, 0), (55, 0, "+A", s), (56, -1, "+A", s), (56, 2, "+A", s), (57, 0, "+A", s, 2), (57, 0, "-A", s, 1), (58, 1, "+A", s),
                (63, 1, "-T", s), (64, 0, "-G", s), (65, 1, "+GG", s), (50 + len(ref), 0, "+A", s), (2 ** 31 - 1, 0, "+A", s), (-2 ** 31, 0, "-A", s, -2 ** 31)])
    calls = [(T, 0, None, 1024, 0, None, 15)]
    for x, val in ((1, T.alleles.size + 1000), (2, 0xFFFFFFFF), (3, 0), (T.m, 0xFFFFFFF0), (T.m, 1), (9, 2)):
        B = Tab(T.pos, T.lib, T.len, T.istat, T.fstat, T.off.copy(), T.alleles)
        B.off[x] = val
        calls.append((B, 0, None, 1024, 0, None, 15))
    some += _sanitized(tmp_path, "not_judged", V, calls)
    some += _sanitized(tmp_path, "no_reference", View(None, pos0=50, n_pos=20, n_lib=2), [(T, 0, None, 1024, 0, None, 15)])
    assert some > 2500
