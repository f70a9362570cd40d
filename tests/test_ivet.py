"""Device-side indel candidate filter (include/brc_ivet.h): brc_ivet_records and bam_readcount_amd.tensors.vet_indels against the header's
predicate written in numpy uint64 / float32 over the ORACLE's brc_result — depth, istat, fstat, refbase and the sorted indel list with
its texts; averages by numpy's fp32 division — fail, keep, vals and ctl_count equal as bit patterns, no tolerance, no cell left out.

Every body runs twice (the `route` fixture): [sim] = libbrc_sim.so + tests/sim_ivet/libbrc_ivet_sim.so, host memory, in the CPU suite;
[hip] = the product's libraries on the GPU (gpu-marked), table, lists, scratch and destinations in device memory allocated through
torch.  Destinations are filled with 0xA5A5A5A5 first and are PAD elements wider than needed: elements behind the contract's size and
every destination that was not asked for must keep it.  The scratch has exactly brc_ivet_workspace bytes.

Where no engine can produce the shape the views are test_vet.full_views and the table is written by hand (`Tab`), in the route's
memory; the reference is the same numpy predicate.  Sizes that matter to the kernels (brc_ivet.hip): a wave is 64 consecutive table
records, a workgroup 256."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from bam_readcount_amd import capi
import abi_side as side
import handmade_views as hv
from route import Route, SENT
import test_dense as td
import test_indels as ti
import test_select as ts
import test_vet as tv

LIBS = tv.LIBS + ("ivet", "indels")
PAD = 3
NVAL = capi.IVET_NVAL
ALL = ("fail", "vals", "ctl_count", "keep")
BIT = capi.IVET_BIT
ALL_TESTS = capi.IVET_ALL_TESTS
NOT_ASKED, NO_SITE = capi.IVET_NOT_ASKED, capi.IVET_NO_SITE
INS, DEL = capi.WHY_INS, capi.WHY_DEL
IGN, CASE, CTL = capi.ROLE_IGNORE, capi.ROLE_CASE, capi.ROLE_CONTROL
F32, U64, U32 = np.float32, np.uint64, 2 ** 32 - 1
MCOL = tv.MCOL
PER_LIB = ts.PER_LIB
# thresholds that judge nothing: every test passes on any finite data and any control record
OPEN = dict({k: x for k, x in tv.OPEN.items() if k != "min_var_bq"}, ctl_min_depth=0, ctl_max_count=U32, ctl_frac_num=U32, ctl_frac_den=1)


def T_(**kw):
    return dict(OPEN, **kw)


# thresholds that split real data
MID = dict({k: x for k, x in tv.MID.items() if k != "min_var_bq"}, min_depth=4, min_var_count=2, min_var_rl=50.0, min_ref_rl=50.0, ctl_min_depth=3,
           ctl_max_count=1, ctl_frac_num=1, ctl_frac_den=4)
EASY = T_(min_depth=4, min_var_count=2, freq_num=1, freq_den=20, min_var_mapq=15.0, min_ref_mapq=15.0, ctl_max_count=1, ctl_frac_num=1, ctl_frac_den=2)


@pytest.fixture(scope="module", params=["sim", pytest.param("hip", marks=pytest.mark.gpu)])
def route(request):
    return Route(request.param, LIBS, engine=True)


@pytest.fixture(scope="module")
def sim_route():
    return Route("sim", LIBS, engine=True)


# ------------------------------------------------------------------------------------------------ tables

def sums(n, plus=None, smq=None, sse=0, nq2=0, smmq=0, sclip=None, f=(0.0, 0.0, 0.0, 0.0)):
    """the 9 + 4 sums of an indel bucket of n reads (BRC_I_* / BRC_F_* order; no base-quality sum)"""
    plus = n // 2 if plus is None else plus
    return ([n, 60 * n if smq is None else smq, sse, plus, n - plus, nq2, smmq, 100 * n if sclip is None else sclip, 0], list(f))


class Tab:
    """an indel table on the host: pos, lib, len int64 [m], istat uint32 [9, m], fstat float32 [4, m], allele_off uint32 [m + 1], alleles uint8"""

    def __init__(self, pos, lib, ln, istat, fstat, off, alleles):
        self.pos, self.lib, self.len = (np.asarray(x, np.int64).reshape(-1) for x in (pos, lib, ln))
        self.m = self.pos.size
        self.istat = np.asarray(istat, np.uint32).reshape(9, self.m); self.fstat = np.asarray(fstat, np.float32).reshape(4, self.m)
        self.off = np.asarray(off, np.uint32).reshape(-1); self.alleles = np.frombuffer(bytes(alleles), np.uint8).copy()
        assert self.off.size == self.m + 1

    @classmethod
    def of(cls, recs):
        """recs: (pos, lib, text with its sign first, (i[9], f[4])[, len]) in table order; len follows from the text where not given"""
        text = [r[2].encode("latin1") if isinstance(r[2], str) else bytes(r[2]) for r in recs]
        ln = [r[4] if len(r) > 4 else (len(t) - 1) * (1 if t[:1] == b"+" else -1) for r, t in zip(recs, text)]
        ist = np.array([r[3][0] for r in recs], np.uint32).reshape(len(recs), 9).T
        fst = np.array([r[3][1] for r in recs], np.float32).reshape(len(recs), 4).T
        return cls([r[0] for r in recs], [r[1] for r in recs], ln, ist, fst, np.concatenate([[0], np.cumsum([len(t) for t in text])]), b"".join(text))

    @classmethod
    def of_oracle(cls, indels):
        return cls.of([(d["pos"], d["lib"], d["allele"], (d["i"], d["f"]), d["len"]) for d in indels])

    def texts(self):
        """text(x) of the header: clamped to alleles, empty when the offsets descend"""
        A = self.alleles.size
        a = self.alleles.tobytes()
        return [a[min(int(self.off[x]), A):min(int(self.off[x + 1]), A)] for x in range(self.m)]

    def take(self, sel):
        sel = np.asarray(sel, np.int64)
        t = self.texts()
        return Tab(self.pos[sel], self.lib[sel], self.len[sel], self.istat[:, sel], self.fstat[:, sel],
                   np.concatenate([[0], np.cumsum([len(t[x]) for x in sel])]), b"".join(t[x] for x in sel))


def roles_of(role, L):
    return np.full(L, CASE, np.int64) if role is None else np.asarray(role, np.int64)


def reference(D, T, idx=None, why=None, role=None, kinds=INS | DEL, tests=ALL_TESTS, with_text=True, **t):
    """The header's predicate: (fail uint32 [m], vals float32 [NVAL, m], ctl_count uint32 [m], keep uint32 [n], status)"""
    m, L, P = T.m, D.n_lib, D.n_pos
    role = roles_of(role, L)
    k = T.pos - D.pos0
    inr = (k >= 0) & (k < P) & (T.lib >= 0) & (T.lib < L)
    kk, ll = np.where(inr, k, 0), np.where(inr, T.lib, 0)
    kind = np.where(T.len > 0, INS, DEL)
    rb = np.where(inr, D.rb[kk], -1) if P else np.full(m, -1)
    status = 0
    if ((T.len != 0) & ~inr).any():
        status |= capi.IVET_TABLE_OUT_OF_RANGE
    if (T.pos[1:] < T.pos[:-1]).any():
        status |= capi.IVET_TABLE_NOT_ASCENDING
    not_asked = (T.len == 0) | (inr & ((role[ll] != CASE) | ((kind & kinds) == 0)))
    no_site = (T.len != 0) & (~inr | (~not_asked & (rb < 0)))
    judged = ~not_asked & ~no_site
    r = np.maximum(rb, 0) + 1
    Dl, Cr = D.depth[ll, kk], D.istat[ll, r, 0, kk]
    mr = D.metrics[ll[:, None], r[:, None], np.array(MCOL)[None, :], kk[:, None]] if m else np.zeros((0, 6), F32)
    mv = ti.metrics_of(T.istat, T.fstat)[np.array(MCOL)].T.copy()
    mv[:, 2] = 0                                            # (AVG_BQ: indel buckets carry no base-quality sum)
    Cv, Pv, Mv = T.istat[0], T.istat[3], T.istat[4]
    S = Pv.astype(U64) + Mv.astype(U64)
    f = np.zeros(m, np.uint32)

    def bit(name, cond):
        f[cond] |= BIT[name]
    bit("DEPTH", Dl < np.uint32(t["min_depth"]))
    bit("VAR_COUNT", Cv < np.uint32(t["min_var_count"]))
    bit("VAR_FREQ", Cv.astype(U64) * U64(t["freq_den"]) < U64(t["freq_num"]) * Dl.astype(U64))
    bit("STRAND", (S >= U64(t["min_strand_reads"])) & (np.minimum(Pv, Mv).astype(U64) * U64(t["strand_den"]) < U64(t["strand_num"]) * S))
    var, ref = Cv > 0, Cr >= np.uint32(t["min_ref_reads"])
    for c, (name, key) in enumerate((("READPOS", "readpos"), ("DIST3", "dist3"), ("BQ", "bq"), ("MAPQ", "mapq"), ("MMQS", None), ("RL", "rl"))):
        if key and name != "BQ":
            bit("VAR_" + name, var & (mv[:, c] < F32(t["min_var_" + key])))
        if key:
            bit("REF_" + name, ref & (mr[:, c] < F32(t["min_ref_" + key])))
    bit("VAR_MMQS", var & (mv[:, 4] > F32(t["max_var_mmqs"])))
    d_mmqs, d_mapq, d_rl = mv[:, 4] - mr[:, 4], mr[:, 3] - mv[:, 3], mr[:, 5] - mv[:, 5]
    with np.errstate(over="ignore"):
        bound = F32(t["max_rl_diff"]) * mr[:, 5]
    assert d_rl.dtype == np.float32 and bound.dtype == np.float32
    bit("MMQS_DIFF", var & ref & (d_mmqs > F32(t["max_mmqs_diff"])))
    bit("MAPQ_DIFF", var & ref & (d_mapq > F32(t["max_mapq_diff"])))
    bit("RL_DIFF", var & ref & (d_rl > bound))
    ctl_libs = np.nonzero(role == CTL)[0]
    if ctl_libs.size and m:
        bit("CTL_DEPTH", (D.depth[ctl_libs][:, kk] < np.uint32(t["ctl_min_depth"])).any(axis=0))
    ctl_count = np.zeros(m, np.uint32)
    text = T.texts()
    for x in range(m if with_text else 0):                      # the run walk, by the contiguous definition
        if not judged[x]:
            continue
        lo = x
        while lo > 0 and T.pos[lo - 1] == T.pos[x]:
            lo -= 1
        hi = x + 1
        while hi < m and T.pos[hi] == T.pos[x]:
            hi += 1
        for y in range(lo, hi):
            c = T.lib[y]
            if y == x or not 0 <= c < L or role[c] != CTL or T.len[y] != T.len[x] or text[y] != text[x]:
                continue
            Cc = int(T.istat[0, y])
            ctl_count[x] = max(ctl_count[x], Cc)
            if not (Cc <= t["ctl_max_count"] and Cc * t["ctl_frac_den"] <= t["ctl_frac_num"] * int(D.depth[c, kk[x]])):
                f[x] |= BIT["CTL_ALLELE"]
    f &= np.uint32(tests)
    with np.errstate(divide="ignore", invalid="ignore"):
        freq = np.where(Dl > 0, Cv.astype(F32) / Dl.astype(F32), F32(0)).astype(F32)
        strand = np.where(S > 0, Pv.astype(F32) / S.astype(F32), F32(0)).astype(F32)
    val = np.stack([Cv.astype(F32), Cr.astype(F32), Dl.astype(F32), freq, strand, d_mmqs.astype(F32), d_mapq.astype(F32), d_rl.astype(F32)] +
                   [mv[:, c] for c in range(6)] + [mr[:, c] for c in range(6)])
    fail = np.where(judged, f, np.where(no_site, NO_SITE, NOT_ASKED)).astype(np.uint32)
    vals = np.where(judged[None, :], val, F32(0)).astype(F32)
    n = 0 if idx is None else len(idx)
    keep = np.zeros(n, np.uint32)
    if n:
        idx = np.asarray(idx, np.int64)
        if ((idx < 0) | (idx >= P)).any():
            status |= capi.IVET_LIST_OUT_OF_RANGE
        if (idx[1:] < idx[:-1]).any():
            status |= capi.IVET_LIST_NOT_ASCENDING
        passed = judged & (fail == 0)
        for j in range(n):
            here = passed & (k == idx[j]) & (0 <= idx[j] < P)
            if why is not None:
                here = here & ((kind & int(why[j])) != 0)
            if here.any():
                keep[j] = np.bitwise_or.reduce(kind[here])
    return fail, vals, ctl_count, keep, status


# ------------------------------------------------------------------------------------------------ calling the library

def call(route, v, d, T, idx=None, why=None, role=None, kinds=INS | DEL, tests=ALL_TESTS, want=ALL, ds=None, status=True, handle=True, params=True,
         table=True, ws=True, no_idx=False, n=None, stride=None, with_text=True, fields=None, tfields=None, **t):
    """brc_ivet_records into sentinel-filled buffers PAD elements wider than the contract's sizes and a scratch of exactly
    brc_ivet_workspace bytes; the table, the lists and the destinations in the route's memory.  Returns (rc, status word, fail words
    [w], vals words [NVAL, w], ctl_count words [w], keep words [wn])"""
    par, keepalive = capi.ivet_params(role, tests, kinds, **t)
    for k, x in (fields or {}).items():
        setattr(par, k, x)
    m = T.m
    stride = m if stride is None else stride
    ist = np.full((9, max(stride, m)), 0xDEADBEEF, np.uint32); ist[:, :m] = T.istat
    fst = np.full((4, max(stride, m)), np.nan, np.float32); fst[:, :m] = T.fstat
    keepbuf = [route.put(x) for x in (T.pos.astype(np.int32), T.lib.astype(np.int32), T.len.astype(np.int32), ist, fst, T.off, T.alleles)]
    tab = capi.IVetTable(m, stride, *[route.ptr(b) for b in keepbuf], T.alleles.size)
    if not with_text:
        tab.allele_off = tab.alleles = None
    for k, x in (tfields or {}).items():
        setattr(tab, k, x)
    idx = np.zeros(0, np.int32) if idx is None else np.asarray(idx, np.int32)
    n = idx.size if n is None else n
    ds = m + PAD if ds is None else ds
    w, wn = max(min(ds, m + PAD), 1), max(n, 0) + PAD
    bf, bv, bc, bk, bs = route.sentinel_words(w), route.sentinel_words(NVAL * w), route.sentinel_words(w), route.sentinel_words(wn), route.sentinel_words(1)
    wsb = route.ivet.workspace(v, m) if v is not None else 0
    assert wsb % 4 == 0
    bw = route.sentinel_words(wsb // 4)
    bi = route.put(idx)
    ba = route.put(np.asarray(why, np.uint32)) if why is not None else None
    rc = route.ivet.lib.brc_ivet_records(route.ivet.h if handle else None, C.byref(v) if v is not None else None, C.byref(d) if d is not None else None,
                                         C.byref(par) if params else None, C.byref(tab) if table else None,
                                         None if (no_idx or (n == 0 and idx.size == 0)) else route.ptr(bi), route.ptr(ba) if ba is not None else None, n, ds,
                                         route.ptr(bf) if "fail" in want else None, route.ptr(bv) if "vals" in want else None,
                                         route.ptr(bc) if "ctl_count" in want else None, route.ptr(bk) if "keep" in want else None,
                                         route.ptr(bs) if status else None, route.ptr(bw) if ws else None, None)
    del keepalive
    return (rc, int(route.words(bs)[0]), route.words(bf)[:w].copy(), route.words(bv)[:NVAL * w].reshape(NVAL, w).copy(), route.words(bc)[:w].copy(),
            route.words(bk)[:wn].copy())


def untouched(*arrays):
    return all((a == SENT).all() for a in arrays)


def check(route, v, d, D, T, idx=None, why=None, role=None, kinds=INS | DEL, tests=ALL_TESTS, what="", want=ALL, **kw):
    """one call against the reference, bit for bit, sentinels included; returns the reference's (fail, vals, ctl_count, keep, status)"""
    t = {k: x for k, x in kw.items() if k in capi.IVET_DEFAULTS}
    with_text = kw.get("with_text", True)
    wf, wv, wc, wk, wst = reference(D, T, idx, why, role, kinds, tests, with_text=with_text, **t)
    m, n = T.m, 0 if idx is None else len(idx)
    rc, st, gf, gv, gc, gk = call(route, v, d, T, idx, why, role, kinds, tests, want=want, **kw)
    assert rc == 0, (what, route.ivet.lib.brc_ivet_last_error(route.ivet.h))
    assert st == wst, (what, st, wst)
    for name, g, w_ in (("fail", gf[:m], wf), ("vals", gv[:, :m], wv.view(np.uint32)), ("ctl_count", gc[:m], wc), ("keep", gk[:n], wk)):
        if name in want:
            assert np.array_equal(g, w_), (what, name, np.argwhere(g != w_)[:4].tolist())
    assert untouched(gf[m:] if "fail" in want else gf, gv[:, m:] if "vals" in want else gv, gc[m:] if "ctl_count" in want else gc,
                     gk[n:] if "keep" in want else gk), "%s: wrote outside its destinations" % what
    return wf, wv, wc, wk, wst


def bits_seen(fail):
    return int(np.bitwise_or.reduce(fail[fail < NOT_ASKED].ravel())) if (fail < NOT_ASKED).any() else 0


# ------------------------------------------------------------------------------------------------ 1. engine fixtures

def gathered_table(route, eng, res, what):
    """tensors.indels over the whole region; shown to equal the oracle's list in pos, lib, len and text first"""
    from bam_readcount_amd import tensors
    t = tensors.indels(eng, route.indels)
    T = Tab.of_oracle(res.indels)
    assert t["m"] == T.m > 0, what
    for k, w in (("pos", T.pos), ("lib", T.lib), ("len", T.len), ("allele_off", T.off), ("alleles", T.alleles)):
        g = tv.host_words(route, t[k]) if k != "alleles" else np.asarray(route.host(t[k]))
        assert np.array_equal(g.view(np.int32) if k in ("pos", "lib", "len") else g, w.astype(np.int32) if k in ("pos", "lib", "len") else w), (what, k)
    return t, T


def check_tensors(route, r, w, what):
    wf, wv, wc, wk, wst = w
    assert np.array_equal(tv.host_words(route, r["fail"]), wf), what
    assert np.array_equal(tv.host_words(route, r["vals"]), wv.view(np.uint32)), what
    assert np.array_equal(tv.host_words(route, r["ctl_count"]), wc), what
    assert np.array_equal(tv.host_words(route, r["keep"]), wk), what
    assert int(tv.host_words(route, r["status"])[0]) == wst, what
    for k in ALL:
        assert isinstance(r[k], np.ndarray) if route.name == "sim" else r[k].is_cuda, (what, k)


def test_golden_fixture_all_lib(route, oracle_lib, test_bam):
    """test_bam.npz all-lib over its whole table: one library, so no control test can fail (the two-library batch below carries those);
    on the reference's side kept and failed records"""
    from bam_readcount_amd import tensors
    beg0, end = 10402736, 10405248
    res, _ = td.oracle_result(oracle_lib, test_bam, beg0, end, test_bam["ref"], tid=20)
    eng = td.computed(route.engine_lib, test_bam, beg0, end, test_bam["ref"], tid=20)
    v, d = ts.views_of(eng)
    D = tv.Dense.of(res)
    t, T = gathered_table(route, eng, res, "test_bam")
    kept = failed = 0
    for name, thr in (("MID", MID), ("EASY", EASY), ("LOOSE", T_(min_var_count=2, min_var_mapq=20.0))):
        w = check(route, v, d, D, T, what="test_bam " + name, **thr)
        kept += int((w[0] == 0).sum()); failed += int(((w[0] != 0) & (w[0] < NOT_ASKED)).sum())
        # ... and the gathered table where it lies
        check_tensors(route, tensors.vet_indels(eng, route.ivet, t, idx=[], **thr), w, "test_bam, tensors " + name)
    assert kept and failed, (kept, failed)
    assert bin(bits_seen(check(route, v, d, D, T, what="test_bam MID", **MID)[0])).count("1") >= 4
    eng.close()


X_SAME, X_SPELL, X_DLEN, X_DSAME, X_PREFIX, X_INSDEL = 600, 700, 800, 900, 1000, 1100


@pytest.fixture(scope="module")
def two_libs(oracle_lib):
    """A synthetic two-library batch (no committed fixture holds a control record of the same allele beside one of another spelling):
    generated reads with indels for depth, and hand-written reads — case-side alleles of four reads, control-side of two or three."""
    import synth
    rng = np.random.default_rng(21)
    ref = bytearray(synth.make_ref(rng, 3000))
    main = synth.make_batch(91, bytes(ref), 700, read_len=(60, 120), style="indel", n_libs=2)
    rows = []
    for x, a, b in ((X_SAME, "AC", "AC"), (X_SPELL, "AC", "AG"), (X_PREFIX, "AC", "ACG")):
        rows += [ti.ins_read(x, a, 0)] * 4 + [ti.ins_read(x, b, 1)] * 3
    rows += [ti.del_read(X_DLEN, 2, 0)] * 4 + [ti.del_read(X_DLEN, 3, 1)] * 3
    rows += [ti.del_read(X_DSAME, 2, 0)] * 4 + [ti.del_read(X_DSAME, 2, 1)] * 3
    rows += [ti.ins_read(X_INSDEL, "AC", 0)] * 4 + [ti.del_read(X_INSDEL, 2, 1)] * 3
    arrs = ti.merged([main, ti.hand_reads(bytes(ref), rows)])
    res, _ = td.oracle_result(oracle_lib, arrs, 50, 2950, bytes(ref), **PER_LIB)
    return bytes(ref), arrs, res


@pytest.mark.parametrize("role", [[CASE, CTL], [CTL, CASE]], ids=["case_control", "control_case"])
def test_two_libraries_per_role_order(route, two_libs, role):
    """the matching control record lies right (case / control) and left (control / case) of the record in the table"""
    from bam_readcount_amd import tensors
    ref, arrs, res = two_libs
    D = tv.Dense.of(res)
    T = Tab.of_oracle(res.indels)
    case = role.index(CASE)
    wf, wv, wc, wk, wst = reference(D, T, role=role, **EASY)
    at = lambda p: [x for x in range(T.m) if T.pos[x] == p and T.lib[x] == case and T.istat[0, x] >= 3]
    assert (wf == 0).any() and ((wf != 0) & (wf < NOT_ASKED)).any()
    for p in (X_SAME, X_DSAME):                              # vetoed by the control's record of the same allele
        assert at(p) and all(wf[x] & BIT["CTL_ALLELE"] and wc[x] >= 3 for x in at(p)), p
    for p in (X_SPELL, X_PREFIX, X_DLEN, X_INSDEL):           # the control has a record of another spelling or length there: no veto
        assert any(T.lib[x] != case for x in range(T.m) if T.pos[x] == p)
        assert at(p) and all(not wf[x] & BIT["CTL_ALLELE"] and wc[x] == 0 for x in at(p)), p
    assert any(wf[x] == 0 for p in (X_SPELL, X_PREFIX, X_DLEN, X_INSDEL) for x in at(p))
    eng = td.computed(route.engine_lib, arrs, 50, 2950, ref, **PER_LIB)
    v, d = ts.views_of(eng)
    t, _ = gathered_table(route, eng, res, "two libraries")
    idx = np.unique(T.pos - D.pos0)
    for thr in (MID, EASY):
        w = check(route, v, d, D, T, idx, None, role, what="two libraries %r" % (role,), **thr)
        check_tensors(route, tensors.vet_indels(eng, route.ivet, t, idx=idx, role=role, **thr), w, "two libraries, tensors")
    assert (w[3] != 0).any() and (w[3] == 0).any()
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. reference buckets in third-allele records

def test_reference_buckets_that_live_in_records_only(route, oracle_lib, monkeypatch):
    """The knob libraries under BRC_FORCE_DOM=3 + BRC_XEV_CAP=1: table records at positions whose reference bucket exists only in a
    third-allele record — and judged without the records they come out otherwise."""
    monkeypatch.setenv("BRC_FORCE_DOM", "3"); monkeypatch.setenv("BRC_XEV_CAP", "1")
    ref, arrs = td.third_allele_inputs()
    opts = dict(PER_LIB, min_bq=10)
    res, _ = td.oracle_result(oracle_lib, arrs, 0, 2000, ref, **opts)
    eng = td.computed(route.knob_lib, arrs, 0, 2000, ref, **opts)
    v, d = ts.views_of(eng)
    assert v.n_xagg > 0
    D = tv.Dense.of(res)
    bare = capi.DeviceView.from_buffer_copy(v); bare.n_xagg = 0
    rc, slots = td.expand(route, bare, 0, res.n_pos, res.n_pos, kinds=("istat",))
    assert rc == 0
    in_slots = slots["istat"].reshape(2, 6, 9, res.n_pos)[:, 1:5, 0, :]
    only_rec = (in_slots != D.istat[:, 1:5, 0, :]) & (D.istat[:, 1:5, 0, :] != 0)
    T = Tab.of_oracle(res.indels)
    k = T.pos - D.pos0
    rbk = D.rb[k]
    hit = [x for x in range(T.m) if rbk[x] >= 0 and only_rec[T.lib[x], rbk[x], k[x]]]
    assert len(hit) >= 3, len(hit)
    t = dict(MID, min_depth=4, min_var_count=1)
    w = check(route, v, d, D, T, np.unique(k), what="records", **t)
    rc, st, gf, gv, gc, gk = call(route, bare, d, T, **t)
    assert rc == 0
    for x in hit[:8]:
        assert not np.array_equal(gv[:, x], w[1].view(np.uint32)[:, x]), x
    eng.close()


def edge_table(D, positions, L, rng, spots=((62, 67), (254, 259)), m=300, role=None):
    """a sorted table of m records whose runs of positions[0], positions[1] lie at the table indices of `spots` — across a wave edge and
    a workgroup edge —, each with every library in it; everywhere else runs of length 1 .. 3"""
    recs = []
    others = [p for p in range(D.n_pos) if p not in positions]
    spot_at = {a: (b, p) for (a, b), p in zip(spots, positions)}
    alleles = ["+A", "+AC", "+AG", "+ACG", "-A", "-AC", "-AG", "-ACG"]
    o = 0
    while len(recs) < m:
        x = len(recs)
        if x in spot_at:
            b, p = spot_at[x]
            for j in range(b - x):
                recs.append((D.pos0 + p, j % L, "+AC" if j < L else "+T" * (j + 1), sums(int(rng.integers(1, 9)))))
            while others[o] <= p:
                o += 1
            continue
        nxt = min([a for a in spot_at if a > x] + [m])
        run = min(int(rng.integers(1, 4)), nxt - x)
        p = others[o]; o += 1
        al = rng.choice(alleles)
        for j in range(run):
            n = int(rng.integers(1, 12))
            recs.append((D.pos0 + p, j % L, al if j < L else al + "T" * j,
                         sums(n, plus=int(rng.integers(0, n + 1)), smq=int(rng.integers(0, 61)) * n, smmq=int(rng.integers(0, 90)) * n,
                              sclip=int(rng.integers(40, 152)) * n, nq2=min(n, 2), f=tuple((rng.random(4) * n).astype(np.float32)))))
    recs = recs[:m]
    keys = [(r[0],) for r in recs]
    assert keys == sorted(keys)
    return Tab.of(recs)


def test_two_records_of_one_position_in_different_libraries(route):
    """test_vet's hand-made view: positions 130 and 330 each with third-allele records of two libraries, the reference's bucket among
    them; their table runs lie across a wave edge (records 62 - 66) and a workgroup edge (254 - 258)"""
    v, d, D, keep, _ = tv.two_record_views(route)
    assert v.n_xagg >= 4
    rng = np.random.default_rng(5)
    T = edge_table(D, (130, 330), 2, rng)
    assert (T.pos[62:67] == 130).all() and (T.pos[254:259] == 330).all() and T.pos[61] != 130 and T.pos[67] != 130
    for role in ([CASE, CTL], [CTL, CASE], None):
        w = check(route, v, d, D, T, np.unique(T.pos), None, role, what="two records %r" % (role,), **MID)
    bare = capi.DeviceView.from_buffer_copy(v); bare.n_xagg = 0
    rc, st, gf, gv, gc, gk = call(route, bare, d, T, **MID)
    differ = [x for x in list(range(62, 67)) + list(range(254, 259)) if not np.array_equal(gv[:, x], w[1].view(np.uint32)[:, x])]
    assert len(differ) >= 2, differ                          # (library 1 at 130, library 0 at 330: the reference bucket is a record's)


# ------------------------------------------------------------------------------------------------ 3. table shapes

def shape_views(route, records=True, L=3):
    depth, istat, fstat, ref = tv.random_sums(700, L=L, seed=6, third=0.3 if records else 0.0)
    if not records:
        full = istat[:, 1:5, 0] != 0
        extra = np.cumsum(full, axis=1) > 2
        istat[:, 1:5][np.broadcast_to(extra[:, :, None, :], istat[:, 1:5].shape)] = 0
        fstat[:, 1:5][np.broadcast_to(extra[:, :, None, :], fstat[:, 1:5].shape)] = 0
    return tv.full_views(route, depth, istat, fstat, ref, pos0=1000, ref_lo=1000)


def random_table(D, m, rng, L, spread=3):
    """m records sorted by (pos, lib, text): runs of 1 .. 6 records over few alleles, so that control records of the same allele, of
    another spelling and of another length all occur"""
    alleles = ["+A", "+AC", "+AG", "+ACG", "-A", "-AC", "-AG", "-ACG"]
    keys = set()
    positions = rng.choice(D.n_pos, size=max(m // spread, 1), replace=False) if m else []
    while len(keys) < m:
        keys.add((D.pos0 + int(rng.choice(positions)), int(rng.integers(0, L)), alleles[int(rng.integers(0, 4)) + 4 * int(rng.random() < 0.3)]))
    recs = []
    for p, l, a in sorted(keys):
        n = int(rng.integers(0, 14))
        recs.append((p, l, a, sums(n, plus=int(rng.integers(0, n + 1)), smq=int(rng.integers(0, 61)) * n, sse=int(rng.integers(0, 30)) * n, nq2=min(n, int(rng.integers(0, 3))),
                                   smmq=int(rng.integers(0, 90)) * n, sclip=int(rng.integers(40, 152)) * n, f=tuple((rng.random(4) * n).astype(np.float32)))))
    return Tab.of(recs)


ROLE3 = [CASE, CTL, CTL]


def test_table_lengths_and_the_workspace(route):
    """m = 0, 1, 63, 64, 65, 256, 257 on a view with third-allele records and on one without (no link launch, a scratch of 0 bytes)"""
    rng = np.random.default_rng(3)
    for records in (True, False):
        v, d, D, keep = shape_views(route, records)
        assert bool(v.n_xagg) == records
        seen = 0
        for m in (0, 1, 63, 64, 65, 256, 257):
            assert route.ivet.workspace(v, m) == (4 * (m + v.n_xagg) if records and m else 0)
            T = random_table(D, m, rng, 3)
            idx = np.unique(T.pos - D.pos0)
            for role in (ROLE3, [CTL, CASE, CASE]):
                w = check(route, v, d, D, T, idx, None, role, what="m = %d" % m, **MID)
                seen |= bits_seen(w[0])
        assert seen & BIT["CTL_ALLELE"] and seen & BIT["CTL_DEPTH"] and bin(seen).count("1") >= 8, hex(seen)
    assert route.ivet.workspace(None, 5) == 0


def test_runs_across_a_wave_edge_and_a_workgroup_edge_and_runs_of_one(route):
    v, d, D, keep = shape_views(route, L=3)
    rng = np.random.default_rng(9)
    T = edge_table(D, (130, 330), 3, rng)
    for role in (ROLE3, [CTL, CTL, CASE], [CTL, CASE, IGN]):
        wf, wv, wc, wk, _ = check(route, v, d, D, T, np.unique(T.pos - D.pos0), None, role, what="edges %r" % (role,), **T_(ctl_max_count=0))
        case = [x for x in list(range(62, 67)) + list(range(254, 259)) if wf[x] < NOT_ASKED]
        assert any(wf[x] & BIT["CTL_ALLELE"] for x in case) and any(wc[x] for x in case), role
    # a stride of its own: istat / fstat planes wider than m
    check(route, v, d, D, T, what="stride", stride=T.m + 5, **MID)
    ones = Tab.of([(D.pos0 + p, p % 3, "+AC", sums(5)) for p in range(0, 600, 2)])
    w = check(route, v, d, D, ones, role=ROLE3, what="runs of one", **T_(ctl_max_count=0))
    assert not (w[0] & BIT["CTL_ALLELE"]).any() and not w[2].any()


# ------------------------------------------------------------------------------------------------ 4. allele matching

def flat_views(route, P=48, L=4, depth=30, cref=20, ctl_depth=None):
    """reference A everywhere, its bucket of cref reads in every library, depth `depth` (ctl_depth: per-library overrides)"""
    istat = np.zeros((L, 6, 9, P), np.uint32); fstat = np.zeros((L, 6, 4, P), np.float32)
    istat[:, 1, 0] = cref; istat[:, 1, 3] = cref // 2; istat[:, 1, 4] = cref - cref // 2; istat[:, 1, 1] = cref * 60; istat[:, 1, 7] = cref * 100
    dep = np.full((L, P), depth, np.uint32)
    for l, x in (ctl_depth or {}).items():
        dep[l] = x
    return tv.full_views(route, dep, istat, fstat, b"A" * P)


ROLE4 = [CASE, CTL, CTL, IGN]
# position -> (the case record's text, its len or None, [(library, text, len or None, count)] of the other records, vetoed, ctl_count) under ctl_max_count = 1
MATCH = [
    (1, "+AC", None, [(1, "+AC", None, 2)], True, 2),                       # same length, same spelling
    (2, "+AC", None, [(1, "+AG", None, 2)], False, 0),                      # same length, other spelling
    (3, "+AC", None, [(1, "+ACG", None, 2)], False, 0),                     # a prefix
    (4, "+ACG", None, [(1, "+AC", None, 2)], False, 0),                     # ... and the longer one as the case
    (5, "-AC", None, [(1, "-AC", None, 2)], True, 2),                       # a deletion of the same length
    (6, "-AC", None, [(1, "-ACG", None, 2)], False, 0),                     # ... of another length
    (7, "+AC", None, [(1, "+AC", -2, 2)], False, 0),                        # an insertion against a deletion: the same bytes, another len
    (8, "+AC", None, [(1, "-AC", None, 2)], False, 0),                      # ... and as a gathered table spells it
    (9, "+AC", None, [(1, "+AC", None, 1), (2, "+AC", None, 5)], True, 5),  # two control libraries, only one of which fails
    (10, "+AC", None, [(1, "+AC", None, 1), (2, "+AC", None, 1)], False, 1),
    (11, "+AC", None, [], False, 0),                                        # control libraries without any record
    (12, "+AC", None, [(3, "+AC", None, 9)], False, 0),                     # an ignored library's record of the same allele
    (13, "+AC", None, [(1, "+AC", None, 1)], False, 1),                     # ctl_max_count met exactly (and exceeded by one at position 1)
    (14, "+AC", None, [(1, "+AC", None, 2), (1, "+AG", None, 7), (2, "+AC", None, 7), (2, "+ACG", None, 9)], True, 7),    # several matching records
    (15, "+AC", 2, [(1, "+AC", 3, 2)], False, 0),                           # same text, another (inconsistent) len
]


def match_table(cases=MATCH):
    recs = []
    for p, text, ln, others, _, _ in cases:
        rows = [(p, 0, text, sums(6)) + (() if ln is None else (ln,))]
        rows += [(p, l, t, sums(c)) + (() if n is None else (n,)) for l, t, n, c in others]
        recs += sorted(rows, key=lambda r: (r[1], r[2]))
    return Tab.of(recs)


def test_allele_matching(route):
    v, d, D, keep = flat_views(route)
    T = match_table()
    t = T_(ctl_max_count=1)
    wf, wv, wc, wk, _ = check(route, v, d, D, T, role=ROLE4, what="matching", **t)
    for p, text, ln, others, veto, count in MATCH:
        x = [x for x in range(T.m) if T.pos[x] == p and T.lib[x] == 0][0]
        assert bool(wf[x] & BIT["CTL_ALLELE"]) == veto and wc[x] == count, (p, hex(wf[x]), wc[x])
        assert wf[x] in (0, BIT["CTL_ALLELE"])
    assert all(f == NOT_ASKED for f, l in zip(wf, T.lib) if l != 0)
    # one test alone sets only its own bit, and without it the bit is never set; ctl_count does not depend on `tests`
    only = check(route, v, d, D, T, role=ROLE4, tests=BIT["CTL_ALLELE"], what="CTL_ALLELE alone", **dict(MID, ctl_max_count=1, ctl_frac_num=U32, ctl_frac_den=1))
    assert bits_seen(only[0]) == BIT["CTL_ALLELE"] and np.array_equal(only[2], wc)
    rest = check(route, v, d, D, T, role=ROLE4, tests=ALL_TESTS & ~BIT["CTL_ALLELE"], what="all but CTL_ALLELE", **t)
    assert not bits_seen(rest[0]) & BIT["CTL_ALLELE"] and np.array_equal(rest[2], wc)
    # with the roles the other way round the records of library 1 are judged against library 0's
    w2 = check(route, v, d, D, T, role=[CTL, CASE, IGN, IGN], what="roles swapped", **T_(ctl_max_count=5))
    x = [x for x in range(T.m) if T.pos[x] == 1 and T.lib[x] == 1][0]
    assert w2[0][x] == BIT["CTL_ALLELE"] and w2[2][x] == 6
    # without the allele arrays: allowed when CTL_ALLELE is not asked; ctl_count is then 0
    w3 = check(route, v, d, D, T, role=ROLE4, tests=ALL_TESTS & ~BIT["CTL_ALLELE"], what="no text", with_text=False, **t)
    assert not w3[2].any()


def test_the_control_fraction_and_the_control_depth_at_their_thresholds(route):
    v, d, D, keep = flat_views(route, ctl_depth={2: 29})
    T = Tab.of([(p, l, "+AC", sums(c)) for p, c in ((1, 3), (2, 4)) for l in (0, 1)])
    t = T_(ctl_frac_num=1, ctl_frac_den=10)                  # depth 30: 3 * 10 <= 30 holds, 4 * 10 <= 30 does not
    wf, _, wc, _, _ = check(route, v, d, D, T, role=[CASE, CTL, IGN, IGN], what="fraction", **t)
    assert wf[0] == 0 and wf[2] == BIT["CTL_ALLELE"] and list(wc[[0, 2]]) == [3, 4]
    for ctl_min_depth, role, want in ((30, [CASE, CTL, IGN, IGN], 0), (31, [CASE, CTL, IGN, IGN], BIT["CTL_DEPTH"]), (30, [CASE, CTL, CTL, IGN], BIT["CTL_DEPTH"]),
                                      (29, [CASE, CTL, CTL, IGN], 0), (31, [CASE, IGN, IGN, IGN], 0)):
        wf, _, _, _, _ = check(route, v, d, D, T, role=role, what="ctl_min_depth %d" % ctl_min_depth, **T_(ctl_min_depth=ctl_min_depth))
        assert wf[0] == want, (ctl_min_depth, role, hex(wf[0]))
        only = check(route, v, d, D, T, role=role, tests=BIT["CTL_DEPTH"], what="CTL_DEPTH alone", **dict(MID, ctl_min_depth=ctl_min_depth))
        assert bits_seen(only[0]) == want


def test_control_counts_and_depths_next_to_two_to_the_32(sim_route):
    """host views, CPU build: a product that a 32-bit multiplication decides otherwise"""
    route = sim_route
    v, d, D, keep = flat_views(route, L=2, ctl_depth={1: U32})
    T = Tab.of([(1, 0, "+AC", sums(6)), (1, 1, "+AC", sums(3)), (2, 0, "+AC", sums(6)), (2, 1, "+AC", sums(U32, plus=7, smq=5, sclip=5)),
                (3, 0, "+AC", sums(6)), (3, 1, "+AC", sums(2 ** 31 + 1, plus=7, smq=5, sclip=5))])
    t = T_(ctl_frac_num=1, ctl_frac_den=2 ** 31)             # 3 * 2^31 > 2^32 - 1, but (3 * 2^31) mod 2^32 = 2^31 is below it
    def wrapped(C, depth, t):
        """the control test's verdict (True: vetoed) with both products taken modulo 2^32"""
        return not (C <= t["ctl_max_count"] and (C * t["ctl_frac_den"]) & U32 <= (t["ctl_frac_num"] * depth) & U32)
    wf, _, wc, _, _ = check(route, v, d, D, T, role=[CASE, CTL], what="2^32", **t)
    assert wf[0] == BIT["CTL_ALLELE"] and not wrapped(3, U32, t)             # a 32-bit product decides otherwise
    assert list(wc[[0, 2, 4]]) == [3, U32, 2 ** 31 + 1]
    wf, _, _, _, _ = check(route, v, d, D, T, role=[CASE, CTL], what="2^32, max count", **T_(ctl_max_count=U32 - 1, ctl_frac_num=U32, ctl_frac_den=1))
    assert wf[2] == BIT["CTL_ALLELE"] and wf[4] == 0         # U32 > U32 - 1; (2^31 + 1) * 1 <= U32 * U32
    wf, _, wc, _, _ = check(route, v, d, D, T, role=[CASE, CTL], what="2^32, max count met exactly", **T_(ctl_max_count=U32, ctl_frac_num=U32, ctl_frac_den=1))
    assert wf[2] == 0 and wc[2] == U32                       # U32 <= U32: a count of 2^32 - 1 under a limit of 2^32 - 1 passes
    t = T_(ctl_frac_num=2, ctl_frac_den=U32)
    wf, _, _, _, _ = check(route, v, d, D, T, role=[CASE, CTL], what="2^32, fraction", **t)
    assert wf[0] == BIT["CTL_ALLELE"] and not wrapped(3, U32, t)             # 3 * U32 > 2 * U32; in 32 bits 3 * U32 = U32 - 2 <= 2 * U32 = U32 - 1


# ------------------------------------------------------------------------------------------------ 5. the inherited tests

def metric_views(route, P=120):
    """one library, reference A with sums whose quotients are no short decimals; a table of one insertion per position with such sums
    too, and handmade_views.FLOATS among the float sums"""
    rng = np.random.default_rng(12)
    istat = np.zeros((1, 6, 9, P), np.uint32); fstat = np.zeros((1, 6, 4, P), np.float32)
    c = rng.integers(1, 24, P)
    istat[0, 1, 0] = c; istat[0, 1, 3] = c // 2; istat[0, 1, 4] = c - c // 2
    for f in (1, 2, 5, 6, 7, 8):
        istat[0, 1, f] = rng.integers(1, 4000, P)
    istat[0, 1, 5] = np.minimum(istat[0, 1, 5], c)
    fstat[0, 1] = (rng.random((4, P)) * c + 0.01).astype(np.float32)
    depth = istat[:, 1:5, 0].sum(axis=1) + 7
    v, d, D, keep = tv.full_views(route, depth, istat, fstat, b"A" * P)
    recs = []
    floats = np.array(hv.FLOATS, np.uint32).view(np.float32)
    for p in range(P):
        n = int(rng.integers(1, 24))
        f = (rng.random(4) * n + 0.01).astype(np.float32)
        if p >= P - 24:
            f[(p // 6) % 4] = floats[p % 6]
        recs.append((p, 0, "+" + "ACGT"[p % 4], sums(n, plus=int(rng.integers(0, n + 1)), smq=int(rng.integers(1, 4000)), sse=int(rng.integers(0, 4000)),
                                                    nq2=min(n, 2), smmq=int(rng.integers(1, 4000)), sclip=int(rng.integers(1, 4000)), f=tuple(f))))
    return v, d, D, keep, Tab.of(recs)


FP_TESTS = [x for x in tv.FP_TESTS if x[0] != "VAR_BQ"]


def test_every_fp32_test_at_its_threshold_and_one_ulp_beside(route):
    v, d, D, keep, T = metric_views(route)
    mv = ti.metrics_of(T.istat, T.fstat)
    for name, key, c, side, sign in FP_TESTS:
        for k in (7, 50, 93):
            a = mv[MCOL[c], k] if side == "v" else D.metrics[0, 1, MCOL[c], k]
            assert a > 0
            got = []
            for thr in (np.nextafter(a, F32(-np.inf)), a, np.nextafter(a, F32(np.inf))):
                wf, _, _, _, _ = check(route, v, d, D, T, tests=BIT[name], what="%s at %r" % (name, thr), want=("fail",), **T_(**{key: float(thr)}))
                got.append(bool(wf[k] & BIT[name]))
                assert not (wf & ~np.uint32(BIT[name])).any()
            assert got == ([False, False, True] if sign < 0 else [True, False, False]), (name, k, got)
    # every value of handmade_views.FLOATS in a float sum: the bits of vals are numpy's, NaN and infinities included
    w = check(route, v, d, D, T, what="FLOATS", **MID)
    assert not np.isfinite(w[1][:, -24:]).all()


def test_the_three_differences_at_their_thresholds(route):
    v, d, D, keep, T = metric_views(route)
    mv, mr = ti.metrics_of(T.istat, T.fstat), D.metrics[0, 1]
    for name, key, dv in (("MMQS_DIFF", "max_mmqs_diff", mv[8] - mr[8]), ("MAPQ_DIFF", "max_mapq_diff", mr[1] - mv[1])):
        assert dv.dtype == np.float32
        for k in (3, 77):
            got = []
            for thr in (np.nextafter(dv[k], F32(-np.inf)), dv[k], np.nextafter(dv[k], F32(np.inf))):
                wf, _, _, _, _ = check(route, v, d, D, T, tests=BIT[name], what="%s at %r" % (name, thr), want=("fail", "vals"), **T_(**{key: float(thr)}))
                got.append(bool(wf[k] & BIT[name]))
            assert got == [True, False, False], (name, k, got)
    d_rl = mr[11] - mv[11]
    done = 0
    for k in range(T.m):
        if not (mr[11][k] > 0 and d_rl[k] > 0):
            continue
        fr = F32(d_rl[k] / mr[11][k])
        got = []
        for thr in (np.nextafter(fr, F32(-np.inf)), fr, np.nextafter(fr, F32(np.inf))):
            wf, wv, _, _, _ = check(route, v, d, D, T, tests=BIT["RL_DIFF"], what="RL_DIFF at %d" % k, want=("fail", "vals"), **T_(max_rl_diff=float(thr)))
            got.append(bool(wf[k] & BIT["RL_DIFF"]))
            assert bool(wf[k]) == bool(d_rl[k] > F32(thr) * mr[11][k])
        assert got[0] or not got[2]
        done += 1
        if done == 3:
            break
    assert done == 3


def test_integer_tests_met_exactly_and_the_judged_only_when_conditions(route):
    P = 64
    istat = np.zeros((1, 6, 9, P), np.uint32); fstat = np.zeros((1, 6, 4, P), np.float32)
    k = np.arange(P)
    istat[0, 1, 0] = 20; istat[0, 1, 3] = 10; istat[0, 1, 4] = 10; istat[0, 1, 1] = 20 * 60
    depth = ((20 + k % 8) * (k >= 8)).astype(np.uint32)[None, :]                       # D == 0 on the first eight positions
    v, d, D, keep = tv.full_views(route, depth, istat, fstat, b"A" * P)
    T = Tab.of([(p, 0, "+AC", sums(p % 8, plus=(p % 8) // 4, smq=(p % 8) * 10)) for p in range(P)])
    t = T_(min_depth=24, min_var_count=4, freq_num=1, freq_den=6, min_strand_reads=4, strand_num=1, strand_den=4, min_ref_reads=21, min_var_mapq=11.0,
           min_ref_mapq=61.0, max_mapq_diff=49.0)
    f, wv, _, _, _ = check(route, v, d, D, T, what="integers", **t)
    assert not f[12] & BIT["DEPTH"] and f[11] & BIT["DEPTH"]                          # D = 24 / 23 against 24
    assert not f[12] & BIT["VAR_COUNT"] and f[11] & BIT["VAR_COUNT"]
    assert not f[12] & BIT["VAR_FREQ"] and f[11] & BIT["VAR_FREQ"]                    # 4 * 6 = 24 * 1; 3 * 6 < 23
    assert not f[12] & BIT["STRAND"] and f[13] & BIT["STRAND"] and not f[11] & BIT["STRAND"]        # 1 * 4 = 4; 1 * 4 < 5; 3 reads: not judged
    assert f[16] == (BIT["DEPTH"] | BIT["VAR_COUNT"] | BIT["VAR_FREQ"])                # C_v == 0: no variant-side fp32 test, no difference
    assert f[12] & BIT["VAR_MAPQ"] and not f[12] & (BIT["REF_MAPQ"] | BIT["MAPQ_DIFF"])  # C_r = 20 < min_ref_reads: the reference side is not judged
    assert not wv[3, :8].any() and not wv[2, :8].any()
    assert (f[:8] & BIT["DEPTH"]).all() and not (f[1:8] & BIT["VAR_FREQ"]).any()       # D == 0: frequency 0 in vals
    f2, _, _, _, _ = check(route, v, d, D, T, what="reference judged", **dict(t, min_ref_reads=20))
    assert f2[12] & BIT["REF_MAPQ"] and f2[12] & BIT["MAPQ_DIFF"]
    assert not (wv[10] != 0).any()                                                       # the variant's AVG_BQ column is 0


def test_each_test_alone_sets_only_its_own_bit(route):
    v, d, D, keep = shape_views(route)
    T = random_table(D, 300, np.random.default_rng(8), 3)
    full = reference(D, T, role=ROLE3, **MID)[0]
    assert bits_seen(full) == ALL_TESTS, "the thresholds leave a test that never fails: %x" % (ALL_TESTS & ~bits_seen(full))
    for name in capi.IVET_TESTS:
        w = check(route, v, d, D, T, role=ROLE3, tests=BIT[name], what=name, want=("fail", "ctl_count"), **MID)
        assert bits_seen(w[0]) == BIT[name]
    w = check(route, v, d, D, T, role=ROLE3, tests=0, what="no test", **MID)
    assert bits_seen(w[0]) == 0


# ------------------------------------------------------------------------------------------------ 6. records that are not judged

def test_records_that_are_not_judged(route):
    v, d, D, keep = shape_views(route)
    p0, P = D.pos0, D.n_pos
    s = sums(6)
    T = Tab.of([(p0 - 1, 0, "+AC", s), (p0 - 1, 1, "", s, 0), (p0, 0, "+AC", s), (p0 + 5, -1, "+AC", s), (p0 + 5, 0, "", s, 0), (p0 + 5, 0, "+AC", s),
                (p0 + 5, 0, "-AC", s), (p0 + 5, 1, "+AC", s), (p0 + 5, 3, "+AC", s), (p0 + P - 1, 2, "-A", s), (p0 + P, 0, "+AC", s), (2 ** 31 - 1, 0, "+A", s)])
    idx = [0, 5, P - 1]
    wf, wv, wc, wk, st = check(route, v, d, D, T, idx, role=ROLE3, what="not judged", **T_(ctl_max_count=0))
    assert st == capi.IVET_TABLE_OUT_OF_RANGE
    assert list(wf[[0, 1, 3, 4, 7, 8, 10, 11]]) == [NO_SITE, NOT_ASKED, NO_SITE, NOT_ASKED, NOT_ASKED, NO_SITE, NO_SITE, NO_SITE]
    assert wf[5] == BIT["CTL_ALLELE"] and wf[6] == 0 and wf[2] == 0 and not wv[:, [0, 1, 3, 4, 7, 8, 10, 11]].any() and not wc[[0, 1, 3, 4, 7, 8]].any()
    assert list(wk) == [INS, DEL, 0]                         # (library 2 is a control library: its record at the last position is not asked)
    # a len of 0 outside the planes is not asked and sets no status bit
    w = check(route, v, d, D, Tab.of([(p0 - 5, 7, "", s, 0)]), what="len 0 outside", **OPEN)
    assert w[4] == 0 and w[0][0] == NOT_ASKED
    # kinds of one kind only; roles of ignore / control on the record's own library
    for kinds, want in ((INS, [0, NOT_ASKED]), (DEL, [NOT_ASKED, 0])):
        w = check(route, v, d, D, T, idx, kinds=kinds, what="kinds %d" % kinds, **OPEN)
        assert list(w[0][[5, 6]]) == want and list(w[3][:2]) == ([INS, INS] if kinds == INS else [0, DEL])
    for role in ([IGN, CASE, CASE], [CTL, CASE, CASE]):
        w = check(route, v, d, D, T, idx, role=role, what="role %r" % (role,), **OPEN)
        assert list(w[0][[2, 5, 6]]) == [NOT_ASKED] * 3 and w[0][7] == 0


def test_reference_characters_and_slices(route):
    kinds = set()
    for what, (v, d, h, keepalive), _ in ts.refchar_views(route):
        kinds.add((bool(d.ref), d.ref_lo > d.pos0, d.ref_hi < d.pos0 + d.n_pos, d.ref_len < d.ref_hi))
        D = tv.Dense.of_counts(h)
        T = Tab.of([(D.pos0 + p, 0, "+AC", sums(5)) for p in range(D.n_pos)])
        wf, _, _, wk, _ = check(route, v, d, D, T, np.arange(D.n_pos), what=what, **T_(min_var_count=2))
        assert np.array_equal(wf == NO_SITE, D.rb < 0) and np.array_equal(wk != 0, D.rb >= 0)
        if what == "characters":
            assert (wf[:32] == 0).all() and (wf[32:] == NO_SITE).all()                  # ACGTacgt, four positions each
        if what == "no reference":
            assert not d.ref and (wf == NO_SITE).all() and not wk.any()
    assert len(kinds) >= 5


# ------------------------------------------------------------------------------------------------ 7. broken tables

def test_an_unsorted_table_and_broken_offsets(route):
    v, d, D, keep = shape_views(route, records=False)        # (no third-allele records: every bucket is exact on any table)
    rng = np.random.default_rng(14)
    T = random_table(D, 200, rng, 3)
    cut = 100
    while T.pos[cut] == T.pos[cut - 1]:
        cut += 1
    U = T.take(list(range(cut, 200)) + list(range(cut)))      # one descent in pos, at 200 - cut
    assert ((U.pos[1:] < U.pos[:-1]).sum()) == 1
    w = check(route, v, d, D, U, np.unique(U.pos - D.pos0), None, ROLE3, what="unsorted", **MID)
    assert w[4] == capi.IVET_TABLE_NOT_ASCENDING
    # a position whose records lie in two stretches: each stretch is a run of its own
    V = Tab.of([(D.pos0 + 9, 0, "+AC", sums(6)), (D.pos0 + 3, 1, "+AC", sums(6)), (D.pos0 + 9, 1, "+AC", sums(6)), (D.pos0 + 9, 0, "+AG", sums(6))])
    w = check(route, v, d, D, V, role=ROLE3, what="two stretches", **T_(ctl_max_count=0))
    assert w[0][0] == 0 and w[2][0] == 0 and w[4] == capi.IVET_TABLE_NOT_ASCENDING
    # offsets above alleles_len, and a descending pair: text() clamps, nothing is read outside alleles
    B = Tab(T.pos, T.lib, T.len, T.istat, T.fstat, T.off.copy(), T.alleles)
    B.off[40] = B.alleles.size + 1000; B.off[41] = 0xFFFFFFFF; B.off[90] = B.off[88]; B.off[120] = 0
    assert (B.off[1:] < B.off[:-1]).any() and (B.off > B.alleles.size).any()
    check(route, v, d, D, B, np.unique(B.pos - D.pos0), None, ROLE3, what="broken offsets", **MID)


def unsorted_over_records(D):
    """a table with one descent over test_vet's two-record view: the run of position 130 (whose reference bucket, A, is a third-allele
    record's in library 1), one record behind it, then two records of a lower position q whose reference is A too — the binary search of
    the last of them over the records before it ends at index 0, the head of position 130's list"""
    q = [k for k in range(5, 100) if D.refbase[k:k + 1] == b"A" and D.istat[1, 1, 0, k]][0]
    s = sums(6)
    return q, Tab.of([(130, 0, "+AC", s), (130, 1, "+AC", s), (130, 1, "+AG", s), (131, 1, "+AC", s), (q, 0, "+AC", s), (q, 1, "+AC", s)])


def test_an_unsorted_table_over_third_allele_records(route):
    """a record takes a list of third-allele records only from a table record of its own position: the records of the lower position
    are exact, those of position 130 are judged on the slots' values or on their position's record, every store stays in range"""
    v, d, D, keep, _ = tv.two_record_views(route)
    q, T = unsorted_over_records(D)
    assert v.n_xagg >= 4 and (T.pos[1:] < T.pos[:-1]).sum() == 1
    wf, wv, wc, wk, wst = reference(D, T, [q, 130], **MID)
    rc, st, gf, gv, gc, gk = call(route, v, d, T, [q, 130], **MID)
    assert rc == 0 and st == wst == capi.IVET_TABLE_NOT_ASCENDING
    assert untouched(gf[T.m:], gv[:, T.m:], gc[T.m:], gk[2:])
    assert np.array_equal(gf[3:6], wf[3:]) and np.array_equal(gv[:, 3:6], wv.view(np.uint32)[:, 3:]) and np.array_equal(gc[:T.m], wc)
    bare = capi.DeviceView.from_buffer_copy(v); bare.n_xagg = 0
    _, _, bf, bv, _, _ = call(route, bare, d, T, [q, 130], **MID)
    assert not np.array_equal(bv[:, 1], wv.view(np.uint32)[:, 1])              # (library 1 at 130: the record matters)
    for x in range(3):
        assert np.array_equal(gv[:, x], wv.view(np.uint32)[:, x]) or np.array_equal(gv[:, x], bv[:, x]), x
    # ... and sorted, the same records are all exact
    check(route, v, d, D, T.take([4, 5, 0, 1, 2, 3]), [q, 130], what="sorted", **MID)


# ------------------------------------------------------------------------------------------------ 8. the list

def test_lists(route):
    v, d, D, keep = shape_views(route)
    rng = np.random.default_rng(15)
    T = random_table(D, 300, rng, 3, spread=2)
    have = np.unique(T.pos - D.pos0)
    P = D.n_pos
    t = T_(min_var_count=5)
    for n in (0, 1, 64, 65):
        idx = np.sort(rng.choice(have, n, replace=False)) if n else []
        w = check(route, v, d, D, T, idx, what="n = %d" % n, **t)
    assert (w[3] != 0).any() and (w[3] == 0).any()
    # equal neighbours across a wave edge, elements without records, elements out of range at both ends
    idx = np.concatenate([[-5, -1], np.sort(rng.choice(have[30], 60, replace=False)), [have[30]] * 5, have[31:60], [P, P + 9]])
    assert (idx[62:67] == have[30]).all() and (np.diff(idx) >= 0).all()
    why = rng.integers(0, 64, idx.size)
    w = check(route, v, d, D, T, idx, what="why NULL", **t)
    assert w[4] == capi.IVET_LIST_OUT_OF_RANGE and len(set(w[3][62:67])) == 1 and not w[3][[0, 1, -1, -2]].any()
    assert not w[3][2:62][~np.isin(idx[2:62], have)].any()
    check(route, v, d, D, T, idx, why, what="why", **t)
    wi = check(route, v, d, D, T, idx, np.full(idx.size, INS), what="why INS", **t)
    assert not (wi[3] & DEL).any() and (w[3] & DEL).any()
    ws = check(route, v, d, D, T, idx, np.full(idx.size, 15), what="why with SNV bits only", **t)
    assert not ws[3].any()
    # a descent: the status bit, every store in range
    bad = np.concatenate([have[20:40], have[:20]])
    rc, st, gf, gv, gc, gk = call(route, v, d, T, bad, **t)
    assert rc == 0 and st == capi.IVET_LIST_NOT_ASCENDING and untouched(gk[bad.size:]) and not (gk[:bad.size] & ~np.uint32(INS | DEL)).any()
    assert np.array_equal(gf[:T.m], w[0])
    # every destination alone, keep among them; none at all
    for want in (("keep",), ("fail",), ("vals",), ("ctl_count",), ("fail", "keep"), ()):
        check(route, v, d, D, T, idx, why, ROLE3, what="want %r" % (want,), want=want, **MID)
    rc, st, gf, gv, gc, gk = call(route, v, d, T, idx, want=(), status=False, **MID)
    assert rc == 0 and st == SENT and untouched(gf, gv, gc, gk)
    # a list over an empty table: keep is cleared, the list is judged
    w = check(route, v, d, D, Tab.of([]), idx, what="m = 0 with a list", **t)
    assert not w[3].any() and w[4] == capi.IVET_LIST_OUT_OF_RANGE


# ------------------------------------------------------------------------------------------------ 9. the contract

def test_two_calls_are_byte_identical(route):
    v, d, D, keep = shape_views(route)
    T = random_table(D, 300, np.random.default_rng(16), 3)
    idx = np.unique(T.pos - D.pos0)
    a = call(route, v, d, T, idx, role=ROLE3, **MID); b = call(route, v, d, T, idx, role=ROLE3, **MID)
    assert a[0] == b[0] == 0 and all(x.tobytes() == y.tobytes() for x, y in zip(a[2:], b[2:]))
    t = route.ivet.last_timing()
    assert t["kernel_s"] > 0 and t["bytes_read"] >= 4 * 300 * (4 + 13 + 28) and t["bytes_written"] >= 4 * (300 * (2 + NVAL) + idx.size)


def lib254_views(route):
    depth, cnt, ref = ts.low_depth(70, L=254, seed=3, alt=0.1)
    istat = np.zeros((254, 6, 9, 70), np.uint32)
    istat[:, 1:5, 0] = cnt; istat[:, 1:5, 3] = cnt // 2; istat[:, 1:5, 4] = cnt - cnt // 2
    istat[:, 1:5, 1] = cnt * (np.arange(254) % 60)[:, None, None]
    return tv.full_views(route, depth, istat, np.zeros((254, 6, 4, 70), np.float32), ref)


def test_254_libraries_with_alternating_roles(route):
    v, d, D, keep = lib254_views(route)
    assert v.n_lib == 254 and v.n_xagg > 0
    role = [CASE if l % 2 else CTL for l in range(254)]
    T = Tab.of([(p, l, "+AC" if (l // 2) % 3 else "+AG", sums(1 + (l + p) % 5)) for p in (3, 40) for l in range(254)] + [(50, 253, "+A", sums(4))])
    t = T_(min_depth=4, min_var_count=2, min_var_mapq=20.0, min_ref_mapq=30.0, min_ref_reads=1, ctl_max_count=4, ctl_min_depth=2)
    wf, _, wc, wk, _ = check(route, v, d, D, T, [3, 40, 50], None, role, what="254 libraries", **t)
    judged = wf[1:508:2] < NOT_ASKED
    assert (wf[0:508:2] == NOT_ASKED).all() and judged.any() and (wf[1:508:2][judged] & BIT["CTL_ALLELE"]).all() and (wc[1:508:2][judged] == 5).all()
    check(route, v, d, D, T, what="254 libraries, all case", **t)
    v2 = capi.DeviceView.from_buffer_copy(v); d2 = capi.DeviceIndels.from_buffer_copy(d); v2.n_lib = d2.n_lib = 255
    rc, st, gf, gv, gc, gk = call(route, v2, d2, T, **t)
    assert rc == capi.E_ARG and st == SENT and untouched(gf, gv, gc, gk)


# ------------------------------------------------------------------------------------------------ 9b. what a mutation pass of the core left standing

def test_roles_above_the_first_role_words(route):
    """254 libraries with the roles of test_select.lib_pattern(3) (ignore / case / control; no copy of itself 16 .. 128 libraries
    further).  Position 3: every library has a record of +AC and ONE control library above 127 — whose role 128 libraries below is not
    control — has more reads than ctl_max_count: it alone vetoes.  Position 40: records of the case libraries, and one such control
    library alone is shallower than ctl_min_depth.  A role table indexed modulo 16 .. 128 libraries gives other words — asserted on
    the reference's side."""
    L = 254
    role = ts.lib_pattern(3)
    assert (IGN, CASE, CTL) == (0, 1, 2)
    high = [l for l in range(128, L) if role[l] == CTL and role[l - 128] != CTL]
    cv, cd = high[0], high[-1]
    assert cv != cd
    shallow = np.full(48, 30, np.uint32); shallow[40] = 1
    v, d, D, keep = flat_views(route, L=L, ctl_depth={cd: shallow})
    T = Tab.of([(3, l, "+AC", sums(9 if l == cv else 2)) for l in range(L)] + [(40, l, "-AC", sums(4)) for l in range(L) if role[l] == CASE])
    t = T_(ctl_max_count=2, ctl_min_depth=2)
    wf, wv, wc, wk, _ = check(route, v, d, D, T, [3, 40], None, role, what="role pattern", **t)
    case = np.array([role[l] == CASE for l in T.lib])
    assert (wf[~case] == NOT_ASKED).all() and (wf[case & (T.pos == 3)] == BIT["CTL_ALLELE"]).all() and (wc[case & (T.pos == 3)] == 9).all()
    assert (wf[case & (T.pos == 40)] == BIT["CTL_DEPTH"]).all() and not wk.any()
    for period in (16, 32, 64, 128):
        other = reference(D, T, [3, 40], None, ts.folded(role, period), **t)
        assert not np.array_equal(other[0], wf), period
    other = reference(D, T, [3, 40], None, ts.folded(role, 128), **t)
    c128 = np.array([ts.folded(role, 128)[l] == CASE for l in T.lib])
    # folded by 128 libraries, neither control library is one: no veto at position 3, no shallow control at position 40
    assert not (other[0][c128 & (T.pos == 3)] & BIT["CTL_ALLELE"]).any() and not (other[0][c128 & (T.pos == 40)] & BIT["CTL_DEPTH"]).any()


def test_the_reference_bucket_named_by_both_slots(route):
    """test_vet.same_bucket_views with the reference's bucket named by both slots (b0 == b1): the reference side of every record is the
    later slot's floats over the integers that are not zero; tables from position 0 .. 3 put every combination on lanes 63 and 64"""
    v, d, D, keep = tv.same_bucket_views(route, 1, 2)
    seen = set()
    for first in range(4):
        T = Tab.of([(p, 0, "+AC", sums(6, f=(2.0, 0.0, 1.0, 3.0))) for p in range(first, D.n_pos)])
        for thr in (MID, dict(MID, min_ref_reads=7, min_ref_mapq=52.0)):
            wf, wv, wc, wk, _ = check(route, v, d, D, T, np.arange(D.n_pos), what="b0 == b1 from %d" % first, **thr)
            seen |= set(wf.tolist())
        assert sorted(wv[1, 60:64].tolist()) == [0.0, 6.0, 9.0, 9.0]                    # cr: the reference bucket's reads
    assert len(seen) >= 3, seen


def bad_library_views(route):
    """test_vet's view of two libraries whose third-allele records at positions 10, 63 and 64 name libraries n_lib, n_lib + 1 and -1 in
    the reference's bucket, the other slot's and a third one, beside one valid record each"""
    L, Pn = 2, 130
    si = np.zeros((L, 2, 9, Pn), np.uint32); sf = np.zeros((L, 2, 4, Pn), np.float32)
    si[:, 0] = tv.SLOT_I[0][None, :, None] * 3; si[:, 1] = tv.SLOT_I[0][None, :, None]
    sf[:, 0] = tv.SLOT_F[0][None, :, None]; sf[:, 1] = tv.SLOT_F[1][None, :, None]
    recs = []
    for t, x in enumerate((10, 63, 64)):
        for bad in (L, L + 1, -1):
            for b in (1, 2, 3):
                recs.append(hv.record(x, bad, b, [50 + b] * 9, hv.f32bits([9.0] * 4).tolist()))
        recs.append(hv.record(x, t % L, 1, [25, 1500, 100, 12, 13, 1, 90, 2600, 150], hv.f32bits([2.0, 1.0, 3.0, 2.5]).tolist()))
    slotid = ts.high_slot_bytes(np.full((L, Pn), 1 | (2 << 8)))
    slotid[:, 120:] = 1 | (0x81 << 8)                       # (slot 1's byte 0x81 beside slot 0's 1: the reference's bucket is slot 0's alone)
    return tv.raw_dense(route, np.full((L, Pn), 30), slotid, si, sf, recs[::-1], b"A" * Pn)


def test_records_of_libraries_that_do_not_exist(route):
    """third-allele records and table records whose library is n_lib, n_lib + 1 or -1, each beside a valid record of the same position
    (table records 63 and 64 among them): the bad third-allele records change no reference bucket, the bad table records are NO_SITE
    with BRC_IVET_TABLE_OUT_OF_RANGE in the status word, veto nothing and count in no ctl_count"""
    v, d, D, keep = bad_library_views(route)
    assert D.istat[0, 1, 0, 10] == 25 and D.istat[1, 1, 0, 10] == 18 and D.istat[1, 1, 0, 63] == 25
    at = lambda p: [(p, l, "+AC", sums(c)) for l, c in ((0, 6), (-1, 9), (2, 9), (3, 9), (1, 1))]
    rows = [(p, 0, "-A", sums(3)) for p in range(0, 10)] + at(10) + [(p, 0, "-A", sums(3)) for p in range(11, 58)] + at(63) + at(64)
    rows += [(p, 0, "-A", sums(3)) for p in range(65, 70)] + [(p, p % 2, "+AC", sums(4)) for p in (100, 104, 109, 110, 117, 129)]     # (slot bytes with bit 7: ts.high_slot_bytes)
    T = Tab.of(rows)
    assert T.lib[63] == -1 and T.lib[64] == 2 and T.pos[63] == T.pos[64] == 63
    for role in ([CASE, CTL], [CTL, CASE], None):
        wf, wv, wc, wk, st = check(route, v, d, D, T, [10, 63, 64], None, role, what="bad libraries %r" % (role,), **T_(ctl_max_count=1, min_ref_reads=1))
        assert st == capi.IVET_TABLE_OUT_OF_RANGE
        bad = (T.lib < 0) | (T.lib >= 2)
        assert bad.sum() == 9 and (wf[bad] == NO_SITE).all() and not wv[:, bad].any() and not wc[bad].any()
        assert wc.max() == (1 if role == [CASE, CTL] else 6 if role == [CTL, CASE] else 0)
    assert list(wk) == [INS, INS, INS]
    # a list element one behind the planes (idx == n_pos) is out of range as any other
    w = check(route, v, d, D, T, [10, 63, 64, D.n_pos], what="idx == n_pos", **T_(min_ref_reads=1))
    assert w[4] == capi.IVET_TABLE_OUT_OF_RANGE | capi.IVET_LIST_OUT_OF_RANGE and list(w[3]) == [INS, INS, INS, 0]


def long_run(p, n, case_at):
    """n records of one position in a table of four libraries (ROLE4): the case records at case_at = (first, middle, last).  The first
    one's only matching control record lies at n - 20 (more than 64 records to its right), the last one's at 10 (to its left); the
    middle one has none: the control records around it spell its text plus one byte under the same len, or its text under another len.
    Everything else is a control or ignored record of another spelling."""
    first, mid, last = case_at
    rows = {first: (0, "+AC", None, 6), n - 20: (1, "+AC", None, 5), last: (0, "+AG", None, 6), 10: (2, "+AG", None, 7), mid: (0, "+AT", None, 6),
            mid + 1: (1, "+ATG", 2, 9), mid - 1: (2, "+AT", 3, 9), mid + 2: (3, "+AT", None, 9)}
    assert len(rows) == 8
    out = []
    for x in range(n):
        l, text, ln, c = rows.get(x, (1 + x % 3, "+C" + "ACGT"[x % 4] * (1 + x % 5), None, 8))
        out.append((p, l, text, sums(c)) + (() if ln is None else (ln,)))
    return out


def test_runs_of_130_and_300_records(route):
    """one position with 130 table records and one with 300: a run crosses a wave edge and a 256 workgroup edge, and a case record's
    only matching control record is more than 64 records away on either side"""
    v, d, D, keep = flat_views(route)
    rows = [(1, 0, "+AC", sums(6))] * 3 + long_run(5, 130, (0, 65, 129)) + [(6, 0, "+AC", sums(6))] + long_run(9, 300, (0, 150, 299)) + [(11, 1, "+AC", sums(9))]
    T = Tab.of(rows)
    assert T.m == 435
    t = T_(ctl_max_count=1)
    wf, wv, wc, wk, _ = check(route, v, d, D, T, [1, 5, 6, 9, 11], None, ROLE4, what="long runs", **t)
    for base, n, (first, mid, last) in ((3, 130, (0, 65, 129)), (134, 300, (0, 150, 299))):
        assert T.pos[base] != T.pos[base - 1] and T.pos[base + n - 1] != T.pos[base + n]
        assert wf[base + first] == BIT["CTL_ALLELE"] and wc[base + first] == 5 and wf[base + last] == BIT["CTL_ALLELE"] and wc[base + last] == 7
        assert wf[base + mid] == 0 and wc[base + mid] == 0
        assert n - 20 - first > 64 and last - 10 > 64
    assert list(wk) == [INS, INS, INS, INS, 0]
    # ... and with the roles turned round the long walks start at the control side's records
    check(route, v, d, D, T, [5, 9], None, [CTL, CASE, CASE, IGN], what="long runs, roles turned", **t)


def table_dict(route, T):
    """a Tab as the dict tensors.indels returns, in the route's memory"""
    a = dict(pos=T.pos.astype(np.int32), lib=T.lib.astype(np.int32), len=T.len.astype(np.int32), istat=T.istat.view(np.int32) if route.name == "hip" else T.istat,
             fstat=T.fstat, allele_off=T.off.view(np.int32) if route.name == "hip" else T.off, alleles=T.alleles)
    if route.name == "hip":
        a = {k: route.torch.from_numpy(np.ascontiguousarray(x)).cuda() for k, x in a.items()}
    return dict(a, m=T.m)


def test_record_sums_with_a_base_quality_sum(route):
    """records whose I_SBQ is not zero (no engine writes one into an indel bucket): the variant's base quality in vals is 0 all the
    same, VAR_BQ is never set, and tensors.vet_indels gives the same words"""
    from bam_readcount_amd import tensors
    v, d, D, keep = flat_views(route)
    recs = []
    for p in range(1, 40):
        i, f = sums(6, f=(1.0, 2.0, 3.0, 4.0))
        i[8] = 7 * p + 1
        recs.append((p, p % 2, "+AC" if p % 3 else "-AC", (i, f)))
    T = Tab.of(recs)
    assert T.istat[8].all()
    for role, thr in ((None, MID), ([CASE, CTL, IGN, IGN], EASY)):
        w = check(route, v, d, D, T, np.arange(1, 40), None, role, what="I_SBQ", **thr)
        judged = w[0] < NOT_ASKED
        assert judged.any() and not (w[0][judged] & tv.BIT["VAR_BQ"]).any() and not w[1][capi.VET_V_NAMES.index("var_bq")].any()
        assert w[1][capi.VET_V_NAMES.index("var_mapq")][judged].all()

        class Views:
            """what tensors.vet_indels asks an engine for"""
            _names = None

            def device_view(self):
                return v

            def device_indels(self):
                return d
        check_tensors(route, tensors.vet_indels(Views(), route.ivet, table_dict(route, T), idx=np.arange(1, 40), role=role, **thr), w, "I_SBQ, tensors")


def test_refused_calls_write_nothing(route, two_libs):
    ref, arrs, res = two_libs
    eng = td.computed(route.engine_lib, arrs, 50, 2950, ref, **PER_LIB)
    v, d = ts.views_of(eng)
    P = int(v.n_pos)
    T = Tab.of_oracle(res.indels).take(range(40))

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
             ("no table", dict(table=False)), ("no list", dict(no_idx=True)), ("n < 0", dict(n=-1)), ("dst_stride < m", dict(ds=T.m - 1)),
             ("memory of the other kind", dict(v=av(memory=other), d=ad(memory=other))), ("memory 0", dict(v=av(memory=0), d=ad(memory=0))),
             ("views of two kinds", dict(d=ad(memory=other))), ("another device", dict(v=av(device=int(v.device) + 1), d=ad(device=int(v.device) + 1))),
             ("views of two devices", dict(v=av(device=int(v.device) + 1))), ("a view without planes", dict(v=av(si=None))),
             ("a view without planes (depth)", dict(v=av(depth=None))), ("not a view", dict(v=capi.DeviceView())),
             ("records without their arrays", dict(d=ad(slots=None))), ("records without the third-allele array", dict(v=av(xagg=None, n_xagg=5))),
             ("n_lib differs", dict(d=ad(n_lib=1))), ("pos0 differs", dict(d=ad(pos0=int(d.pos0) + 1))), ("n_pos differs", dict(d=ad(n_pos=P - 1))),
             ("stride < m", dict(stride=T.m - 1)), ("m < 0", dict(tfields=dict(m=-1))), ("m too large", dict(tfields=dict(m=2 ** 31, stride=2 ** 31), ds=2 ** 31)),
             ("alleles_len < 0", dict(tfields=dict(alleles_len=-1))),
             ("no pos", dict(tfields=dict(pos=None))), ("no lib", dict(tfields=dict(lib=None))), ("no len", dict(tfields=dict(len=None))),
             ("no istat", dict(tfields=dict(istat=None))), ("no fstat", dict(tfields=dict(fstat=None))),
             ("no allele_off with CTL_ALLELE", dict(tfields=dict(allele_off=None))), ("no alleles with CTL_ALLELE", dict(tfields=dict(alleles=None))),
             ("kinds 0", dict(kinds=0)), ("unknown kinds", dict(kinds=INS | 1)), ("unknown kinds above", dict(kinds=DEL | 64)),
             ("a role above 2", dict(role=[1, 3])), ("no case library", dict(role=[0, 2])),
             ("freq_den 0", dict(freq_den=0)), ("strand_den 0", dict(strand_den=0)), ("ctl_frac_den 0", dict(ctl_frac_den=0)),
             ("VAR_BQ", dict(tests=capi.VET_BIT["VAR_BQ"])), ("VAR_BQ beside known ones", dict(tests=ALL_TESTS | capi.VET_BIT["VAR_BQ"])),
             ("unknown test bits", dict(tests=1 << 20)), ("unknown test bits beside known ones", dict(tests=7 | 1 << 30)), ("no workspace", dict(ws=False))]
    cases += [("%s = %r" % (k, x), dict(fields={k: x})) for k in capi.IVET_FLOATS for x in (float("nan"), float("inf"))][::3]
    cases += [("min_ref_bq = -inf", dict(fields=dict(min_ref_bq=float("-inf"))))]
    for what, kw in cases:
        a = dict(ok, **kw)
        rc, st, gf, gv, gc, gk = call(route, a.pop("v"), a.pop("d"), T, a.pop("idx"), **dict(MID, **a))
        assert rc == capi.E_ARG, what
        assert st == SENT and untouched(gf, gv, gc, gk), "%s: something was written" % what
        if kw.get("handle", True):
            assert route.ivet.lib.brc_ivet_last_error(route.ivet.h), what
    rc, st, gf, gv, gc, gk = call(route, v, d, Tab.of([]), **MID)
    assert (rc, st) == (0, 0) and untouched(gf, gv, gc, gk) and route.ivet.lib.brc_ivet_last_error(route.ivet.h) == b""
    eng.close()


# ------------------------------------------------------------------------------------------------ 10. tensors.vet_indels

def test_tensors_vet_indels_on_text_only_engines_and_its_errors(route, oracle_lib, test_bam):
    from bam_readcount_amd import tensors
    beg0, end = 10402736, 10405248
    res, text = td.oracle_result(oracle_lib, test_bam, beg0, end, test_bam["ref"], tid=20, chrom="21")
    D = tv.Dense.of(res)
    T = Tab.of_oracle(res.indels)
    assert T.m > 3
    idx = np.unique(T.pos - D.pos0)
    for opts in (dict(text_only=True), dict(device_text="21")):
        eng = td.computed(route.engine_lib, test_bam, beg0, end, test_bam["ref"], tid=20, **opts)
        t = tensors.indels(eng, route.indels)
        check_tensors(route, tensors.vet_indels(eng, route.ivet, t, idx=idx, **MID), reference(D, T, idx, **MID), "before fetch %r" % opts)
        eng.fetch_result()
        assert eng.format_region("21") == text
        r = tensors.vet_indels(eng, route.ivet, t, idx=idx.tolist(), why=[INS] * len(idx), kinds=("ins",), tests=("VAR_MAPQ", "DEPTH", "CTL_ALLELE"), **MID)
        check_tensors(route, r, reference(D, T, idx, [INS] * len(idx), kinds=INS, tests=BIT["VAR_MAPQ"] | BIT["DEPTH"] | BIT["CTL_ALLELE"], **MID), "after fetch %r" % opts)
        r = tensors.vet_indels(eng, route.ivet, t, want=("fail",), **MID)
        assert sorted(r) == ["fail", "m", "n", "n_lib", "pos0", "status"] and r["n"] == 0 and r["m"] == T.m
        no_text = {k: x for k, x in t.items() if k not in ("allele_off", "alleles")}
        r = tensors.vet_indels(eng, route.ivet, no_text, tests=("DEPTH", "VAR_COUNT"), want=("fail",), **MID)
        assert np.array_equal(tv.host_words(route, r["fail"]), reference(D, T, tests=BIT["DEPTH"] | BIT["VAR_COUNT"], **MID)[0])
        bad = [dict(idx=[5, 4]), dict(idx=[-1]), dict(idx=[res.n_pos]), dict(idx=idx, why=[1]), dict(why=[1]), dict(want=("nothing",)), dict(tests=("NOTHING",)),
               dict(tests=("VAR_BQ",)), dict(tests=capi.VET_BIT["VAR_BQ"]), dict(tests=1 << 20), dict(kinds=()), dict(kinds=("snv",)), dict(role=[2]), dict(role=[1, 1]),
               dict(role=[1], case=["x"]), dict(control=["nobody"]), dict(freq_den=0), dict(ctl_frac_den=0), dict(min_depth=-1), dict(ctl_max_count=1.5),
               dict(min_ref_bq=float("nan")), dict(max_rl_diff=1e39), dict(min_var_bq=1.0), dict(no_such_threshold=1), dict(table=no_text), dict(table=dict(m=3)),
               dict(table=None), dict(table=dict(t, m=T.m + 1))]
        wrong = (lambda a, dt: a.astype(dt)) if route.name == "sim" else (lambda a, dt: a.to(getattr(route.torch, dt)))
        bad += [dict(table=dict(t, istat=t["fstat"])), dict(table=dict(t, fstat=t["istat"])), dict(table=dict(t, istat=t["istat"][:4])),
                dict(table=dict(t, fstat=t["fstat"][:3])), dict(table=dict(t, pos=wrong(t["pos"], "int64"))), dict(table=dict(t, lib=wrong(t["lib"], "int16"))),
                dict(table=dict(t, len=wrong(t["len"], "float32"))), dict(table=dict(t, allele_off=wrong(t["allele_off"].view(t["pos"].dtype), "int16"))),
                dict(table=dict(t, alleles=wrong(t["alleles"], "int32"))), dict(table=dict(t, pos=t["istat"][:1])), dict(table=dict(t, alleles=t["istat"]))]
        for b in bad:
            with pytest.raises(ValueError):
                tensors.vet_indels(eng, route.ivet, b.pop("table", t), **b)
        eng.close()


def test_the_chain_select_indels_vet_indels_sites(route, two_libs):
    """tensors.select(indel=True, controls ignored) -> tensors.indels -> tensors.vet_indels(idx=sel["idx"], why=sel["why"]) ->
    keep.nonzero() -> tensors.sites, with device lists throughout on the GPU route: the panel holds the oracle's planes at the positions
    the reference predicate keeps"""
    from bam_readcount_amd import tensors
    import test_panel as tp
    panel = route.another("panel")
    ref, arrs, res = two_libs
    D = tv.Dense.of(res)
    T = Tab.of_oracle(res.indels)
    eng = td.computed(route.engine_lib, arrs, 50, 2950, ref, **PER_LIB)
    sel = tensors.select(eng, route.select, role=[CASE, IGN], snv=False, indel=True, min_depth=4, min_alt=2)
    h = ts.Dense(D.depth, D.istat[:, 1:5, 0, :], D.refbase, [(d_["pos"], d_["lib"], d_["len"], d_["i"][0]) for d_ in res.indels], D.pos0)
    widx, wwhy = h.want([CASE, IGN], ts.P_(ts.INDEL, min_depth=4, min_alt=2))
    assert sel["n"] == len(widx) > 5
    t = tensors.indels(eng, route.indels)
    r = tensors.vet_indels(eng, route.ivet, t, idx=sel["idx"], why=sel["why"], role=[CASE, CTL], **EASY)
    if route.name == "hip":
        assert sel["idx"].is_cuda and sel["why"].is_cuda and t["pos"].is_cuda
    w = reference(D, T, widx, wwhy, [CASE, CTL], **EASY)
    check_tensors(route, r, w, "chain")
    kept = np.nonzero(w[3])[0]
    assert 0 < len(kept) < len(widx)
    for p, is_kept in ((X_SAME, False), (X_DSAME, False), (X_SPELL, True), (X_PREFIX, True), (X_DLEN, True), (X_INSDEL, True)):
        assert ((p - D.pos0) in widx[kept]) == is_kept, p    # select's allele-blind veto would have dropped every one of them
    k = r["keep"].nonzero()[0] if route.name == "sim" else r["keep"].nonzero()[:, 0]
    pn = tensors.sites(eng, panel, positions=sel["pos"][k], want=tensors.KINDS)
    want = tp.want_at(res, widx[kept])
    assert pn["n"] == len(kept)
    for kind in tp.KINDS:
        assert np.array_equal(tp.host_words(route, pn[kind]).reshape(want[kind].shape), want[kind]), kind
    # the table of a site list (tensors.sites(indels=)): the records at the listed positions alone, judged where they lie
    listed = [X_SAME, X_SPELL, X_DLEN, X_DSAME, X_DSAME]
    ps = tensors.sites(eng, panel, positions=listed, want=("depth",), indels=route.indels)
    sub = T.take([x for x in range(T.m) if T.pos[x] in listed])
    assert ps["indels"]["m"] == sub.m >= 8
    r2 = tensors.vet_indels(eng, route.ivet, ps["indels"], idx=np.array(listed) - D.pos0, role=[CASE, CTL], **EASY)
    w2 = reference(D, sub, np.array(listed) - D.pos0, None, [CASE, CTL], **EASY)
    check_tensors(route, r2, w2, "the table of a site list")
    assert list(w2[3] != 0) == [False, True, True, False, False]
    eng.close()


# ------------------------------------------------------------------------------------------------ 11. the host sanitizers

def _serialize(v, d, calls):
    """the host views and the calls as ivet_check.cpp reads them"""
    b = ts._serialize(v, d, [])
    b = b[:36] + struct.pack("<i", len(calls)) + b[40:]
    for T, idx, why, role, kinds, tests, want, with_text, t in calls:
        idx = np.zeros(0, np.int32) if idx is None else np.asarray(idx, np.int32)
        b += struct.pack("<qqqiiiiII", T.m, idx.size, T.alleles.size if with_text else 0, 0 if why is None else 1, 0 if role is None else 1, 1 if with_text else 0,
                         want, tests, kinds)
        b += struct.pack("<12I13f", *[t[k] for k in capi.IVET_UINTS + capi.IVET_FLOATS])
        b += T.pos.astype(np.int32).tobytes() + T.lib.astype(np.int32).tobytes() + T.len.astype(np.int32).tobytes() + T.istat.tobytes() + T.fstat.tobytes()
        if with_text:
            b += T.off.tobytes() + T.alleles.tobytes()
        b += idx.tobytes() + (np.asarray(why, np.uint32).tobytes() if why is not None else b"") + bytes(role or [])
    return b


def _sanitized(tmp_path, name, v, d, D, calls):
    """ivet_check_asan over one pair of host views: every call must return 0 without a report and give the reference's words, every
    destination that was not wanted as it was filled; returns the number of records compared"""
    assert v.memory == capi.MEM_HOST and d.memory == capi.MEM_HOST
    case, out = str(tmp_path / (name + ".bin")), str(tmp_path / (name + ".res"))
    open(case, "wb").write(_serialize(v, d, calls))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    pr = subprocess.run([side.sim_checker(side.SIDE["ivet"]), case, out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert pr.returncode == 0, (name, pr.stderr.decode()[-3000:])
    assert pr.stdout.decode().strip() == "%d calls" % len(calls), name
    raw = np.fromfile(out, np.uint32); o = 0
    some = 0
    for T, idx, why, role, kinds, tests, want, with_text, t in calls:
        wf, wv, wc, wk, wst = reference(D, T, idx, why, role, kinds, tests, with_text=with_text, **t)
        assert raw[o].view(np.int32) == 0 and raw[o + 1] == (wst if want & 16 else SENT), (name, T.m, raw[o:o + 2])
        o += 2
        for bit, w in ((1, wf), (2, wv.view(np.uint32)), (4, wc), (8, wk)):
            g = raw[o:o + w.size]; o += w.size
            assert np.array_equal(g, w.ravel()) if want & bit else untouched(g), (name, T.m, bit)
        some += T.m
    assert o == raw.size, name
    return some


def test_calls_under_the_host_sanitizers(sim_route, tmp_path):
    """The hand-made cases above on the CPU build with -fsanitize=address,undefined, a stand-alone program: views and table of exactly
    their sizes (alleles of exactly alleles_len bytes, stride == m), lists of exactly n elements, role of exactly n_lib bytes, a scratch
    of exactly brc_ivet_workspace bytes, destinations of exactly [planes][m] and [n] — a load or store outside them is a report — and
    the results are the reference's.  Never under the gpu mark; nothing is loaded into python with a sanitizer."""
    route = sim_route
    rng = np.random.default_rng(2)
    some = 0
    for records in (True, False):
        v, d, D, keep = shape_views(route, records)
        calls = []
        for m in (0, 1, 63, 64, 65, 256, 257):
            T = random_table(D, m, rng, 3)
            idx = np.unique(T.pos - D.pos0)
            calls += [(T, idx, rng.integers(0, 64, idx.size), ROLE3, INS | DEL, ALL_TESTS, 31, True, MID), (T, None, None, None, INS, ALL_TESTS, 31, True, MID)]
        T = edge_table(D, (130, 330), 3, rng)
        idx = np.concatenate([[-3], np.unique(T.pos - D.pos0), [D.n_pos]])
        calls += [(T, idx, None, ROLE3, INS | DEL, BIT["CTL_ALLELE"] | BIT["RL_DIFF"], w, True, MID) for w in (1, 2, 4, 8, 16, 0, 15)]
        calls += [(T, idx, None, [CTL, CASE, IGN], INS | DEL, ALL_TESTS & ~BIT["CTL_ALLELE"], 31, False, MID)]
        if not records:
            R = random_table(D, 200, rng, 3)
            U = R.take(list(range(120, 200)) + list(range(120)))
            B = Tab(R.pos, R.lib, R.len, R.istat, R.fstat, R.off.copy(), R.alleles)
            B.off[40] = B.alleles.size + 1000; B.off[41] = 0xFFFFFFFF; B.off[90] = B.off[88]; B.off[120] = 0; B.off[200] = 0xFFFFFFF0
            bad = np.unique(R.pos - D.pos0)[::-1]
            calls += [(U, np.unique(U.pos - D.pos0), None, ROLE3, INS | DEL, ALL_TESTS, 31, True, MID), (B, None, None, ROLE3, INS | DEL, ALL_TESTS, 31, True, MID),
                      (R, bad, None, ROLE3, INS | DEL, ALL_TESTS, 23, True, MID)]
            s = sums(6)
            p0, P = D.pos0, D.n_pos
            N = Tab.of([(p0 - 1, 0, "+AC", s), (p0, 0, "+AC", s), (p0 + 5, -1, "+AC", s), (p0 + 5, 0, "", s, 0), (p0 + 5, 3, "+AC", s), (p0 + P - 1, 2, "-A", s),
                        (p0 + P, 0, "+AC", s), (2 ** 31 - 1, 0, "+A", s)])
            calls += [(N, [0, 5, P - 1], None, ROLE3, INS | DEL, ALL_TESTS, 31, True, MID)]
        some += _sanitized(tmp_path, "shapes%d" % records, v, d, D, calls)
    assert some > 3000
    v, d, D, keep = flat_views(route)
    some = _sanitized(tmp_path, "matching", v, d, D, [(match_table(), np.arange(1, 16), None, ROLE4, INS | DEL, ALL_TESTS, 31, True, T_(ctl_max_count=1))])
    v, d, D, keep, _ = tv.two_record_views(route)
    T = edge_table(D, (130, 330), 2, rng)
    some += _sanitized(tmp_path, "two_records", v, d, D, [(T, np.unique(T.pos), None, [CTL, CASE], INS | DEL, ALL_TESTS, 31, True, MID)])
    # an unsorted table over linked third-allele records: in range, and exact where the contract says so (the sanitizer is the check here)
    q, U = unsorted_over_records(D)
    open(str(tmp_path / "unsorted.bin"), "wb").write(_serialize(v, d, [(U, [q, 130], None, None, INS | DEL, ALL_TESTS, 31, True, MID)]))
    pr = subprocess.run([side.sim_checker(side.SIDE["ivet"]), str(tmp_path / "unsorted.bin"), str(tmp_path / "unsorted.res")], stdout=subprocess.PIPE,
                        stderr=subprocess.PIPE, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert pr.returncode == 0 and pr.stdout.decode().strip() == "1 calls", pr.stderr.decode()[-3000:]
    raw = np.fromfile(str(tmp_path / "unsorted.res"), np.uint32)
    assert raw[0] == 0 and raw[1] == capi.IVET_TABLE_NOT_ASCENDING and np.array_equal(raw[2 + 3:2 + 6], reference(D, U, [q, 130], **MID)[0][3:])
    v, d, D, keep, T = metric_views(route)
    some += _sanitized(tmp_path, "metrics", v, d, D, [(T, None, None, None, INS | DEL, ALL_TESTS, 31, True, MID)])
    assert some > 400
