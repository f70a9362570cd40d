"""Device-side consensus caller (include/brc_cons.h): brc_cons_call and bam_readcount_amd.tensors.consensus against the header's rule
restated in plain Python / numpy uint64 over the ORACLE's dense result (test_vet.Dense.of, test_ivet.Tab.of_oracle) and over hand-made
arrays — call, cnt, ins_rec, off, seq, counts and the status word equal byte for byte, no tolerance.  The reference reads nothing of
the core.

Every body runs twice (the `route` fixture): [sim] = libbrc_sim.so + tests/cpu_cons/libbrc_cons_sim.so, host memory, in the CPU suite;
[hip] = the product's libraries on the GPU (gpu-marked), views, table, scratch and destinations in device memory allocated through
torch.  Destinations are filled with 0xA5 first and are PAD elements wider than the contract: everything outside the contract must
keep it.  The scratch has exactly brc_cons_workspace bytes.  The consensus library is no row of tests/abi_side.py's table yet: the
module makes its own handle beside the Route's.

Sizes that matter to the kernels (brc_cons.hip): a wave is 64 consecutive positions, a workgroup and a scan tile 256, the scan's
single workgroup takes 256 tile sums per round — 65 537 positions need a second round."""
import os
import struct
import subprocess

import numpy as np
import pytest

from bam_readcount_amd import capi
from bam_readcount_amd import consensus as cc
from conftest import ROOT
import handmade_views as hv
from route import Route, SENT, SENT8
import synth
import test_indels as ti
import test_ivet as tiv
import test_vet as tv

LIBS = ("dense", "indels", "inorm", "join")
CPU_DIR = os.path.join(ROOT, "tests", "cpu_cons")
PAD = 3
ALL = ("call", "cnt", "ins_rec", "off", "seq")
ALIGNED, FILL_REF, CENTRIC = cc.CONS_ALIGNED, cc.CONS_FILL_REF, cc.CONS_INS_CENTRIC
NOT_ASC, OOR = cc.CONS_TABLE_NOT_ASCENDING, cc.CONS_TABLE_OUT_OF_RANGE
NO_INS, U32 = cc.CONS_NO_INS, 2 ** 32 - 1
U64 = np.uint64
DEFAULT = dict(lib_on=None, flags=0, min_depth=0, min_count=1, num=1, den=2, ins_min_count=1, ins_num=1, ins_den=2, fill=ord("N"), gap=ord("-"))


def P_(**kw):
    assert not set(kw) - set(DEFAULT)
    return dict(DEFAULT, **kw)


def cons_sim_lib():
    """the CPU build of the consensus library, built"""
    subprocess.check_call(["make", "-s", "-C", CPU_DIR], stderr=subprocess.DEVNULL)
    return os.path.join(CPU_DIR, "libbrc_cons_sim.so")


def cons_handle(route):
    h = cc.Cons(None if route.name == "hip" else cons_sim_lib())
    assert h.kind() == ("hip-gfx950" if route.name == "hip" else "sim")
    return h


def make_route(name, libs=LIBS):
    r = Route(name, libs, engine=True)
    r.cons = cons_handle(r)
    return r


@pytest.fixture(scope="module", params=["sim", pytest.param("hip", marks=pytest.mark.gpu)])
def route(request):
    return make_route(request.param)


@pytest.fixture(scope="module")
def sim_route():
    return make_route("sim")


# ------------------------------------------------------------------------------------------------ the header's rule, restated

def reference(cnt, refbase, pos0, T, k0, n, seq_cap=None, **p):
    """cnt: counts [L, 4, P] of A C G T; refbase: P characters ('N' where the reference has none); T: a test_ivet.Tab
    -> dict(call uint8 [n], cnt uint32 [6, n], ins_rec uint32 [n], off uint32 [n + 1], seq uint8 [cap] with 0xA5 where nothing is
    written, counts, status)"""
    p = P_(**p)
    cnt = np.asarray(cnt).astype(U64)
    L = cnt.shape[0]
    on = np.ones(L, bool) if p["lib_on"] is None else np.asarray(p["lib_on"], bool)
    count = T.istat[0].astype(U64)
    ok_lib = lambda l: 0 <= l < L and bool(on[l])
    c = cnt[on][:, :, k0:k0 + n].sum(axis=0, dtype=U64).reshape(4, n)
    d = np.zeros(n, U64)
    status = 0
    for r in range(T.m):
        ln, l = int(T.len[r]), int(T.lib[r])
        if ln != 0 and not 0 <= l < L:
            status |= OOR
        if r and T.pos[r] < T.pos[r - 1]:
            status |= NOT_ASC
        if ln < 0 and ok_lib(l):
            a = int(T.pos[r]) - pos0 - k0 + 1
            lo, hi = max(a, 0), min(a - ln, n)
            if lo < hi:
                d[lo:hi] += count[r]
    d &= U64(U32)
    if n == 0:
        status = 0                                                    # (no position: the table is not looked at, the word is cleared)
    tot = c.sum(axis=0, dtype=U64) + d
    q = lambda x: (x >= U64(p["min_count"])) & (x * U64(p["den"]) >= U64(p["num"]) * tot)
    shallow = tot < U64(p["min_depth"])
    deleted = ~shallow & q(d) & (d > c).all(axis=0)
    mask = np.zeros(n, np.int64)
    for b in range(4):
        mask |= q(c[b]).astype(np.int64) << b
    uncalled = shallow | (~deleted & (mask == 0))
    fill = np.frombuffer(refbase, np.uint8)[k0:k0 + n] if p["flags"] & FILL_REF else np.full(n, p["fill"], np.uint8)
    call = np.where(uncalled, fill, np.where(deleted, np.uint8(p["gap"]), np.frombuffer(cc.CONS_IUPAC.encode(), np.uint8)[mask])).astype(np.uint8)
    # the insertions: run by run; a position takes the first run that names it
    texts = T.texts()
    ins = np.full(n, NO_INS, np.int64); sup = np.zeros(n, U64); taken = set()
    r = 0
    while r < T.m:
        e = r
        while e + 1 < T.m and T.pos[e + 1] == T.pos[r]:
            e += 1
        j = int(T.pos[r]) - pos0 - k0
        if 0 <= j < n and j not in taken:
            taken.add(j)
            cand = [x for x in range(r, e + 1) if T.len[x] > 0 and ok_lib(int(T.lib[x]))]
            pooled = {}
            for x in range(r, e + 1):
                if ok_lib(int(T.lib[x])):
                    key = (int(T.len[x]), texts[x])
                    pooled[key] = pooled.get(key, 0) + int(count[x])
            if cand:
                best = max(cand, key=lambda x: (pooled[(int(T.len[x]), texts[x])], -x))
                s = pooled[(int(T.len[best]), texts[best])]
                t2 = int(tot[j]) + (sum(int(count[x]) for x in cand) if p["flags"] & CENTRIC else 0)
                sup[j] = s
                if t2 >= p["min_depth"] and s >= p["ins_min_count"] and s * p["ins_den"] >= p["ins_num"] * t2:
                    ins[j] = best
        r = e + 1
    out_cnt = np.concatenate([c, d[None], sup[None]]).astype(np.uint32)
    if p["flags"] & ALIGNED:
        off = np.arange(n + 1, dtype=np.int64); total = n
        cap = n if seq_cap is None else seq_cap
        seq = np.full(cap, SENT8, np.uint8); seq[:min(cap, n)] = call[:min(cap, n)]
    else:
        emitted = [texts[x][1:] if x != NO_INS else b"" for x in ins]
        lens = (~deleted).astype(np.int64) + np.array([len(t) for t in emitted], np.int64)
        off = np.concatenate([[0], np.cumsum(lens)]); total = int(off[-1])
        cap = total if seq_cap is None else seq_cap
        lim = min(cap, total)
        seq = np.full(cap, SENT8, np.uint8)
        at = off[:-1][~deleted]
        fits = at + 1 <= lim
        seq[at[fits]] = call[~deleted][fits]
        for j in np.flatnonzero(ins != NO_INS):
            o = int(off[j]) + (0 if deleted[j] else 1)
            if emitted[j] and o + len(emitted[j]) <= lim:
                seq[o:o + len(emitted[j])] = np.frombuffer(emitted[j], np.uint8)
    return dict(call=call, cnt=out_cnt, ins_rec=ins.astype(np.uint32), off=off.astype(np.uint32), seq=seq, counts=total & U32, status=status)


# ------------------------------------------------------------------------------------------------ views, tables, the call

def count_views(route, cnt, mode=None, stride=None, pos0=0, ref=None, ref_lo=0, ref_len=None, extra=()):
    """A hand-made view whose base buckets hold cnt [L, 4, P] and whose other sums hold junk.  mode [P]: 0 — the first two non-zero
    buckets in slot 0 and slot 1, the others in third-allele records; 1 — slot 0 names no bucket, the first non-zero bucket sits in slot
    1; 2 — every bucket in a record.  extra: further records (hv.record) as they are.  -> (view, indels view, refbase, keep-alive)"""
    cnt = np.asarray(cnt, np.uint32)
    L, _, Pn = cnt.shape
    mode = np.zeros(Pn, np.int64) if mode is None else np.asarray(mode)
    junk_i = np.arange(7001, 7009, dtype=np.uint32)
    A = {"ncol": np.ones((L, Pn), np.uint32), "depth": cnt.sum(axis=1).astype(np.uint32), "slotid": np.full((L, Pn), 0xFFFF, np.uint32),
         "si": np.zeros((L, 2, 9, Pn), np.uint32), "sf": hv.f32bits(np.full((L, 2, 4, Pn), 1.5, np.float32)), "unavail": None}
    recs = list(extra)
    for l, k in zip(*np.nonzero(cnt.any(axis=1))):
        nz = [b for b in range(4) if cnt[l, b, k]]
        slots = {0: nz[:2], 1: [None] + nz[:1], 2: []}[int(mode[k])]
        sid = 0xFFFF
        for s, b in enumerate(slots):
            if b is None:
                continue
            sid = (sid & ~(0xFF << (8 * s))) | ((b + 1) << (8 * s))
            A["si"][l, s, 0, k] = cnt[l, b, k]; A["si"][l, s, 1:, k] = junk_i
        A["slotid"][l, k] = sid
        for b in nz:
            if b not in slots:
                recs.append(hv.record(k, l, b + 1, [int(cnt[l, b, k])] + junk_i.tolist(), [0x3FC00000] * 4))
    v, keep = hv.make_view(route, A, recs, stride=stride, pos0=pos0)
    d = capi.DeviceIndels(route.mem, 0, L, pos0, Pn, None, 0)
    rl = pos0 + Pn if ref_len is None else ref_len
    refbase = bytearray(b"N" * Pn)
    if ref is not None:
        keep["ref"] = route.copy_bytes(np.frombuffer(bytes(ref), np.uint8))
        d.ref, d.ref_lo, d.ref_hi, d.ref_len = route.ptr(keep["ref"]), ref_lo, ref_lo + len(ref), rl
        for k in range(Pn):
            p = pos0 + k
            if ref_lo <= p < ref_lo + len(ref) and 0 <= p < rl and ref[p - ref_lo] != 0:
                refbase[k] = ref[p - ref_lo]
    return v, d, bytes(refbase), keep


def tab(recs):
    """recs: (pos, lib, text with its sign, count[, len]) in table order -> test_ivet.Tab"""
    return tiv.Tab.of([(r[0], r[1], r[2], ([r[3]] + [0] * 8, [0.0] * 4)) + tuple(r[4:5]) for r in recs]) if recs else \
        tiv.Tab([], [], [], np.zeros((9, 0), np.uint32), np.zeros((4, 0), np.float32), [0], b"")


def table_bufs(route, T, stride=None):
    """the table in the route's memory, every array of exactly its own size -> (ConsTable, keep-alive)"""
    keep = dict(pos=route.copy_bytes(T.pos.astype(np.int32)), lib=route.copy_bytes(T.lib.astype(np.int32)), len=route.copy_bytes(T.len.astype(np.int32)),
                count=route.copy_bytes(T.istat[0].astype(np.uint32)), allele_off=route.copy_bytes(T.off.astype(np.uint32)), alleles=route.copy_bytes(T.alleles))
    t = cc.ConsTable(T.m, T.m if stride is None else stride, alleles_len=int(T.alleles.size))
    for k, b in keep.items():
        setattr(t, k, route.ptr(b) if T.m else None)
    return t, keep


def run(route, v, d, T, k0, n, ds=None, want=ALL, counts=True, seq_cap=None, status=True, ws=True, handle=True, params=True, table=True, stride=None,
        wsb=None, **p):
    """brc_cons_call into sentinel-filled destinations PAD elements wider than the contract; without BRC_CONS_ALIGNED and a given seq_cap,
    a first call asks for the count alone.  -> dict(rc, counts, status, <destination>: the contract's part, buf: the raw buffers)"""
    p = P_(**p)
    ds = n if ds is None else ds
    par, keepalive = cc.cons_params(p["lib_on"], p["flags"], p["min_depth"], p["min_count"], (p["num"], p["den"]), p["ins_min_count"], (p["ins_num"], p["ins_den"]),
                                    p["fill"], p["gap"])
    t, tkeep = table_bufs(route, T, stride)
    wsb = (route.cons.workspace(v, n, T.m) if v is not None else 0) if wsb is None else wsb
    wsbuf = route.sentinel_bytes(wsb)
    base = dict(workspace=route.ptr(wsbuf) if ws else None)

    def fn(v, d, par, t, k0, n, ds, seq_cap=0, **kw):                     # (brc_cons_call itself: the handle may be NULL)
        return route.cons.lib.brc_cons_call(route.cons.h if handle else None, capi._ref(v), capi._ref(d), capi._ref(par), capi._ref(t), k0, n, ds, seq_cap,
                                            *[kw.get(k) for k in ("counts", "call", "cnt", "ins_rec", "off", "seq", "status", "workspace")], None)
    args = (v, d, par if params else None, t if table else None, k0, n, ds)
    cbuf = route.sentinel_bytes(4)
    if seq_cap is None:
        if p["flags"] & ALIGNED:
            seq_cap = n
        else:
            rc = fn(*args, counts=route.ptr(cbuf), **base)
            if rc:
                return dict(rc=rc)
            seq_cap = int(route.host(cbuf)[:4].view(np.uint32)[0])
            cbuf = route.sentinel_bytes(4)
    size = dict(call=n + PAD, cnt=4 * (6 * ds + PAD), ins_rec=4 * (n + PAD), off=4 * (n + 1 + PAD), seq=seq_cap + PAD)
    bufs = {k: route.sentinel_bytes(size[k]) for k in ALL}
    sbuf = route.sentinel_bytes(4)
    rc = fn(*args, seq_cap=seq_cap, counts=route.ptr(cbuf) if counts else None, status=route.ptr(sbuf) if status else None,
            **{k: route.ptr(bufs[k]) for k in want}, **base)
    hb = {k: route.host(b)[:size[k]].copy() for k, b in bufs.items()}
    out = dict(rc=rc, buf=hb, seq_cap=seq_cap, counts=int(route.host(cbuf)[:4].view(np.uint32)[0]), status=int(route.host(sbuf)[:4].view(np.uint32)[0]))
    out["call"] = hb["call"][:n]; out["cnt"] = hb["cnt"][:24 * ds].view(np.uint32).reshape(6, ds)
    out["ins_rec"] = hb["ins_rec"][:4 * n].view(np.uint32); out["off"] = hb["off"][:4 * (n + 1)].view(np.uint32); out["seq"] = hb["seq"][:seq_cap]
    for k in ALL:                                                         # behind the contract, and whatever was not asked for
        edge = dict(call=n, cnt=24 * ds, ins_rec=4 * n, off=4 * (n + 1), seq=seq_cap)[k] if (k in want and rc == 0) else 0
        assert (hb[k][edge:] == SENT8).all(), "%s: written outside the contract" % k
    del keepalive, tkeep
    return out


def untouched(o):
    return all((b == SENT8).all() for b in o["buf"].values()) and o["counts"] == SENT and o["status"] == SENT


def check(route, v, d, cnt, refbase, T, k0, n, what="", want=ALL, ds=None, seq_cap=None, stride=None, **p):
    pos0 = int(v.pos0)
    w = reference(cnt, refbase, pos0, T, k0, n, seq_cap=seq_cap, **p)
    g = run(route, v, d, T, k0, n, ds=ds, want=want, seq_cap=seq_cap, stride=stride, **p)
    assert g["rc"] == 0, (what, route.cons._call("_last_error")(route.cons.h))
    assert g["status"] == w["status"], (what, g["status"], w["status"])
    assert g["counts"] == w["counts"], (what, g["counts"], w["counts"])
    for k in want:
        got = g[k][:, :n] if k == "cnt" else g[k]
        assert np.array_equal(got, w[k]), "%s: %s differs at %r" % (what, k, np.argwhere(got != w[k])[:4].tolist())
    if "cnt" in want:
        assert (g["cnt"][:, n:] == SENT).all(), "%s: cnt wrote into the padding" % what
    return g, w


def random_counts(rng, L, Pn, deep=40):
    """mostly one deep base, some two- and three-allele positions, some empty ones"""
    cnt = np.zeros((L, 4, Pn), np.uint32)
    major = rng.integers(0, 4, Pn)
    cnt[:, major, np.arange(Pn)] = rng.integers(1, deep, (L, Pn))
    for frac, hi in ((0.3, deep), (0.15, 6), (0.1, 3)):
        m = rng.random(Pn) < frac
        cnt[:, rng.integers(0, 4, Pn)[m], np.flatnonzero(m)] = rng.integers(0, hi, (L, int(m.sum())))
    cnt[:, :, rng.random(Pn) < 0.05] = 0
    return cnt


def random_table(rng, L, pos0, Pn, m, max_del=9, count_hi=30):
    """a sorted table of m records around the planes: insertions of a few texts, deletions of 1 .. max_del bases"""
    recs = []
    for p in np.sort(rng.integers(pos0 - 6, pos0 + Pn + 2, m)):
        l = int(rng.integers(0, L))
        if rng.random() < 0.5:
            recs.append((int(p), l, "+" + "".join(rng.choice(list("ACGT"), int(rng.integers(1, 4)))), int(rng.integers(1, count_hi))))
        else:
            recs.append((int(p), l, "-" + "N" * int(rng.integers(1, max_del + 1)), int(rng.integers(1, count_hi))))
    return tab(recs)


# ------------------------------------------------------------------------------------------------ a haplotype end to end

RL, LO, HI = 3000, 100, 900
SUBS = (163, 207, 251, 333, 377, 455, 561, 655, 707, 777, 829)


def _free(ref, cands, width):
    """the first candidate anchor with no substitution near it whose event cannot be left-aligned: (a deletion of `width` bases) the
    reference character at the anchor differs from the last deleted one; an insertion's text is chosen to end differently"""
    for a in cands:
        if (not width or ref[a] != ref[a + width]) and not set(range(a - 8, a + width + 8)) & set(SUBS):
            return a
    raise AssertionError("no anchor outside a repeat")


@pytest.fixture(scope="module")
def haplotype(oracle_lib):
    """A 3 kb reference, a haplotype over it — eleven substitutions, a 3-base insertion, a 5-base deletion, one site where six of ten
    reads carry the haplotype's base and four the reference's — and reads of length 100 every 10 bases over [100, 900) that spell it.
    -> dict(ref, arrs (library 0 / 1 by turns), hap: the haplotype string of [150, 850), ...)"""
    rng = np.random.default_rng(2024)
    ref = synth.make_ref(rng, RL)
    other = lambda ch: b"ACGT"[(b"ACGT".index(ch) + 1) % 4]
    sub = ref.copy()
    for p in SUBS:
        sub[p] = other(ref[p])
    het = 504
    hap_base = other(ref[het])
    ia = _free(ref, (404, 414, 424), 0)                               # the insertion's anchor: ≡ 4 mod 10, so every spanning read has 5 bases of flank
    itext = "GA" + chr(other(ref[ia]))
    da = _free(ref, (604, 614, 624), 5)                               # the deletion's anchor; deleted: da + 1 .. da + 5
    assert chr(ref[ia]) != itext[-1] and ref[da] != ref[da + 5]
    with_alt, without = sub.copy(), sub.copy()
    with_alt[het] = hap_base
    rows = []
    for i, s in enumerate(range(LO, HI - 99, 10)):
        e = s + 100
        ops = [(0, 100)]
        if s + 4 <= ia and ia + 6 <= e:                               # five bases of flank on either side at the least
            ops = [(0, ia + 1 - s), (1, 3), (0, e - ia - 1)]
        elif s + 4 <= da and da + 5 + 5 <= e:
            ops = [(0, da + 1 - s), (2, 5), (0, e - da - 6)]
        elif s <= da < e:                                             # the deletion without flank behind it: the read ends in front of it
            ops = [(0, da + 1 - s)]
        assert not s > da or s > da + 5                               # (no read starts inside the deletion)
        assert not (s <= ia < e) or len(ops) == 3                     # (every read across the insertion's anchor carries it)
        rows.append((s, ops, itext if len(ops) == 3 and ops[1][0] == 1 else None, i % 2, with_alt if i % 5 < 3 else without))
    rows.append((1200, [(0, 100)], None, 0, sub))                     # a lone read far behind: the planes reach it, [900, 1200) has no reads
    batches = [ti.hand_reads(r[4], [r[:4]]) for r in rows]
    arrs = ti.merged(batches)
    hap = bytearray()
    for p in range(150, 850):
        if not da < p <= da + 5:
            hap.append(hap_base if p == het else sub[p])
        if p == ia:
            hap += itext.encode()
    return dict(ref=ref, sub=sub, arrs=arrs, hap=bytes(hap), het=het, hap_base=hap_base, ia=ia, itext=itext, da=da)


def host(route, a):
    return np.ascontiguousarray(a.cpu().numpy() if route.name == "hip" else a)


def assert_tensors(route, r, w, what, want=ALL):
    for k in want:
        got = host(route, r[k]).view(np.uint8 if k in ("seq", "call") else np.uint32)
        assert np.array_equal(got, w[k]), "%s: %s differs at %r" % (what, k, np.argwhere(got != w[k])[:4].tolist())
    assert int(host(route, r["status"]).view(np.uint32)[0]) == w["status"], what


def dense_of(res):
    D = tv.Dense.of(res)
    return D.istat[:, 1:5, 0, :], D.refbase, tiv.Tab.of_oracle(res.indels)


@pytest.mark.parametrize("normalized", [False, True], ids=["gathered", "normalized"])
def test_a_haplotype_is_called_back_byte_for_byte(route, oracle_lib, haplotype, normalized):
    from bam_readcount_amd import tensors
    H = haplotype
    ref, ia, da, het = H["ref"], H["ia"], H["da"], H["het"]
    res, _ = ti.oracle_result(oracle_lib, H["arrs"], 41, 1400, ref)
    cnt, refbase, T = dense_of(res)
    assert {(d["pos"], d["allele"]) for d in res.indels} == {(ia, "+" + H["itext"]), (da, "-" + bytes(ref[da + 1:da + 6]).decode())}
    eng = ti.computed(route.engine_lib, H["arrs"], 41, 1400, ref)
    table = tensors.indels(eng, route.indels)
    if normalized:
        table = tensors.normalize_indels(eng, route.inorm, table)
        assert table["m"] == T.m and not host(route, table["src"]["shift"]).any()          # (the events stand outside repeats)
    pos0 = res.pos0
    kw = dict(table=table, min_depth=4, beg0=150, end=850)
    # 3. the haplotype, and the liftover map
    r = tensors.consensus(eng, route.cons, frac=(1, 2), **kw)
    assert (r["first"], r["n"], r["m"]) == (150, 700, T.m)
    assert bytes(host(route, r["seq"])) == H["hap"]
    off = host(route, r["off"]).view(np.uint32).astype(np.int64)
    want_off = np.array([p - 150 + (3 if p > ia else 0) - min(max(p - da - 1, 0), 5) for p in range(150, 851)])
    assert np.array_equal(off, want_off)
    w = reference(cnt, refbase, pos0, T, 150 - pos0, 700, min_depth=4)
    assert_tensors(route, r, w, "haplotype")
    assert int(host(route, r["ins_rec"]).view(np.uint32)[ia - 150]) == int(np.flatnonzero(T.len > 0)[0])
    # 4. a quarter is enough: the heterozygous site prints its two-base code
    r4 = tensors.consensus(eng, route.cons, frac=(1, 4), **kw)
    code = cc.CONS_IUPAC[(1 << b"ACGT".index(ref[het])) | (1 << b"ACGT".index(H["hap_base"]))]
    s4 = bytearray(H["hap"]); s4[int(want_off[het - 150])] = ord(code)
    assert bytes(host(route, r4["seq"])) == bytes(s4) and code in "MRWSYK"
    assert_tensors(route, r4, reference(cnt, refbase, pos0, T, 150 - pos0, 700, min_depth=4, den=4), "a quarter")
    # 5. aligned: the substituted reference, `gap` on the five deleted positions — and no count is read
    ra = tensors.consensus(eng, route.cons, aligned=True, gap="*", **kw)
    al = bytearray(bytes(H["sub"][150:850])); al[het - 150] = H["hap_base"]; al[da + 1 - 150:da + 6 - 150] = b"*****"
    assert bytes(host(route, ra["seq"])) == bytes(al) == bytes(host(route, ra["call"]))
    assert_tensors(route, ra, reference(cnt, refbase, pos0, T, 150 - pos0, 700, min_depth=4, flags=ALIGNED, gap=ord("*")), "aligned")
    # 6. fill="ref": a stretch without reads prints the TRUE reference
    rf = tensors.consensus(eng, route.cons, table=table, min_depth=4, fill="ref", beg0=800, end=1250)
    wf = reference(cnt, refbase, pos0, T, 800 - pos0, 450, min_depth=4, flags=FILL_REF)
    assert_tensors(route, rf, wf, "fill=ref")
    s = bytes(host(route, rf["seq"]))
    assert not cnt[:, :, 900 - pos0:1200 - pos0].any() and s[100:] == bytes(ref[900:1250]) and s[:50] == H["hap"][-50:] and len(s) == 450
    rn = tensors.consensus(eng, route.cons, table=table, min_depth=4, fill="n", beg0=800, end=1250, want=("seq",))
    assert bytes(host(route, rn["seq"]))[70:] == b"n" * 380 and bytes(host(route, rn["seq"]))[:50] == H["hap"][-50:]
    # the table gathered by the call itself
    rg = tensors.consensus(eng, route.cons, indels=route.indels, min_depth=4, beg0=150, end=850)
    assert_tensors(route, rg, w, "table=None")
    eng.close()


def test_libraries_pooled_masked_and_joined(route, oracle_lib, haplotype):
    from bam_readcount_amd import tensors
    import test_join as tj
    H = haplotype
    ref, arrs = H["ref"], H["arrs"]
    allL, _ = ti.oracle_result(oracle_lib, arrs, 41, 1400, ref)
    only0, _ = ti.oracle_result(oracle_lib, tj.one_library(arrs, 0), 41, 1400, ref)
    per, _ = ti.oracle_result(oracle_lib, arrs, 41, 1400, ref, **tv.PER_LIB)
    assert per.n_lib == 2
    pos0 = allL.pos0
    P2 = ti.computed(route.engine_lib, arrs, 41, 1400, ref, **tv.PER_LIB)
    t2 = tensors.normalize_indels(P2, route.inorm, tensors.indels(P2, route.indels))
    kw = dict(min_depth=3, beg0=120, end=880)
    pooled = tensors.consensus(P2, route.cons, table=t2, **kw)
    w_all = reference(*dense_of(allL)[:2], pos0, dense_of(allL)[2], 120 - pos0, 760, min_depth=3)
    # two libraries pooled == the all-library engine on the same reads (ins_rec names another table's record: the texts agree)
    for k in ("seq", "off", "call", "cnt"):
        assert np.array_equal(host(route, pooled[k]).view(np.uint8 if k in ("seq", "call") else np.uint32), w_all[k]), k
    assert_tensors(route, pooled, reference(*dense_of(per)[:2], pos0, dense_of(per)[2], 120 - pos0, 760, min_depth=3), "pooled")
    # libs=[0] == an engine on library 0's reads alone
    first = tensors.consensus(P2, route.cons, table=t2, libs=["libA"], **kw)
    w0 = reference(*dense_of(only0)[:2], pos0, dense_of(only0)[2], 120 - pos0, 760, min_depth=3)
    for k in ("seq", "off", "call", "cnt"):
        assert np.array_equal(host(route, first[k]).view(np.uint8 if k in ("seq", "call") else np.uint32), w0[k]), k
    assert bytes(w0["seq"]) != bytes(w_all["seq"])                       # (half the depth: the window's ends fall below min_depth)
    assert_tensors(route, first, reference(*dense_of(per)[:2], pos0, dense_of(per)[2], 120 - pos0, 760, min_depth=3, lib_on=[1, 0]), "libs=[0]")
    # ... and through a join of two single-library engines
    Bs = [ti.computed(route.engine_lib, tj.one_library(arrs, l), 41, 1400, ref) for l in (0, 1)]
    J = tensors.join(Bs, route.join, names=["a", "b"])
    tJ = tensors.indels(J, route.indels)
    joined = tensors.consensus(J, route.cons, table=tJ, **kw)
    for k in ("seq", "off", "call", "cnt"):
        assert np.array_equal(host(route, joined[k]), host(route, pooled[k])), k
    j0 = tensors.consensus(J, route.cons, table=tJ, libs=["a"], **kw)
    assert np.array_equal(host(route, j0["seq"]), host(route, first["seq"]))
    for bad in (dict(libs=[]), dict(libs=["nobody"]), dict(frac=(3, 2)), dict(frac=(1, 0)), dict(frac=(1, 65536)), dict(ins_frac=(2, 1)), dict(fill="NN"),
                dict(gap=""), dict(want=("text",)), dict(min_count=-1), dict(table=None)):
        with pytest.raises(ValueError):
            tensors.consensus(P2, route.cons, **dict(dict(kw, table=t2), **bad))
    for e in Bs + [P2, J]:
        e.close()


# ------------------------------------------------------------------------------------------------ boundaries: hand-made views and tables

@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 65537])
def test_window_lengths_and_strides(route, n):
    """every n around a wave, a workgroup and the scan's second carry round; a stride equal to n and an odd one; buckets in slot 0, in
    slot 1 and in a third-allele record on lanes 0, 63, 64; records outside the window, unused, of a library that does not exist"""
    rng = np.random.default_rng(n)
    L, k0 = 2, (0 if n > 1000 else 5)
    Pn = k0 + n + (0 if n > 1000 else 4)
    cnt = random_counts(rng, L, Pn)
    mode = rng.integers(0, 3, Pn) if n < 1000 else (rng.random(Pn) < 0.01) * 2
    if k0:
        cnt[:, :, [k0 - 1, k0 + n]] = 0                                   # (the records below are the only ones there)
    for lane in (0, 63, 64):
        for m_, k in enumerate(range(k0 + lane, min(k0 + lane + 3, Pn))):
            cnt[:, :, k] = [[9, 4, 0, 2], [1, 0, 6, 3]]
            mode[k] = m_
    body = ([99] * 9, [0x3FC00000] * 4)
    extra = [hv.record(k0 - 1 if k0 else Pn, 0, 1, *body), hv.record(k0 + n if k0 else Pn + 1, 1, 2, *body), hv.record(hv.NONE32, 0, 3, *body),
             hv.record(k0, L, 1, *body), hv.record(k0, 0, 5, *body), hv.record(k0, 1, 0, *body)]
    ref = rng.choice(np.frombuffer(b"ACGTacgtN\0", np.uint8), Pn).tobytes()
    T = random_table(rng, L, 40, Pn, min(3 * n, 600) if n > 1 else 6)
    p = dict(min_depth=6, min_count=2, num=1, den=4, ins_num=1, ins_den=5)
    for stride in (None, (Pn + 7) | 1):                                   # the planes' own length, and an odd stride
        v, d, refbase, keep = count_views(route, cnt, mode, stride=stride, pos0=40, ref=ref, ref_lo=40, extra=extra)
        for flags in (0, ALIGNED | FILL_REF):
            check(route, v, d, cnt, refbase, T, k0, n, "n=%d stride=%r flags=%d" % (n, stride, flags), ds=n + (stride is not None) * 5, flags=flags, **p)
    if k0:                                                                # the window is the whole view: a stride equal to n
        w = slice(k0, k0 + n)
        v, d, refbase, keep = count_views(route, cnt[:, :, w], mode[w], pos0=40 + k0, ref=ref, ref_lo=40)
        assert int(v.stride) == int(v.n_pos) == n
        check(route, v, d, cnt[:, :, w], refbase, T, 0, n, "n=%d, the whole view" % n, **p)


def test_all_fifteen_codes_and_every_threshold(route):
    # the fifteen sets: bucket b holds 10 where it is in the set, else 1
    cnt = np.ones((1, 4, 16), np.uint32)
    for mask in range(16):
        for b in range(4):
            if mask >> b & 1:
                cnt[0, b, mask] = 10
    v, d, refbase, keep = count_views(route, cnt)
    g, w = check(route, v, d, cnt, refbase, tab([]), 0, 16, "iupac", min_count=5, num=0, den=1, fill=ord("?"))
    assert bytes(g["call"]) == b"?ACMGRSVTWYHKDBN"
    # x * den == num * T and one read below; min_count and min_depth at and one below
    cnt = np.zeros((1, 4, 6), np.uint32)
    cnt[0, :2, 0] = [6, 2]            # 2 * 4 == 1 * 8: C qualifies
    cnt[0, :2, 1] = [7, 2]            # 2 * 4 <  1 * 9: it does not
    cnt[0, :2, 2] = [9, 3]            # min_count = 3 at
    cnt[0, :2, 3] = [6, 2]            # ... (as element 0, judged with min_count 3 below)
    cnt[0, :2, 4] = [5, 3]            # T == min_depth
    cnt[0, :2, 5] = [4, 3]            # one below
    v, d, refbase, keep = count_views(route, cnt)
    g, _ = check(route, v, d, cnt, refbase, tab([]), 0, 6, "fraction", num=1, den=4)
    assert bytes(g["call"][:2]) == b"MA"
    g, _ = check(route, v, d, cnt, refbase, tab([]), 0, 6, "min_count", min_count=3, num=1, den=4)
    assert bytes(g["call"][2:4]) == b"MA"
    g, _ = check(route, v, d, cnt, refbase, tab([]), 0, 6, "min_depth", min_depth=8, num=1, den=4, fill=ord("x"))
    assert bytes(g["call"][4:6]) == b"Mx"
    # d equal to the largest base is not deleted, one above is
    cnt = np.zeros((1, 4, 4), np.uint32); cnt[0, 2, :] = 5
    T = tab([(0, 0, "-N", 5), (1, 0, "-N", 6), (2, 0, "-N", 4)])
    v, d, refbase, keep = count_views(route, cnt)
    g, _ = check(route, v, d, cnt, refbase, T, 0, 4, "deleted", num=1, den=2)
    assert bytes(g["call"]) == b"GG-G"
    g, _ = check(route, v, d, cnt, refbase, T, 0, 4, "min_count above the bases", num=1, den=2, min_count=6)
    assert bytes(g["call"]) == b"NN-N"


@pytest.mark.parametrize("L", [1, 2, 254])
def test_library_counts_and_lib_on(route, L):
    rng = np.random.default_rng(L)
    Pn = 70
    cnt = random_counts(rng, L, Pn, deep=9)
    T = random_table(rng, L, 0, Pn, 60)
    T.lib[::7] = L; T.lib[3] = -1                                       # (some records of libraries that do not exist)
    v, d, refbase, keep = count_views(route, cnt, rng.integers(0, 3, Pn))
    g, w = check(route, v, d, cnt, refbase, T, 0, Pn, "all", min_depth=3)
    assert w["status"] & OOR
    if L > 1:
        on = (rng.random(L) < 0.5).astype(np.uint8); on[L - 1] = 1; on[0] = 0
        g2, w2 = check(route, v, d, cnt, refbase, T, 0, Pn, "masked", min_depth=3, lib_on=on)
        assert not np.array_equal(w["cnt"], w2["cnt"])                  # an ignored library's reads and records are masked
        only = np.zeros(L, np.uint8); only[L - 1] = 1                   # (a bit above the first words of the mask)
        check(route, v, d, cnt, refbase, T, 0, Pn, "last library alone", lib_on=only)


def test_255_libraries_are_refused(route):
    cnt = np.ones((255, 4, 3), np.uint32)
    v, d, refbase, keep = count_views(route, cnt)
    o = run(route, v, d, tab([]), 0, 3, seq_cap=3)
    assert o["rc"] == capi.E_ARG and untouched(o)


def test_deletions(route):
    Pn, pos0, k0, n = 300, 1000, 20, 260
    cnt = np.zeros((2, 4, Pn), np.uint32); cnt[:, 1, :] = 3
    v, d, refbase, keep = count_views(route, cnt, pos0=pos0, ref=b"A" * 200, ref_lo=pos0, ref_len=pos0 + 150)
    w0 = pos0 + k0
    recs = [(w0 - 30, 0, "-" + "N" * 30, 9),          # from an anchor in front of the window, ending ON its first element
            (w0 - 5, 1, "-NN", 50),                    # ending in front of the window: counts nowhere
            (w0 + 9, 0, "-N", 8),                      # length 1
            (w0 + 20, 0, "-" + "N" * 30, 7), (w0 + 25, 1, "-" + "N" * 10, 7),          # nested
            (w0 + 60, 0, "-NNN", 8), (w0 + 63, 0, "-NNNN", 9),                         # adjacent
            (w0 + 100, 0, "-NN", U32), (w0 + 100, 1, "-NN", 7),                        # counts that wrap 2^32: d = 6
            (w0 + 140, 1, "-" + "N" * 40, 20),         # running past ref_len (pos0 + 150)
            (w0 + n - 4, 0, "-NNN", 9),                # ending on the last element
            (w0 + n - 2, 1, "-" + "N" * 100, 9),       # running past the window and past the planes
            (w0 + n - 1, 0, "-NN", 30), (w0 + n + 5, 0, "-NN", 30)]                    # behind the window: count nowhere inside
    T = tab(recs)
    g, w = check(route, v, d, cnt, refbase, T, k0, n, "deletions", min_depth=2, num=1, den=2)
    dd = g["cnt"][4, :n]
    assert dd[0] == 9 and dd[1] == 0 and dd[10] == 8 and dd[9] == 0 and dd[11] == 0 and dd[26] == 14 and dd[36] == 7 and dd[51] == 0
    assert list(dd[61:69]) == [8, 8, 8, 9, 9, 9, 9, 0] and dd[101] == 6 and dd[102] == 6 and dd[n - 1] == 18 and dd[n - 3] == 9 and dd[n - 4] == 0
    assert bytes(g["call"][100:104]) == b"CCCC" and g["call"][10] == ord("-")         # (6 of 12 ties nothing: 6 > 6 is false)
    check(route, v, d, cnt, refbase, T, k0, n, "deletions, library 1 alone", lib_on=[0, 1], flags=ALIGNED)


def test_a_deletion_of_100000_bases_costs_what_a_deletion_of_one_costs(route):
    n = 131073
    cnt = np.zeros((1, 4, n), np.uint32); cnt[0, 3, :] = 2
    v, d, refbase, keep = count_views(route, cnt)
    acct = []
    for ln in (1, 100000):
        T = tab([(7, 0, "-N", 5, -ln), (n - 3, 0, "+AC", 4)])
        g, w = check(route, v, d, cnt, refbase, T, 0, n, "a deletion of %d" % ln)
        t = route.cons.last_timing()
        acct.append((t["bytes_read"], t["bytes_written"]))
        assert int(g["cnt"][4].astype(np.int64).sum()) == 5 * ln and g["counts"] == n - ln + 2
    assert acct[0] == acct[1] and acct[0][0] > 12 * n                  # by construction: two atomic adds per record, one scan over n


def test_insertions(route):
    Pn, pos0 = 80, 500
    cnt = np.zeros((2, 4, Pn), np.uint32); cnt[0, 0, :] = 6; cnt[1, 0, :] = 4
    v, d, refbase, keep = count_views(route, cnt, pos0=pos0)
    recs = [(pos0 + 2, 0, "+AC", 5), (pos0 + 2, 0, "+GT", 5),                      # a tie: the smaller index
            (pos0 + 5, 0, "+TT", 3), (pos0 + 5, 1, "+TT", 3), (pos0 + 5, 1, "+GG", 5),          # one text in two libraries is pooled: 6 > 5
            (pos0 + 8, 0, "+A", 4), (pos0 + 8, 0, "+AC", 5), (pos0 + 8, 1, "+AG", 5), (pos0 + 8, 1, "+A", 2),   # a prefix and another text are distinct: +A pooled 6
            (pos0 + 11, 0, "+A=N", 9),                                             # '=' and 'N' pass through
            (pos0 + 14, 0, "-NN", 30), (pos0 + 15, 0, "+CG", 30),                  # behind a DELETED position
            (pos0 + 20, 0, "+C", 4), (pos0 + 21, 0, "+C", 5),                      # ins_num at its boundary: 4 * 2 < 10 <= 5 * 2
            (pos0 + 30, 1, "+G", 3, 1), (pos0 + 30, 0, "-N", 2), (pos0 + 30, 0, "+G", 3, 2),    # another length is another allele; a deletion in the run
            (pos0 + Pn - 1, 0, "+TTT", 9)]                                         # behind the window's last position
    T = tab(recs)
    g, w = check(route, v, d, cnt, refbase, T, 0, Pn, "insertions")
    ir = g["ins_rec"].astype(np.int64)
    assert [ir[2], ir[5], ir[8], ir[11], ir[15], ir[20], ir[21], ir[30], ir[Pn - 1]] == [0, 2, 5, 9, 11, NO_INS, 13, NO_INS, 17]
    assert list(g["cnt"][5, [2, 5, 8, 30]]) == [5, 6, 6, 3]
    s = bytes(g["seq"])
    assert s[:16] == b"AAAACAAATTAAAAAA"[:16] and b"AA=NA" in s and s.endswith(b"ATTT") and g["call"][15] == ord("-") and g["call"][16] == ord("-")
    assert s[int(g["off"][15]):int(g["off"][17])] == b"CG"               # the text alone: neither position prints a base
    # INS_CENTRIC on and off at the boundary: support 5, I = 5, T = 10: 5 * 2 >= 10 but 5 * 2 < 15
    g2, _ = check(route, v, d, cnt, refbase, T, 0, Pn, "insertion-centric", flags=CENTRIC)
    assert g2["ins_rec"][21] == NO_INS and g["ins_rec"][21] == 13
    g3, _ = check(route, v, d, cnt, refbase, T, 0, Pn, "insertion-centric, a third", flags=CENTRIC, ins_num=1, ins_den=3)
    assert g3["ins_rec"][21] == 13 and g3["ins_rec"][20] == NO_INS       # 4 * 3 < 14
    check(route, v, d, cnt, refbase, T, 0, Pn, "ins_min_count", ins_min_count=6)
    check(route, v, d, cnt, refbase, T, 3, Pn - 9, "a window inside", lib_on=[1, 0])
    # runs of 65 and 257 alleles at one position: every text once, one of them in both libraries
    for run_len in (65, 257):
        texts = ["+" + "".join("ACGT"[(i >> s) & 3] for s in (0, 2, 4, 6, 8)) for i in range(run_len)]
        recs = [(pos0 + 1, 0, "+A", 1)] + [(pos0 + 40, i % 2, t, 2) for i, t in enumerate(texts)] + [(pos0 + 40, 1, texts[run_len - 2], 1), (pos0 + 41, 0, "+C", 1)]
        g, w = check(route, v, d, cnt, refbase, tab(recs), 0, Pn, "a run of %d" % run_len, ins_num=0, ins_den=1)
        assert g["ins_rec"][40] == run_len - 1 and g["cnt"][5, 40] == 3


def test_allele_offsets_that_are_garbage_stay_inside_alleles(route):
    Pn = 40
    cnt = np.zeros((1, 4, Pn), np.uint32); cnt[0, 0, :] = 6
    v, d, refbase, keep = count_views(route, cnt)
    T = tab([(3, 0, "+AC", 5), (3, 0, "+AC", 1), (9, 0, "+GGG", 6), (12, 0, "+T", 6), (20, 0, "+CC", 6)])
    for off in ([0, 3, 6, U32, 2, 5], [7, 3, U32, U32, 0, 14], [14, 0, 0, 14, 0, 13]):
        T.off = np.array(off, np.uint32)
        check(route, v, d, cnt, refbase, T, 0, Pn, "offsets %r" % (off,), ins_num=0, ins_den=1)


@pytest.mark.parametrize("m", [0, 1, 256, 257, 65537])
def test_table_lengths(route, m):
    rng = np.random.default_rng(m)
    Pn = 200 if m < 1000 else 4000
    cnt = random_counts(rng, 2, Pn, deep=12)
    T = random_table(rng, 2, 10, Pn, m)
    v, d, refbase, keep = count_views(route, cnt, pos0=10)
    check(route, v, d, cnt, refbase, T, 0, Pn, "m=%d" % m, min_depth=3, stride=m + 11)
    check(route, v, d, cnt, refbase, T, 7, Pn - 20, "m=%d aligned" % m, min_depth=3, flags=ALIGNED)


def test_capacities_single_destinations_and_two_calls(route):
    rng = np.random.default_rng(77)
    Pn = 300
    cnt = random_counts(rng, 2, Pn, deep=12)
    T = random_table(rng, 2, 0, Pn, 120)
    v, d, refbase, keep = count_views(route, cnt, rng.integers(0, 3, Pn))
    p = dict(min_depth=3, ins_num=1, ins_den=8)
    g, w = check(route, v, d, cnt, refbase, T, 0, Pn, "exact", **p)
    total = w["counts"]
    assert total > Pn - 60 and (w["ins_rec"] != NO_INS).sum() > 5
    last_ins = int(np.flatnonzero(w["ins_rec"] != NO_INS)[-1])
    for cap in (total - 1, int(w["off"][last_ins]) + 2, int(w["off"][last_ins]) + 1, 1, 0, total + 2):
        check(route, v, d, cnt, refbase, T, 0, Pn, "seq_cap=%d" % cap, seq_cap=cap, **p)          # a piece that does not fit whole is not written
    for cap in (Pn - 1, 0):
        check(route, v, d, cnt, refbase, T, 0, Pn, "aligned seq_cap=%d" % cap, seq_cap=cap, flags=ALIGNED, **p)
    check(route, v, d, cnt, refbase, T, 0, Pn, "the counts alone", want=(), seq_cap=0, **p)
    for k in ALL:
        check(route, v, d, cnt, refbase, T, 0, Pn, k + " alone", want=(k,), seq_cap=total, **p)
        check(route, v, d, cnt, refbase, T, 0, Pn, k + " alone, aligned", want=(k,), flags=ALIGNED, **p)
    o = run(route, v, d, T, 0, Pn, want=(), counts=False, seq_cap=0, **p)                           # the status word alone
    assert o["rc"] == 0 and o["status"] == 0 and o["counts"] == SENT
    a, b = run(route, v, d, T, 0, Pn, **p), run(route, v, d, T, 0, Pn, **p)
    assert all(np.array_equal(a["buf"][k], b["buf"][k]) for k in ALL)
    o = run(route, v, d, T, 9, 0, seq_cap=0, **p)                                                   # n == 0
    assert o["rc"] == 0 and o["counts"] == 0 and o["status"] == 0 and (o["buf"]["off"][:4] == 0).all() and (o["buf"]["off"][4:] == SENT8).all()


def test_a_table_that_is_not_ascending(route):
    rng = np.random.default_rng(5)
    Pn = 150
    cnt = random_counts(rng, 2, Pn, deep=12)
    T = random_table(rng, 2, 0, Pn, 90)
    T = T.take(rng.permutation(T.m))
    v, d, refbase, keep = count_views(route, cnt)
    g, w = check(route, v, d, cnt, refbase, T, 0, Pn, "shuffled", min_depth=3)
    assert w["status"] & NOT_ASC


def test_refused_calls_write_nothing(route):
    cnt = np.ones((2, 4, 20), np.uint32)
    v, d, refbase, keep = count_views(route, cnt, pos0=5)
    T = tab([(7, 0, "+A", 3), (9, 1, "-N", 2)])

    def refused(what, vv=v, dd=d, TT=T, k0=0, n=20, **kw):
        o = run(route, vv, dd, TT, k0, n, **dict(dict(seq_cap=20), **kw))
        assert o["rc"] == capi.E_ARG and untouched(o), what
        if kw.get("handle", True):
            assert route.cons._call("_last_error")(route.cons.h), what

    def av(**kw):
        c = capi.DeviceView(); capi.C.memmove(capi.C.byref(c), capi.C.byref(v), capi.C.sizeof(v))
        for k, x in kw.items():
            setattr(c, k, x)
        return c

    def ad(**kw):
        c = capi.DeviceIndels(); capi.C.memmove(capi.C.byref(c), capi.C.byref(d), capi.C.sizeof(d))
        for k, x in kw.items():
            setattr(c, k, x)
        return c

    def at(**kw):
        t = tiv.Tab(T.pos, T.lib, T.len, T.istat, T.fstat, T.off, T.alleles.tobytes())
        return t, kw
    refused("no handle", handle=False)
    refused("no view", vv=None, wsb=64); refused("no indels view", dd=None); refused("no params", params=False); refused("no table", table=False)
    refused("k0 < 0", k0=-1); refused("n < 0", n=-1, ds=0, wsb=64); refused("window past the planes", k0=1, n=20); refused("dst_stride < n", ds=19)
    refused("seq_cap < 0", seq_cap=-1); refused("no workspace", ws=False); refused("stride < m", stride=1)
    refused("another region", dd=ad(pos0=6)); refused("another library count", dd=ad(n_lib=3)); refused("another length", dd=ad(n_pos=19))
    refused("other memory", vv=av(memory=3 - route.mem), dd=ad(memory=3 - route.mem)); refused("another device", vv=av(device=1), dd=ad(device=1))
    refused("no planes", vv=av(slotid=None)); refused("records without their array", vv=av(xagg=None)); refused("stride < n_pos", vv=av(stride=19))
    for bad in (dict(flags=8), dict(den=0), dict(den=65536), dict(ins_den=0), dict(ins_den=65536), dict(num=3, den=2), dict(ins_num=2, ins_den=1), dict(fill=256),
                dict(gap=256), dict(lib_on=[0, 0]), dict(lib_on=[1, 2])):
        refused(repr(bad), **bad)
    # a table with records but without one of its arrays
    par, _ = cc.cons_params()
    for k in ("pos", "lib", "len", "count", "allele_off", "alleles"):
        t, tkeep = table_bufs(route, T)
        setattr(t, k, None)
        ws = route.sentinel_bytes(route.cons.workspace(v, 20, 2)); c = route.sentinel_bytes(4)
        assert route.cons.call_raw(v, d, par, t, 0, 20, 20, counts=route.ptr(c), workspace=route.ptr(ws)) == capi.E_ARG and (route.host(c)[:4] == SENT8).all(), k
    t, tkeep = table_bufs(route, T); t.alleles_len = -1
    assert route.cons.call_raw(v, d, par, t, 0, 20, 20, counts=route.ptr(c), workspace=route.ptr(ws)) == capi.E_ARG
    t, tkeep = table_bufs(route, T); t.m = -1
    assert route.cons.call_raw(v, d, par, t, 0, 20, 20, counts=route.ptr(c), workspace=route.ptr(ws)) == capi.E_ARG
    t.m = 2 ** 31; t.stride = 2 ** 31
    assert route.cons.call_raw(v, d, par, t, 0, 20, 20, counts=route.ptr(c), workspace=route.ptr(ws)) == capi.E_ARG
    assert (route.host(c)[:4] == SENT8).all()
    assert route.cons.workspace(None, 5, 5) == 0 and route.cons.workspace(v, 0, 5) == 0 and route.cons.workspace(v, 20, 2) % 4 == 0


# ------------------------------------------------------------------------------------------------ the host sanitizers

def serialize(cnt_view, T, calls):
    """a view, a table and a list of calls as cons_check.cpp reads them (tests/cpu_cons/cons_check.cpp has the layout)"""
    A, recs, stride, pos0, ref, ref_lo, ref_len = cnt_view
    L, Pn = A["ncol"].shape
    rec = hv.records_array(recs) if len(recs) else np.zeros((0, 16), np.uint32)

    def planes(a, rows):
        out = np.full((rows, stride), hv.POISON, np.uint32); out[:, :Pn] = np.asarray(a, np.uint32).reshape(rows, Pn)
        return out.tobytes()
    b = struct.pack("<iiqqQqqq", L, pos0, Pn, stride, len(rec), ref_lo, len(ref), ref_len)
    b += planes(A["ncol"], L) + planes(A["depth"], L) + planes(A["slotid"], L) + planes(A["si"], L * 18) + planes(A["sf"], L * 8) + rec.tobytes() + bytes(ref)
    b += struct.pack("<qq", T.m, T.alleles.size)
    b += T.pos.astype(np.int32).tobytes() + T.lib.astype(np.int32).tobytes() + T.len.astype(np.int32).tobytes() + T.istat[0].astype(np.uint32).tobytes()
    b += T.off.astype(np.uint32).tobytes() + T.alleles.tobytes()
    b += struct.pack("<i", len(calls))
    for c in calls:
        p = P_(**c["p"])
        on = p["lib_on"]
        b += struct.pack("<qqqq", c["k0"], c["n"], c["ds"], c["seq_cap"])
        b += struct.pack("<i10I", 0 if on is None else 1, p["flags"], p["min_depth"], p["min_count"], p["num"], p["den"], p["ins_min_count"], p["ins_num"], p["ins_den"],
                         p["fill"], p["gap"])
        b += bytes(on if on is not None else [1] * L)
    return b


def test_calls_under_the_host_sanitizers(tmp_path):
    """cons_check_asan: the CPU build with a main of its own under -fsanitize=address,undefined; every buffer of exactly the contract's
    size.  A subset of the boundary cases above, fed as a file; no Python process is involved."""
    subprocess.check_call(["make", "-s", "-C", CPU_DIR, "asan"], stderr=subprocess.DEVNULL)
    exe = os.path.join(CPU_DIR, "cons_check_asan")
    rng = np.random.default_rng(31)
    L, Pn, pos0, stride = 2, 330, 40, 337
    cnt = random_counts(rng, L, Pn, deep=12)
    route = Route("sim")                                              # (memory only: nothing is called through it)
    mode = rng.integers(0, 3, Pn)
    ref = rng.choice(np.frombuffer(b"ACGTacgtN\0", np.uint8), Pn - 10).tobytes()
    v, d, refbase, keep = count_views(route, cnt, mode, stride=stride, pos0=pos0, ref=ref, ref_lo=pos0 + 3, ref_len=pos0 + 300)
    host = {k: route.host(b).view(np.uint32).reshape(-1, stride)[:, :Pn] for k, b in keep.items() if k in ("ncol", "depth", "slotid", "si", "sf")}
    A = dict(ncol=host["ncol"], depth=host["depth"], slotid=host["slotid"], si=host["si"].reshape(L, 2, 9, Pn), sf=host["sf"].reshape(L, 2, 4, Pn))
    recs = route.host(keep["xagg"]).view(np.uint32).reshape(-1, 16)
    assert len(recs) == int(v.n_xagg) > 10
    T = random_table(rng, L + 1, pos0, Pn, 200, max_del=400)
    T2 = T.take(rng.permutation(T.m)); T2.off = T2.off.copy(); T2.off[5] = U32; T2.off[9] = 0              # unsorted, garbage offsets
    for tag, TT in (("sorted", T), ("shuffled", T2)):
        calls = []
        for k0, n in ((0, Pn), (1, 1), (3, 63), (7, 257), (Pn - 1, 1), (5, 0)):
            for p in (dict(min_depth=3), dict(min_depth=3, flags=ALIGNED | FILL_REF), dict(lib_on=[0, 1], flags=CENTRIC, ins_num=0, ins_den=1)):
                w = reference(cnt, refbase, pos0, TT, k0, n, **p)
                for cap in sorted({int(w["counts"]), max(int(w["counts"]) - 1, 0), 0}):
                    calls.append(dict(k0=k0, n=n, ds=n + 2, seq_cap=cap, p=p, w=reference(cnt, refbase, pos0, TT, k0, n, seq_cap=cap, **p)))
        open(tmp_path / "case.bin", "wb").write(serialize((A, recs, stride, pos0, ref, pos0 + 3, pos0 + 300), TT, calls))
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        pr = subprocess.run([exe, str(tmp_path / "case.bin"), str(tmp_path / "res.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert pr.returncode == 0, pr.stderr.decode()[-3000:]
        assert pr.stdout.decode().strip() == "%d calls" % len(calls)
        res = np.fromfile(tmp_path / "res.bin", np.uint8); o = 0
        for c in calls:
            n, ds, cap, w = c["n"], c["ds"], c["seq_cap"], c["w"]
            rc, status, counts = struct.unpack_from("<iII", res, o); o += 12
            assert (rc, status, counts) == (0, w["status"], w["counts"]), (tag, c["k0"], n, c["p"])
            for k, size in (("call", n), ("cnt", 4 * (5 * ds + n) if n else 0), ("ins_rec", 4 * n), ("off", 4 * (n + 1)), ("seq", cap)):
                got = res[o:o + size]; o += size
                if k == "cnt":
                    flat = np.full(6 * ds, SENT, np.uint32); flat[:size // 4] = got.view(np.uint32)
                    got = flat.reshape(6, ds)
                    assert (got[:, n:] == SENT).all()
                    got = got[:, :n]
                elif k in ("ins_rec", "off"):
                    got = got.view(np.uint32)
                assert np.array_equal(got, w[k]), (tag, k, c["k0"], n, cap, c["p"])
        assert o == res.size
