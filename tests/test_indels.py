"""The device-resident indel table (include/brc_indels.h): brc_device_indels_get + brc_indels_gather against the ORACLE's
brc_result.indel list — integers equal, floats equal as uint32 bit patterns, allele text equal bytewise, order equal — and the thirteen
metric columns against numpy's fp32 division on the oracle's sums and against the text the oracle prints.

Every body runs twice (the `route` fixture): [sim] = libbrc_sim.so + tests/sim_indels/libbrc_indels_sim.so, host memory, in the CPU
suite; [hip] = the product's libraries on the GPU (gpu-marked), scratch and destinations in device memory allocated through torch.
The host sanitizers run the CPU build over the window list.

Sizes that matter to the kernels (brc_indels.hip): a wave has 64 lanes — one position of the `pressure` batch carries 72 records (4
libraries x 18 insertion alleles), so its run is ranked by lanes of more than one wave; every kernel and every scan tile is 256 wide —
the batch spans more than 256 positions and yields more than 256 records, so both scans (positions, allele lengths) need more than
one workgroup."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from bam_readcount_amd import capi
import abi_side as side
from route import Route, SENT, SENT8
import synth

DESTS = capi.INDEL_DESTS
PLANES = dict(pos=1, lib=1, len=1, rep_read=1, rep_qpos=1, istat=9, fstat=4, metrics=13)
PAD = 3              # elements of every destination behind what the contract lets a call touch
WAVE, TILE = 64, 256


@pytest.fixture(scope="module", params=["sim", pytest.param("hip", marks=pytest.mark.gpu)])
def route(request):
    return Route(request.param, ("indels",), engine=True)


def gather(route, view, k0, n, cap, acap, dests=DESTS, counts=True, ws_bytes=None, handle=True):
    """brc_indels_gather into sentinel-filled buffers with PAD elements behind every destination's contract size; the scratch has
    exactly brc_indels_workspace bytes (or ws_bytes; 0: a NULL scratch).  Returns (rc, counts u32[2], {dest: u32 / u8 words})."""
    c, a = max(cap, 0), max(acap, 0)
    size = {k: 4 * (PLANES[k] * c + PAD) for k in PLANES}
    size["allele_off"] = 4 * (c + 1 + PAD); size["alleles"] = a + PAD
    bufs = {k: route.sentinel_bytes(size[k]) for k in dests}
    cbuf = route.sentinel_bytes(8)
    need = route.indels.workspace(view, n) if view is not None else 0
    wsb = need if ws_bytes is None else ws_bytes
    ws = route.sentinel_bytes(wsb)
    args = {k: route.ptr(b) for k, b in bufs.items()}
    fn = route.indels.lib.brc_indels_gather
    rc = fn(route.indels.h if handle else None, C.byref(view) if view is not None else None, k0, n, route.ptr(ws) if wsb else None, wsb,
            route.ptr(cbuf) if counts else None, cap, acap, *[args.get(k) for k in DESTS], None)
    out = {k: (route.host(b)[:size[k]] if k == "alleles" else route.host(b)[:size[k]].view(np.uint32)) for k, b in bufs.items()}
    return rc, route.host(cbuf)[:8].view(np.uint32).copy(), out


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
    """The thirteen printed columns (BasicStat.cpp:117-140) of records [9][m] / [4][m], by numpy's fp32 division of the sums converted
    with astype(np.float32)."""
    i = istat.astype(np.float32); f = fstat
    c = i[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        cols = [c, i[1] / c, i[8] / c, i[2] / c, i[3], i[4], f[0] / c, f[2] / c, i[6] / c, i[5],
                np.where(istat[5] > 0, f[1] / i[5], np.float32(0)), i[7] / c, f[3] / c]
    m = np.stack([np.asarray(x, np.float32) for x in cols], axis=0)
    m[:, istat[0] == 0] = 0
    assert m.dtype == np.float32
    return m


def table_of(indels):
    """{dest: u32 / u8 words} of a list of the oracle's indel records, in the list's order"""
    m = len(indels)
    t = {k: np.array([d[k] for d in indels], np.int64).astype(np.uint32).reshape(1, m) for k in ("pos", "lib", "len", "rep_read", "rep_qpos")}
    ist = np.array([d["i"] for d in indels], np.uint32).reshape(m, 9).T.copy()
    fst = np.array([d["f"] for d in indels], np.float32).reshape(m, 4).T.copy()
    t["istat"] = ist; t["fstat"] = fst.view(np.uint32); t["metrics"] = metrics_of(ist, fst).view(np.uint32)
    text = [d["allele"].encode("latin1") for d in indels]
    t["allele_off"] = np.concatenate([[0], np.cumsum([len(x) for x in text])]).astype(np.uint32)
    t["alleles"] = np.frombuffer(b"".join(text), np.uint8)
    return t


def window_of(res, k0, n):
    lo = res.pos0 + k0
    return [d for d in res.indels if lo <= d["pos"] < lo + n]


def assert_table(got, want, cap, acap, what, dests=DESTS):
    """the prefix the capacities allow equals the oracle's, everything else still holds the sentinel"""
    m = want["pos"].shape[1]; w = min(m, cap)
    for k in dests:
        if k in PLANES:
            g = got[k][:PLANES[k] * cap].reshape(PLANES[k], cap)
            assert np.array_equal(g[:, :w], want[k][:, :w]), "%s: %s differs at %r" % (what, k, np.argwhere(g[:, :w] != want[k][:, :w])[:4].tolist())
            assert (g[:, w:] == SENT).all() and (got[k][PLANES[k] * cap:] == SENT).all(), "%s: %s written behind the records" % (what, k)
        elif k == "allele_off":
            assert np.array_equal(got[k][:w + 1], want[k][:w + 1]), "%s: allele_off" % what
            assert (got[k][w + 1:] == SENT).all(), "%s: allele_off written behind counts[0] + 1" % what
        else:
            exp = np.full(got[k].size, SENT8, np.uint8)
            for r in range(w):
                a, b = int(want["allele_off"][r]), int(want["allele_off"][r + 1])
                if b <= acap:
                    exp[a:b] = want["alleles"][a:b]
            assert np.array_equal(got[k], exp), "%s: allele bytes differ at %r" % (what, np.argwhere(got[k] != exp)[:4].ravel().tolist())


def check_window(route, view, res, k0, n, what, slack=0):
    """the two-call protocol on one window: counts alone, then everything with exact (+ slack) capacities"""
    want = table_of(window_of(res, k0, n))
    m, nb = want["pos"].shape[1], int(want["alleles"].size)
    rc, counts, _ = gather(route, view, k0, n, 0, 0, dests=())
    assert rc == 0, (what, route.indels.lib.brc_indels_last_error(route.indels.h))
    assert counts.tolist() == [m, nb], (what, counts.tolist(), [m, nb])
    rc, counts, got = gather(route, view, k0, n, m + slack, nb + slack)
    assert rc == 0 and counts.tolist() == [m, nb], what
    assert_table(got, want, m + slack, nb + slack, what)
    return want, got


def check_whole(route, eng, res, what):
    v = eng.device_indels()
    assert v.memory == route.mem
    assert (v.n_lib, v.pos0, v.n_pos) == (res.n_lib, res.pos0, res.n_pos), what
    want, got = check_window(route, v, res, 0, res.n_pos, what)
    return v, want, got


# ------------------------------------------------------------------------------------------------ 1. fixtures

def assert_text_fields(res, text, got, per_lib):
    """'%.2f' of the metric columns == the fields of the indel entries the oracle prints (an insertion on its own position's line, a
    deletion on the line of the position behind it; -p: inside the library's block).  Returns the number of entries met."""
    m = len(res.indels)
    met = got["metrics"][:13 * m].reshape(13, m).view(np.float32)
    by_key = {(d["pos"], d["lib"], d["allele"]): r for r, d in enumerate(res.indels)}
    n_entries = 0
    for line in text.decode().splitlines():
        cols = line.split("\t")
        lib = -1
        for entry in cols[4:]:
            f = entry.split(":")
            if len(f) == 1 or f[0] == "":                       # -p: a library's name opens its block ("name\t{" ... "}")
                continue
            if per_lib and f[0].lstrip("{") == "=":
                lib += 1
            a = f[0].lstrip("{")
            if a[0] not in "+-":
                continue
            r = by_key[(int(cols[1]) - 1 if a[0] == "+" else int(cols[1]) - 2, lib if per_lib else 0, a)]
            f[-1] = f[-1].rstrip("}")
            assert len(f) == 14
            for c in range(13):
                x = met[c, r]
                mine = "%d" % int(x) if c in (0, 4, 5, 9) else "%.2f" % float(x)
                assert mine == f[1 + c], (line, a, c, mine)
            assert f[3] == "0.00"
            n_entries += 1
    return n_entries


@pytest.mark.parametrize("per_lib", [False, True], ids=["all_lib", "per_lib"])
def test_golden_fixtures_whole_equal_oracle_and_its_text(route, oracle_lib, test_bam, twolib, per_lib):
    """Both golden fixtures whole, all-lib and -p, with and without -i: every field of every brc_indel the oracle returns, in order
    (the small two-library fixture has no indel: its table is empty), and the printed fields of the indel entries."""
    n_rec = n_ent = 0
    for name, arrs, tid, beg0, end in (("test_bam", test_bam, 20, 10402736, 10405248), ("twolib", twolib, 0, 0, int(twolib["ref"].size))):
        for ic in (False, True):
            opts = dict(insertion_centric=ic)
            if per_lib:
                opts.update(lib_names=[str(s) for s in arrs["lib_names"]], per_lib=True)
            res, text = oracle_result(oracle_lib, arrs, beg0, end, arrs["ref"], tid=tid, chrom="21", **opts)
            eng = computed(route.engine_lib, arrs, beg0, end, arrs["ref"], tid=tid, **opts)
            v, want, got = check_whole(route, eng, res, "%s per_lib=%d ic=%d" % (name, per_lib, ic))
            eng.close()
            n = assert_text_fields(res, text, got, per_lib)
            assert n >= len(res.indels) - 1, (name, n, len(res.indels))      # (a deletion at the region's last position prints nowhere)
            n_rec += len(res.indels); n_ent += n
    assert n_rec >= 8 and n_ent >= 6                              # (test_bam's region holds four indel buckets)


# ------------------------------------------------------------------------------------------------ 2. / 3. ordering under pressure

RL = 3000
LIBS = ["libA", "libB", "libC", "libD"]
CODE = {"=": 0, "A": 1, "C": 2, "G": 4, "T": 8, "N": 15}
X_PREFIX, X_MIXED, X_N, X_ADJ, X_DEEP, NOLIB = 500, 600, 700, 800, 1000, (2000, 2200)


def hand_reads(ref, rows):
    """rows of (pos, [(op, len)], inserted text or None, library): reads that copy the reference except for the inserted bases"""
    a = {k: [] for k in ("pos", "flag", "mapq", "lib", "l_qseq", "n_cigar", "cigar_off", "seq_off", "qual_off", "nm", "sm", "tags")}
    cig, seqs, quals = [], [], []; so = qo = 0
    for pos, ops, ins, lib in rows:
        seq = []; rp = pos
        for o, l in ops:
            if o == 0:
                seq += [CODE.get(chr(ref[rp + j]), 15) if rp + j < len(ref) else 15 for j in range(l)]; rp += l
            elif o == 1:
                seq += [CODE[ch] for ch in ins]
            else:
                rp += l
        L = len(seq)
        a["pos"].append(pos); a["flag"].append(0); a["mapq"].append(60); a["lib"].append(lib); a["l_qseq"].append(L); a["n_cigar"].append(len(ops))
        a["cigar_off"].append(len(cig)); a["seq_off"].append(so); a["qual_off"].append(qo); a["nm"].append(1); a["sm"].append(0); a["tags"].append(1)
        cig += [(l << 4) | o for o, l in ops]
        s4 = np.array(seq + [0] * (L & 1), np.uint8)
        seqs.append(((s4[0::2] << 4) | s4[1::2]).astype(np.uint8)); so += (L + 1) // 2
        quals.append(np.full(L, 30, np.uint8)); qo += L
    out = {k: np.array(v, capi.BATCH_DTYPES[k]) for k, v in a.items()}
    out["cigar"] = np.array(cig, np.uint32); out["seq4"] = np.concatenate(seqs); out["qual"] = np.concatenate(quals)
    return out


def merged(batches):
    """several batches as one, coordinate-sorted (stable)"""
    cat = {}; co = so = qo = 0
    parts = {k: [] for k in capi.BATCH_DTYPES}
    for b in batches:
        for k in capi.BATCH_DTYPES:
            v = np.asarray(b[k])
            if k in ("cigar_off", "seq_off", "qual_off"):
                v = v.astype(np.uint64) + np.uint64({"cigar_off": co, "seq_off": so, "qual_off": qo}[k])
            parts[k].append(v)
        co += len(b["cigar"]); so += len(b["seq4"]); qo += len(b["qual"])
    for k, dt in capi.BATCH_DTYPES.items():
        cat[k] = np.concatenate(parts[k]).astype(dt)
    return capi.select_reads(cat, np.argsort(cat["pos"], kind="stable"))


def ins_read(x, text, lib):
    """a read with `text` inserted behind reference position x"""
    return (x - 19, [(0, 20), (1, len(text)), (0, 20)], text, lib)


def del_read(x, n, lib):
    return (x - 19, [(0, 20), (2, n), (0, 20)], None, lib)


@pytest.fixture(scope="module")
def pressure(oracle_lib):
    """A few thousand reads over 3 kb, four libraries, -p; on top of the generator's indels, hand-made reads for every situation the
    ordering has to get right (asserted on the oracle's list below).  Returns (ref, arrs, opts, oracle result)."""
    rng = np.random.default_rng(11)
    ref = synth.make_ref(rng, RL)
    main = synth.make_batch(2101, ref, 2400, read_len=(60, 120), style="mixed", n_libs=4, p_nolib=0.0)
    nolib = synth.make_batch(2102, ref, 40, read_len=(60, 100), style="simple", n_libs=4, p_nolib=1.0, region=NOLIB, p_flagdrop=0.0)
    rows = [ins_read(X_PREFIX, t, 0) for t in ("A", "AC", "AG", "ACGT", "ACGA", "ACG")]                      # prefixes of one another, differing late
    rows += [ins_read(X_MIXED, "TT", 1)] + [del_read(X_MIXED, n, 1) for n in (1, 2, 5)]                      # an insertion and deletions of several lengths
    rows += [ins_read(X_N, "ANT", 2), ins_read(X_N, "A=T", 2)]                                               # an inserted N (and an '=')
    rows += [(RL - 30, [(0, 25), (2, 12), (0, 5)], None, 3)]                                                 # a deletion running past the reference's end
    rows += [ins_read(X_ADJ, "G", 2), ins_read(X_ADJ + 1, "G", 0), ins_read(X_ADJ + 2, "G", 1), del_read(X_ADJ + 3, 2, 3)]   # adjacent positions, other libraries
    kmers = [a + b + c for a in "ACGT" for b in "ACGT" for c in "ACGT"][5:23]                                # 18 distinct insertion alleles ...
    rows += [ins_read(X_DEEP, t, lib) for lib in range(4) for t in kmers]                                    # ... in each of 4 libraries: 72 records at one position
    arrs = merged([main, nolib, hand_reads(ref, rows)])
    opts = dict(lib_names=LIBS, per_lib=True)
    res, _ = oracle_result(oracle_lib, arrs, 0, RL, ref, **opts)
    return ref, arrs, opts, res


def test_the_pressure_batch_holds_every_situation(pressure):
    ref, arrs, opts, res = pressure
    at = lambda p, l=None: [d["allele"] for d in res.indels if d["pos"] == p and (l is None or d["lib"] == l)]
    assert {"+A", "+AC", "+AG", "+ACG", "+ACGT", "+ACGA"} <= set(at(X_PREFIX, 0))
    mixed = at(X_MIXED, 1)
    assert any(a[0] == "+" for a in mixed) and len({len(a) for a in mixed if a[0] == "-"}) >= 3
    assert "+ANT" in at(X_N, 2) and "+A=T" in at(X_N, 2)
    past = [d for d in res.indels if d["len"] < 0 and d["pos"] + 1 - d["len"] > RL]
    assert past and all(d["allele"].endswith("N") for d in past)
    libs_at = lambda p: {d["lib"] for d in res.indels if d["pos"] == p}
    assert 2 in libs_at(X_ADJ) and 0 in libs_at(X_ADJ + 1) and 1 in libs_at(X_ADJ + 2) and 3 in libs_at(X_ADJ + 3)
    assert res.unavail is not None and (res.unavail != 0xFFFFFFFF).sum() > 50                 # abandoned positions ...
    gone = {res.pos0 + int(k) for k in np.nonzero(res.unavail != 0xFFFFFFFF)[0]}
    assert not [d for d in res.indels if d["pos"] in gone]                                   # ... yield no record
    assert len(at(X_DEEP)) >= 72 > WAVE                                                      # a run longer than a wave
    assert res.n_pos > TILE and len(res.indels) > TILE                                       # both scans: more than one workgroup
    # the oracle's order is the contract's
    keys = [(d["pos"], d["lib"], d["allele"].encode("latin1")) for d in res.indels]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)


@pytest.fixture(scope="module")
def pressed(route, pressure):
    """the pressure batch computed by the route's engine: (engine, view)"""
    ref, arrs, opts, res = pressure
    eng = computed(route.engine_lib, arrs, 0, RL, ref, **opts)
    yield eng, eng.device_indels()
    eng.close()


def test_ordering_under_pressure_whole_region(route, pressure, pressed):
    res = pressure[3]
    v = pressed[1]
    assert v.n_slots >= len(res.indels)
    check_window(route, v, res, 0, res.n_pos, "pressure")


# ------------------------------------------------------------------------------------------------ 4. windows and capacities

def window_list(res):
    """(k0, n): the whole region, k0 off every power-of-two grid, a window without a record, an edge between two records at adjacent
    positions (both sides), the lead position alone, the deep position alone, the last position, an empty window"""
    P = res.n_pos
    has = np.zeros(P, bool); has[[d["pos"] - res.pos0 for d in res.indels]] = True
    empty = int(np.nonzero(~has[300:1900])[0][0]) + 300
    adj = X_ADJ - res.pos0
    assert has[adj] and has[adj + 1] and not has[empty]
    return [(0, P), (37, 301), (empty, 1), (333, adj + 1 - 333), (adj + 1, 259), (0, 1), (X_DEEP - res.pos0, 1), (P - 1, 1), (P - 77, 77), (17, 0), (P, 0)]


def test_windows_equal_the_slices_of_the_oracle_list(route, pressure, pressed):
    res = pressure[3]; v = pressed[1]
    for k0, n in window_list(res):
        check_window(route, v, res, k0, n, "window %r" % ((k0, n),), slack=5)             # capacities above the need: nothing behind the totals is touched
    assert not window_of(res, *window_list(res)[2])


def test_capacities_one_short_and_single_destinations(route, pressure, pressed):
    res = pressure[3]; v = pressed[1]
    k0, n = 37, 301
    want = table_of(window_of(res, k0, n))
    m, nb = want["pos"].shape[1], int(want["alleles"].size)
    assert m > 20
    for cap, acap in ((m - 1, nb), (m, nb - 1), (m - 1, nb - 1), (0, 0), (1, 1)):
        rc, counts, got = gather(route, v, k0, n, cap, acap)
        assert rc == 0 and counts.tolist() == [m, nb], (cap, acap)                         # the true totals, whatever fits
        assert_table(got, want, cap, acap, "cap %d alleles_cap %d" % (cap, acap))
    for k in DESTS:                                                                        # every destination alone, with and without counts
        for with_counts in (True, False):
            rc, counts, got = gather(route, v, k0, n, m, nb, dests=(k,), counts=with_counts)
            assert rc == 0 and counts.tolist() == ([m, nb] if with_counts else [SENT, SENT]), k
            assert_table(got, want, m, nb, k + " alone", dests=(k,))
    assert route.indels.gather_raw(v, k0, n, workspace=None, workspace_bytes=0) == capi.E_ARG      # (even a call that wants nothing needs its scratch)


def test_refused_calls_write_nothing(route, pressure, pressed, test_bam):
    res = pressure[3]; eng, v = pressed
    P = int(v.n_pos)
    early = capi.DeviceIndels()
    e2 = capi.Engine(route.engine_lib)
    idx = capi.fetch_overlapping(test_bam, capi.read_ends(test_bam), 10402999, 10403500)
    e2.begin_region(20, 10403000, 10403500, test_bam["ref"]); e2.push_reads(capi.select_reads(test_bam, idx)); e2.upload()
    assert route.engine_lib.lib.brc_device_indels_get(e2.h, C.byref(early)) == capi.E_ARG        # before a compute
    with pytest.raises(capi.BrcError):
        e2.device_indels()
    e2.close()
    assert route.engine_lib.lib.brc_device_indels_get(None, C.byref(early)) == capi.E_ARG
    assert route.engine_lib.lib.brc_device_indels_get(eng.h, None) == capi.E_ARG

    def altered(**kw):
        w = capi.DeviceIndels.from_buffer_copy(v)
        for k, x in kw.items():
            setattr(w, k, x)
        return w
    other = capi.MEM_HOST if route.mem == capi.MEM_DEVICE else capi.MEM_DEVICE
    need = route.indels.workspace(v, 100)
    assert need > 0 and route.indels.workspace(v, 0) == 0 and route.indels.workspace(None, 100) == 0
    cases = [("no handle", dict(view=v, handle=False)), ("no view", dict(view=None)), ("k0 < 0", dict(view=v, k0=-1)), ("n < 0", dict(view=v, n=-1)),
             ("k0 + n > n_pos", dict(view=v, k0=P - 5, n=6)), ("k0 beyond the positions", dict(view=v, k0=P + 1, n=0)), ("n > n_pos", dict(view=v, k0=0, n=P + 1)),
             ("cap < 0", dict(view=v, cap=-1)), ("alleles_cap < 0", dict(view=v, acap=-1)),
             ("a scratch one byte short", dict(view=v, ws_bytes=need - 1)), ("no scratch", dict(view=v, ws_bytes=0)),
             ("memory of the other kind", dict(view=altered(memory=other))), ("memory 0", dict(view=altered(memory=0))),
             ("another device", dict(view=altered(device=int(v.device) + 1)))]
    for what, kw in cases:
        a = dict(k0=10, n=100, cap=50, acap=200, ws_bytes=None, handle=True); a.update(kw)
        view = a.pop("view")
        if a["ws_bytes"] is None and view is not None and 0 <= a["n"] <= P:
            a["ws_bytes"] = route.indels.workspace(v, a["n"])
        rc, counts, got = gather(route, view, a["k0"], a["n"], a["cap"], a["acap"], ws_bytes=a["ws_bytes"], handle=a["handle"])
        assert rc == capi.E_ARG, what
        assert counts.tolist() == [SENT, SENT], what
        for k in DESTS:
            assert (got[k] == (SENT8 if k == "alleles" else SENT)).all(), "%s: %s was written" % (what, k)
    # n == 0 and a view without slots are fine: counts = {0, 0}, allele_off[0] = 0, nothing else
    for view, k0, n in ((v, 7, 0), (altered(n_slots=0, slots=None), 10, 100)):
        rc, counts, got = gather(route, view, k0, n, 4, 16, ws_bytes=0)
        assert rc == 0 and counts.tolist() == [0, 0]
        assert got["allele_off"][0] == 0 and (got["allele_off"][1:] == SENT).all()
        assert all((got[k] == (SENT8 if k == "alleles" else SENT)).all() for k in DESTS if k != "allele_off")
    assert route.indels.gather_raw(v, 0, 0) == 0


# ------------------------------------------------------------------------------------------------ 5. determinism

def test_two_gathers_are_byte_identical(route, pressure, pressed):
    res = pressure[3]; v = pressed[1]
    m, nb = len(res.indels), sum(len(d["allele"]) for d in res.indels)
    a = gather(route, v, 0, res.n_pos, m, nb)
    b = gather(route, v, 0, res.n_pos, m, nb)
    assert a[0] == 0 and b[0] == 0 and a[1].tolist() == b[1].tolist() == [m, nb]
    for k in DESTS:
        assert a[2][k].tobytes() == b[2][k].tobytes(), k


# ------------------------------------------------------------------------------------------------ 6. text-only engines

def test_view_works_on_text_only_engines_and_after_the_text_was_taken(route, oracle_lib, test_bam):
    beg0, end = 10402736, 10405248
    res, text = oracle_result(oracle_lib, test_bam, beg0, end, test_bam["ref"], tid=20, chrom="21")
    for opts in (dict(text_only=True), dict(device_text="21")):
        eng = computed(route.engine_lib, test_bam, beg0, end, test_bam["ref"], tid=20, **opts)
        check_whole(route, eng, res, "before fetch %r" % opts)
        eng.fetch_result()
        assert eng.format_region("21") == text
        check_whole(route, eng, res, "after the text %r" % opts)
        eng.close()


# ------------------------------------------------------------------------------------------------ 7. knob libraries

def test_indel_records_under_third_allele_pressure(route, oracle_lib, pressure, monkeypatch):
    """The knob libraries with every lane forced to treat bucket 3 as dominant and third-allele lists of one entry (grow and compute
    again): the indel records are the oracle's all the same."""
    monkeypatch.setenv("BRC_FORCE_DOM", "3"); monkeypatch.setenv("BRC_XEV_CAP", "1")
    ref, arrs, opts, res = pressure
    eng = computed(route.knob_lib, arrs, 0, RL, ref, **opts)
    assert eng.device_view().n_xagg > 0
    check_whole(route, eng, res, "knobs")
    eng.close()


# ------------------------------------------------------------------------------------------------ 8. sanitizers

def _serialize(v, calls):
    """the host view of a sim engine as indels_check.cpp reads it"""
    nr, ns = int(v.n_reads), int(v.n_slots)

    def raw(p, nbytes):
        return C.string_at(p, nbytes) if nbytes else b""
    seq_off = np.frombuffer(raw(v.seq_off, 8 * nr), np.uint64); lq = np.frombuffer(raw(v.l_qseq, 4 * nr), np.int32)
    seq_bytes = int((seq_off + ((lq.astype(np.int64) + 1) // 2).astype(np.uint64)).max()) if nr else 0
    b = struct.pack("<iiqQqQqqqii", v.n_lib, v.pos0, v.n_pos, ns, nr, seq_bytes, v.ref_lo, v.ref_hi, v.ref_len, 1 if v.ref else 0, len(calls))
    b += raw(v.slots, 72 * ns) + seq_off.tobytes() + lq.tobytes() + raw(v.seq4, seq_bytes) + (raw(v.ref, v.ref_hi - v.ref_lo) if v.ref else b"")
    for c in calls:
        b += struct.pack("<qqqq", *c)
    return b


def test_windows_under_the_host_sanitizers(pressure, sim_lib, tmp_path):
    """The window list on the CPU build with -fsanitize=address,undefined: sources of exactly the view's sizes, a scratch of exactly
    brc_indels_workspace bytes and destinations of exactly the contract's sizes on the heap — a load or store outside them is a
    report — exact capacities and capacities one short; the results are the oracle's."""
    checker = side.sim_checker(side.SIDE["indels"])
    ref, arrs, opts, res = pressure
    eng = computed(sim_lib, arrs, 0, RL, ref, **opts)
    v = eng.device_indels()
    assert v.memory == capi.MEM_HOST and v.n_slots > 0
    calls = []
    for k0, n in window_list(res):
        w = window_of(res, k0, n); m = len(w); nb = sum(len(d["allele"]) for d in w)
        calls.append((k0, n, m, nb))
        if m:
            calls.append((k0, n, m - 1, nb - 1))
    open(tmp_path / "case.bin", "wb").write(_serialize(v, calls))
    eng.close()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([checker, str(tmp_path / "case.bin"), str(tmp_path / "res.bin")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    assert p.stdout.decode().strip() == "%d calls" % len(calls)
    d = np.fromfile(tmp_path / "res.bin", np.uint8); o = 0
    for k0, n, cap, acap in calls:
        want = table_of(window_of(res, k0, n))
        assert d[o:o + 4].view(np.int32)[0] == 0; o += 4
        assert d[o:o + 8].view(np.uint32).tolist() == [want["pos"].shape[1], want["alleles"].size]; o += 8
        got = {}
        for k in DESTS:
            nbytes = acap if k == "alleles" else 4 * (cap + 1 if k == "allele_off" else PLANES[k] * cap)
            got[k] = d[o:o + nbytes] if k == "alleles" else d[o:o + nbytes].view(np.uint32); o += nbytes
        assert_table(got, want, cap, acap, "asan %r" % ((k0, n, cap, acap),))
    assert o == d.size


# ------------------------------------------------------------------------------------------------ 9. the Python interface

def test_tensors_indels(route, pressure, pressed):
    """bam_readcount_amd.tensors.indels: shapes, dtypes, device, values, windows in reference coordinates, an empty window; [hip]: the
    tensors lie on the engine's device and a torch reduction queued right behind the call sees them."""
    from bam_readcount_amd import tensors
    res = pressure[3]; eng, v = pressed
    want = table_of(res.indels)
    m, nb = len(res.indels), int(want["alleles"].size)

    def host(a):
        return a.cpu().numpy() if route.name == "hip" else a
    t = tensors.indels(eng, route.indels)
    assert (t["m"], t["first"], t["n"]) == (m, res.pos0, res.n_pos)
    if route.name == "hip":
        torch = route.torch
        assert all(t[k].is_cuda and t[k].device.index == int(v.device) for k in tensors.INDEL_KINDS)
        total = t["istat"][0].to(torch.int64).sum()                       # queued on the stream the gather was queued on: no wait in between
        assert int(total) == int(want["istat"][0].astype(np.int64).sum())
        assert (t["pos"].dtype, t["rep_read"].dtype, t["fstat"].dtype, t["alleles"].dtype) == (torch.int32, torch.uint32, torch.float32, torch.uint8)
    else:
        assert all(isinstance(t[k], np.ndarray) for k in tensors.INDEL_KINDS)
    for k in tensors.INDEL_KINDS:
        shape, dt = tensors.indel_shapes(m, nb)[k]
        assert tuple(t[k].shape) == shape and host(t[k]).dtype == dt, k
        assert np.array_equal(host(t[k]).view(np.uint8 if k == "alleles" else np.uint32).reshape(want[k].shape), want[k]), k
    text = bytes(host(t["alleles"])); off = host(t["allele_off"])
    assert [text[off[r]:off[r + 1]].decode("latin1") for r in range(m)] == [d["allele"] for d in res.indels]
    # a window in reference coordinates, a subset of the kinds
    lo, hi = res.pos0 + 450, res.pos0 + 1100
    w = tensors.indels(eng, route.indels, beg0=lo, end=hi, want=("pos", "len", "metrics"))
    sub = table_of([d for d in res.indels if lo <= d["pos"] < hi])
    assert (w["first"], w["n"], w["m"]) == (lo, hi - lo, sub["pos"].shape[1]) and "alleles" not in w and w["m"] > 72
    for k in ("pos", "len", "metrics"):
        assert np.array_equal(host(w[k]).view(np.uint32).reshape(sub[k].shape), sub[k]), k
    c = tensors.indels(eng, route.indels, beg0=-5, end=10 ** 9, want=("lib",))
    assert c["m"] == m and c["n"] == res.n_pos
    e = tensors.indels(eng, route.indels, beg0=res.pos0 + res.n_pos + 5)
    assert (e["m"], e["n"]) == (0, 0) and tuple(e["pos"].shape) == (0,) and tuple(e["metrics"].shape) == (13, 0) and tuple(e["allele_off"].shape) == (1,)
    assert int(host(e["allele_off"])[0]) == 0
    with pytest.raises(ValueError):
        tensors.indels(eng, route.indels, want=("nonsense",))
