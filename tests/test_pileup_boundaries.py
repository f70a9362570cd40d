"""k_pileup2 at the boundaries of its own pipeline, on columns constructed by hand (no make_batch, no random batch): pieces per tile
across every multiple of HALF with every kind of piece on every step of both ring halves (A), the deferred queue at its bound (B), flushes
before and after huge pieces with dead lanes and a partial last tile (C), a column deeper than 65 535 reads (D) and every alignment of a
staged window (E).  Every batch is compared with the oracle bit for bit and byte for byte (parity.compare_libs) on three routes: the
bounds-checked build (libbrc_hip_checked.so — a violation record fails the call), then the product ([hip]; the knob builds through
libbrc_hip_testknobs.so), and the CPU lane simulator ([sim]) so that the CPU suite runs every body.

No test can see from outside which path a piece took, so every test first runs its batch through the simulator with the COVERAGE WITNESS on
(tests/sim/brc_sim.cpp: brc_sim_witness) and asserts the cells the batch was built to hit: pieces by (kind, step J, ring half), the most queue
entries of a half-batch as the device counts them, flushes per tile and those started inside the drain, the most pieces / half-batches /
columns of a tile, the parity of the tiles' first piece, and that no staged window leaves the padded stream.  The witness speaks for the
device because both backends take table_len, flush_k, pack_lim and pack_shift from the same host functions — Staged::modal_len and
choose_pack, called by HipBackend::upload (brc_engine.hip) and SimBackend::upload (brc_sim.cpp) alike — and cut the same tile ranges
(tile_range2, k_mask_tiles' trimming); the record repeats the four values and the tests assert them.

Third-allele events are held to at most XEV_CAP per (tile, library) bucket in every batch here: fold_xev_bucket is quadratic on one lane
(ADVICE.md), and this file stays clear of it."""
import ctypes
import json

import numpy as np
import pytest

import parity
from bam_readcount_amd import capi
from constructed import OTHER, THIRD, Reads, ACGT_CODE, chain, checked_lib, mismatches, ref_of  # noqa: F401  (checked_lib: fixture)

HALF = 12                        # brc_core.h: BRC_HALF (the witness repeats it; asserted)
QCAP = 3 * HALF + 2              # brc_engine.hip
XEV_CAP = 512

class Case:
    def __init__(self, ref, arrs, regions, witness, opts=None, env=None, names=(), windows=None, check_warn=True):
        self.ref, self.arrs, self.regions, self.witness = ref, arrs, regions, witness
        self.opts, self.env, self.names, self.windows, self.check_warn = opts or {}, env or {}, names, windows, check_warn


def fillers(R, pos, n):
    """plain reads that make 100 the modal length of the region"""
    for k in range(n):
        R.add(pos, [(0, 100)], flag=(0, 16)[k & 1])


# ------------------------------------------------------------------------------------------------ A. pieces per tile x kind x step

A_COUNTS = list(range(0, 3 * HALF + 3)) + [4 * HALF - 1, 4 * HALF, 4 * HALF + 1] + [43, 44, 45, 32, 51, 57]   # (the last six: see case_a)
FORMS = ([(0, 100)], [(0, 70)], [(4, 100), (0, 100), (4, 100)])       # modal length, another length (in-lane division), a length with a rare record
LONG = [(4, 250), (0, 100), (4, 250)]                                 # 600 bases, soft-clipped to the cluster's own tiles


def a_read(R, T, i, j, n, with_i, n_libs):
    K = 11 if with_i else 10
    kind = (i + j) % K; form = FORMS[((i + j) // K) % 3]
    s = T + (j * 64) // n                                           # starts spread over the tile, in read order
    flag = (0, 16, 99, 147)[(i + j) % 4]
    kw = dict(flag=flag, nm=j % 4, sm=(7 * j) % 60, tags=(3, 3, 1, 2)[(i + 2 * j) % 4], lib=(0, 0, 0, 1, 1, 2)[j % 6] if n_libs > 1 else 0)
    snv = mismatches([1], OTHER) if j % 3 == 1 else mismatches([1], THIRD) if j % 5 == 2 else None
    if kind == 0:
        R.add(s, [(0, 100)], edit=snv, **kw)
    elif kind == 1:
        R.add(s, [(4, 10), (0, 90)], edit=snv, **kw)               # a left clip alone keeps q2 == tp: every term but one from the tables
    elif kind == 2:
        R.add(s, [(0, 70)], edit=snv, **kw)
    elif kind == 3:
        R.add(s, FORMS[2], edit=snv, **kw)
    elif kind == 4:                                                 # reverse, Q2 run of three at the head, behind it the clip: q2 = 2, tp = 10
        def q2run(seq, qual, aq, ar, code):
            qual[:3] = 2
        R.add(s, [(4, 10), (0, 90)], edit=chain(snv, q2run), **dict(kw, flag=16 | (flag & 3)))
    elif kind == 5:
        def quals(seq, qual, aq, ar, code):
            qual[aq[:3]] = [0, 63, 93]; qual[aq[40]] = (0, 63, 93)[j % 3]
        R.add(s, form, edit=chain(snv, quals), **kw)
    elif kind == 6:
        def nbase(seq, qual, aq, ar, code):
            seq[aq[0]] = 15; seq[aq[30]] = 15
            if j & 1:
                seq[aq[2]] = 0
        R.add(s, form, edit=chain(snv, nbase), **kw)
    elif kind == 7:                                                 # a mismatch-quality sum above every pack_lim of a short-read region
        R.add(s, LONG if (i + j) // K % 2 == 0 else [(0, 100)], edit=mismatches(range(0, 100, 2), OTHER, q=40), **kw)
    elif kind == 8:
        R.add(s, [(0, 100)], edit=snv, **dict(kw, mapq=5))
    elif kind == 9:
        R.add(s, [(0, 40), (2, 30), (0, 60)], edit=snv, **kw)
    else:
        R.add(s, [(0, 50), (1, 2), (0, 48)], edit=snv, **kw)


def need_cells(w, kinds, what, per_half=True):
    """every kind on every step of both ring halves (per_half=False: on every step, and in both halves)"""
    for kind in kinds:
        cells = np.zeros(2 * HALF, np.int64)
        for name, v in w["pieces"].items():
            if name == kind or ("+" + kind) in name:
                cells += np.asarray(v)
        if not per_half:
            assert cells[HALF:].any(), (what, kind)
            cells = cells[:HALF] + cells[HALF:]
        assert cells.all(), "%s: no piece of kind %r on (ring half, step) %s" % (what, kind, [(int(x) // HALF, int(x) % HALF) for x in np.nonzero(cells == 0)[0]])


def case_a(variant):
    """42 + 6 clusters 256 positions apart (a workgroup's four tiles each); cluster i holds A_COUNTS[i] reads that start inside its first
    tile, read j of kind (i + j) mod K.  Reads longer than 100 bases are soft-clipped to 100 aligned ones and the deletion read spans 130, so
    no cluster reaches its neighbour's tiles.  A deletion read is two pieces (an insertion read under -i: three) and -p deals a cluster's
    reads to three streams, so the PIECES of a (tile, library) do not step through every count its reads do: the six clusters appended to
    the list bring the counts the sweep steps over — 4 HALF - 1, 4 HALF, 4 HALF + 1 with one library; 2 HALF and 3 HALF with three (the
    witness's tile_pieces asserts every count named below)."""
    with_i = variant == "libs3_i"; n_libs = 3 if with_i else 1
    ref = ref_of(256 * (len(A_COUNTS) + 2) + 7000)
    R = Reads(ref)
    for i, n in enumerate(A_COUNTS):
        for j in range(n):
            a_read(R, 256 * (i + 1), i, j, n, with_i, n_libs)
    end = 256 * (len(A_COUNTS) + 1)
    if variant == "long":
        R.add(end + 300, [(0, 6000)]); end += 6400
    opts = dict(min_mapq=20, min_bq=5)
    names = ()
    if with_i:
        opts.update(per_lib=True, insertion_centric=True); names = ["libA", "libB", "libC"]
    windows = None
    if variant == "windows":                                        # lanes 0 / 63 (and lane 0 of the next tile) / 1-62 / none of a cluster's first tile
        windows = []
        for i in range(len(A_COUNTS)):
            T = 256 * (i + 1)
            if i % 4 != 3:
                windows.append(((T, T + 1), (T + 64, T + 65), (T + 2, T + 63))[i % 4])

    w_tiles_all = (end // 64 + 1) * n_libs

    def witness(w):
        assert w["table_len"] == 100 and w["pack_shift"] == (12 if variant == "long" else 16) and not w["stage_fault"]
        assert w["windows"] == (variant == "windows")
        kinds = ["table", "tabq", "div", "rare", "eventless", "ext", "wide"] + (["nb"] if with_i else []) + (["huge"] if variant != "long" else [])
        if variant != "windows":                                    # (announced windows trim the ranges: the steps move, the sweep below is the other variants')
            need_cells(w, kinds, variant, per_half=not with_i)      # (-p deals the reads to three streams: few tiles of one library reach the second half)
            got = {int(k) for k in w["tile_pieces"]}
            want = {1, HALF - 1, HALF, HALF + 1, 2 * HALF - 1, 2 * HALF, 2 * HALF + 1, 3 * HALF} | (set() if with_i else {4 * HALF - 1, 4 * HALF, 4 * HALF + 1})
            assert want <= got, (variant, sorted(want - got))
            assert w["tiles"] < w_tiles_all                         # (and tiles without a piece: count 0)
        combos = ["tabq+wide", "div+wide", "rare+wide"] + (["tabq+huge", "rare+huge"] if variant != "long" else [])
        assert all(k in w["pieces"] for k in combos), (variant, sorted(w["pieces"]))
        assert w["lo_parity"][0] > 0 and w["lo_parity"][1] > 0, w["lo_parity"]
        assert 1 <= w["queue_max"] <= QCAP
    return Case(ref, R.arrays(), [(1, end)], witness, opts=opts, names=names, windows=windows)


# ------------------------------------------------------------------------------------------------ B. the queue at its bound

def case_b(knob):
    """cluster k (k = 0 .. HALF - 1): a plain read that makes `other` the alternate bucket at b, k plain reads, then 2 HALF reads that are
    wide and huge with an N at a and a third base at b — three queue entries each, the run starting on step k + 1.  Without a knob the run
    is 600-base reads (rare record + huge); with BRC_PACK_LIM=255 modal-length reads whose mismatch-quality sum of 320 is huge only then."""
    ref = ref_of(256 * (HALF + 3))
    R = Reads(ref)

    def run_edit(seq, qual, aq, ar, code):
        offs = np.arange(0, 100, 2) if not knob else np.array([4, 10, 20, 30, 40, 50, 60, 70])
        seq[aq[offs]] = OTHER[code[ar[offs]]]; qual[aq[offs]] = 40
        seq[aq[20]] = 15; seq[aq[40]] = THIRD[code[ar[40]]]
    for k in range(HALF):
        T = 256 * (k + 1)
        R.add(T, [(0, 100)], edit=mismatches([40], OTHER))
        for _ in range(k):
            R.add(T, [(0, 100)])
        for j in range(2 * HALF):
            R.add(T, [(0, 100)] if knob else LONG, edit=run_edit, flag=(0, 16)[j & 1])
    fillers(R, 256 * (HALF + 1), 2 * HALF * HALF)

    def witness(w):
        assert w["table_len"] == 100 and not w["stage_fault"]
        assert w["pack_lim"] == (255 if knob else 65535 // max(w["flush_k"], HALF))
        assert w["queue_max"] == 3 * HALF and w["queue_max"] <= QCAP
        need_cells(w, ["tabq+wide+huge" if knob else "rare+wide+huge"], "queue")          # the run starts on every step
    n_third = 2 * HALF                                              # per tile: one event of every run read at b (and its N at a)
    assert 2 * n_third <= XEV_CAP
    return Case(ref, R.arrays(), [(1, 256 * (HALF + 2))], witness, env={"BRC_PACK_LIM": "255"} if knob else None)


# ------------------------------------------------------------------------------------------------ C. flush and final store

def flush_k_of(sim_lib, max_len):
    """flush_k as choose_pack returns it for a region whose longest read has max_len bases (through the witness: no literal here)"""
    ref = ref_of(2000)
    R = Reads(ref); R.add(100, [(0, 100)]); R.add(100, [(0, 100)]); R.add(300, [(0, max_len)])
    sim_lib.lib.brc_sim_witness(1)
    parity.run_engine(sim_lib, R.arrays(), [(1, 1500)], ref=ref)
    return witness_of(sim_lib)[0]["flush_k"]


def case_c(variant, flush_k):
    """one column of 3 flush_k + 5 pieces, all starting on the tile's first position; a huge piece before the first regular flush (the
    drain flushes for it) and one after it"""
    ref = ref_of(4096)
    R = Reads(ref)
    T = 1024; n = 3 * flush_k + 5
    huge_at = (5, flush_k + 20)
    for j in range(n):
        kw = dict(flag=(0, 16, 99, 147)[j % 4], nm=j % 5, sm=(11 * j) % 60)
        if j in huge_at:
            R.add(T, [(0, 100)], edit=mismatches(range(0, 100, 2), OTHER, q=40), **kw)
        else:
            R.add(T, [(0, 100)], edit=mismatches([j % 64], OTHER) if j % 4 == 1 else mismatches([(3 * j) % 64], THIRD) if j % 9 == 2 else None, **kw)
    opts, names, end, check_warn = {}, (), 2048, True
    if variant == "nolib":                                          # a library-less read abandons lanes 30 .. 49 of the flushed tile
        R.add(T + 30, [(0, 20)], lib=-1); opts = dict(per_lib=True); names = ["libA", "libB"]; check_warn = False
    if variant == "partial":
        end = T + 37                                                # the region ends inside the flushed tile

    def witness(w):
        assert w["table_len"] == 100 and w["flush_k"] == flush_k and not w["stage_fault"]
        assert w["flush_in_drain"] >= 1 and w["flush_regular"] >= 2 and w["flush_max"] >= 3
        assert w["pieces_max"] >= n
        assert "tabq+huge" in w["pieces"]
    return Case(ref, R.arrays(), [(1, end)], witness, opts=opts, names=names, check_warn=check_warn)


# ------------------------------------------------------------------------------------------------ D. a column deeper than 65 535

def case_d(two_libs):
    """70 000 reads of 100 bases with starts spread over one tile, every seventh carrying a second allele throughout; every 150th a third
    allele at its eleventh base (counted: at most XEV_CAP per bucket).  Built vectorised."""
    n, L, T = 70_000, 100, 1024
    ref = ref_of(2048); code = ACGT_CODE[ref]
    starts = np.sort(np.random.default_rng(1).integers(T, T + 64, n)).astype(np.int32)
    seq = code[starts[:, None] + np.arange(L)[None, :]]
    seq[::7] = OTHER[seq[::7]]
    third = np.arange(n) % 150 == 3
    seq[third, 10] = THIRD[code[starts[third] + 10]]
    lib = np.zeros(n, np.int16)
    if two_libs:
        lib[np.arange(n) % 35 == 17] = 1; lib[np.nonzero(lib == 0)[0][66_000:]] = 1
        assert (lib == 0).sum() == 66_000 and (lib == 1).sum() == 4_000
    for l in range(2 if two_libs else 1):                           # third-allele events per (tile, library) bucket
        k = (starts[third & (lib == l)] + 10) // 64
        assert np.bincount(k).max() <= XEV_CAP
    ar = np.arange(n)
    arrs = dict(pos=starts, flag=np.where(ar % 3 == 0, 16, 0), mapq=np.array([60, 47, 29])[ar % 3], lib=lib, l_qseq=np.full(n, L), n_cigar=np.ones(n),
                cigar_off=ar, seq_off=ar * (L // 2), qual_off=ar * L, nm=ar % 5, sm=(ar * 7) % 61, tags=np.full(n, 3), cigar=np.full(n, L << 4),
                seq4=((seq[:, 0::2] << 4) | seq[:, 1::2]).reshape(-1), qual=(20 + (ar[:, None] + 3 * np.arange(L)[None, :]) % 21).reshape(-1))
    arrs = {k: np.asarray(arrs[k]).astype(dt) for k, dt in capi.BATCH_DTYPES.items()}

    def witness(w):
        assert w["table_len"] == 100 and not w["stage_fault"]
        assert w["ncol_max"] >= 65_536 and w["halves_max"] > 5_000
    return Case(ref, arrs, [(900, 1300)], witness, opts=dict(per_lib=True) if two_libs else None, names=["libA", "libB"] if two_libs else ())


# ------------------------------------------------------------------------------------------------ E. window alignment

def case_e():
    """reads of 1 .. 100 bases starting on each of the 64 lanes of a tile: every (p0 - a) & 15 with piece ends on lanes 0, 1, 62, 63; the
    arena's first read starts on lane 63 (of the tile before), its last read (two bases from lane 63) ends on lane 0"""
    ref = ref_of(4096)
    R = Reads(ref)
    T = 1024
    fillers(R, T - 1, 80)
    for s in range(64):
        for L in (1, 15, 16, 17, 63, 64, 65, 100, 2):
            R.add(T + s, [(0, L)], flag=(0, 16)[(s + L) & 1], edit=mismatches([0], OTHER) if (s + L) % 5 == 0 else None)
    arrs = R.arrays()
    assert arrs["pos"][0] % 64 == 63 and arrs["qual_off"][0] == 0
    assert (arrs["pos"][-1] + arrs["l_qseq"][-1] - 1) % 64 == 0 and arrs["qual_off"][-1] == arrs["qual_off"].max()

    def witness(w):
        assert w["table_len"] == 100 and not w["stage_fault"]
        assert "div" in w["pieces"] and "table" in w["pieces"]
    return Case(ref, arrs, [(1, 2048)], witness)


# ------------------------------------------------------------------------------------------------ the cases and the routes

BUILDERS = {
    "A-one_library": lambda sim: case_a("one"), "A-three_libraries-i": lambda sim: case_a("libs3_i"), "A-windows": lambda sim: case_a("windows"),
    "A-long_read_SH12": lambda sim: case_a("long"),
    "B-queue-600_bases": lambda sim: case_b(False), "B-queue-PACK_LIM_255": lambda sim: case_b(True),
    "C-flush-huge_before_and_after": lambda sim: case_c("plain", flush_k_of(sim, 100)), "C-flush-dead_lanes": lambda sim: case_c("nolib", flush_k_of(sim, 100)),
    "C-flush-partial_last_tile": lambda sim: case_c("partial", flush_k_of(sim, 100)),
    "D-deep-one_library": lambda sim: case_d(False), "D-deep-two_libraries": lambda sim: case_d(True),
    "E-window_alignment": lambda sim: case_e(),
}
PLAIN = [k for k in BUILDERS if "PACK_LIM" not in k]
KNOBS = [k for k in BUILDERS if "PACK_LIM" in k]
_cases = {}


def witness_of(sim_lib):
    f = sim_lib.lib.brc_sim_witness; f.restype = ctypes.c_char_p
    return json.loads(f(0).decode())


def prepared(name, sim_lib, monkeypatch):
    """the case, built once; its batch through the simulator with the witness on, the cells it was built to hit asserted — before anything
    goes to another route"""
    if name not in _cases:
        _cases[name] = BUILDERS[name](sim_lib)
    case = _cases[name]
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    if not hasattr(case, "seen"):
        sim_lib.lib.brc_sim_witness.restype = ctypes.c_char_p
        sim_lib.lib.brc_sim_witness(1)
        run(sim_lib, case)
        (w,) = witness_of(sim_lib)
        assert w["half"] == HALF
        case.witness(w)
        case.seen = w
    return case


def run(lib, case):
    kw = dict(ref=case.ref, lib_names=case.names, **case.opts)
    if case.windows is None:
        return parity.run_engine(lib, case.arrs, case.regions, **kw)
    # announced windows (the WINDOWS instantiation): the text of every window, and the planes at the positions the windows ask for
    (beg0, end), = case.regions
    eng = capi.Engine(lib, lib_names=case.names, **case.opts)
    try:
        eng.begin_region(0, beg0, end, case.ref); eng.push_reads(case.arrs)
        eng.region_windows(np.array([w[0] for w in case.windows], np.int32), np.array([w[1] for w in case.windows], np.int32))
        res = eng.end_region()
        asked = np.zeros(res.n_pos, bool)
        for b, e in case.windows:
            asked[b - 1 - res.pos0:e - res.pos0] = True
        return b"".join(eng.format_window("chrS", b, e, 0) for b, e in case.windows), [res.ncol[..., asked], res.depth[..., asked], res.istat[..., asked], res.fstat[..., asked].view(np.uint32)]
    finally:
        eng.close()


def check(lib, oracle_lib, case):
    if case.windows is None:
        text, _ = parity.compare_libs(lib, oracle_lib, case.arrs, case.regions, check_warn=case.check_warn, ref=case.ref, lib_names=case.names, **case.opts)
        assert text.count(b"\n") > 30
        return
    if not hasattr(case, "want"):                                   # the reference: every window a region of its own (its text), and the whole region (its planes)
        kw = dict(ref=case.ref, lib_names=case.names, **case.opts)
        text, _ = parity.run_engine(oracle_lib, case.arrs, case.windows, **kw)
        _, (res,) = parity.run_engine(oracle_lib, case.arrs, case.regions, **kw)
        asked = np.zeros(res.n_pos, bool)
        for b, e in case.windows:
            asked[b - 1 - res.pos0:e - res.pos0] = True
        case.want = text, [res.ncol[..., asked], res.depth[..., asked], res.istat[..., asked], res.fstat[..., asked].view(np.uint32)]
    got_text, got_planes = run(lib, case)
    assert got_text == case.want[0] and got_text.count(b"\n") > 30
    for g, w in zip(got_planes, case.want[1]):
        np.testing.assert_array_equal(g, w)


# (the checked route stands first: in file order, and in the GPU job, the product runs a batch only after the bounds-checked build did)
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BUILDERS))
def test_checked_build_reports_no_violation(checked_lib, sim_lib, oracle_lib, monkeypatch, name):
    check(checked_lib, oracle_lib, prepared(name, sim_lib, monkeypatch))


@pytest.mark.parametrize("name", PLAIN)
def test_constructed_columns_equal_oracle(dev_lib, sim_lib, oracle_lib, monkeypatch, name):
    check(dev_lib, oracle_lib, prepared(name, sim_lib, monkeypatch))


@pytest.mark.parametrize("name", KNOBS)
def test_constructed_columns_equal_oracle_under_knobs(knob_lib, sim_lib, oracle_lib, monkeypatch, name):
    check(knob_lib, oracle_lib, prepared(name, sim_lib, monkeypatch))
