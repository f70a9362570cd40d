"""The device's text (BRC_OPT_DEVICE_TEXT: k_text_len, the 32-bit scan, k_text_total, k_text_write running text_line of brc_core.h;
k_last_processed; the side tables k_indel_reduce and k_xev_fold leave; prepare_text_queues and format_device_text of brc_host.cpp) at the
formatter's own boundaries, on lines constructed by hand (constructed.Reads; no make_batch, no random batch): numbers (A), where a bucket's
sums come from (B), indel entries (C), the geometry of lengths, offsets, total and last processed column (D) and the host side across
regions (E).  Every case is compared with the oracle byte for byte through device_text="chrS" and through text_only=True, on the CPU lane
simulator ([sim]) and the product ([hip]; the knob builds through libbrc_hip_testknobs.so).

What no test can see from outside — which of the two slots or the third-allele table a printed bucket came from — the simulator's TEXT
WITNESS reports (tests/sim/brc_sim.cpp: brc_sim_text_witness), and family B asserts the cells its batch was built to hit.  The witness
speaks for the device because both backends build the same planes and tables (the parity tests hold that) and this file compares the
text of both.

Third-allele events are held to at most XEV_CAP per (tile, library) bucket in every batch here (fold_xev_bucket is quadratic on one lane,
ADVICE.md); no region has more than about 10 000 planes or a few thousand reads."""
import ctypes
import json
import re
from fractions import Fraction

import numpy as np
import pytest

from bam_readcount_amd import capi
from constructed import OTHER, THIRD, Reads, mismatches, queue_expectations, queue_scenarios, ref_of, run_steps

XEV_CAP = 512
SCAN_CHUNK = 4096                # brc_engine.hip
CODE = {"A": 1, "C": 2, "G": 4, "T": 8, "N": 15, "=": 0}
ROUTES = (dict(device_text="chrS"), dict(text_only=True))
_want = {}
SIM = None


@pytest.fixture(autouse=True)
def _simulator(sim_lib):
    """every test of this file may ask the simulator's witness about its batch (third_events_ok), the [hip] ids included"""
    global SIM
    SIM = sim_lib


def oracle(oracle_lib, key, steps, **kw):
    """the oracle's texts and results of a scenario, computed once"""
    if key not in _want:
        _want[key] = run_steps(oracle_lib, steps, **kw)
    return _want[key]


def without_planes(r):
    """The route, seen from outside: a result whose text the device wrote carries no planes (brc_fetch_result) — no reference characters, no
    plane of abandoned positions.  A region the backend handed back (the scan's entry P disagrees with k_text_total's 64-bit sum, or the
    total is over the limit) is formatted by the host from planes, and its bytes alone would not tell.  (A region without a plane, as a
    piece inside an empty stretch is, shows nothing either way: None.)"""
    if r.n_pos == 0:
        return None
    return r.refbase == b"" and r.unavail is None


def assert_routes(key, route, got_res, on_device=True):
    """every region of a device_text run was written by the device (on_device: one flag for all steps, or one per step); no region of a
    text_only run was"""
    flags = [without_planes(r) for r in got_res]
    if "device_text" in route:
        expect = list(on_device) if isinstance(on_device, (list, tuple)) else [on_device] * len(got_res)
        expect = [x if f is not None else None for x, f in zip(expect, flags)]
        assert flags == expect, "%s: device-written regions %r, expected %r (a region was handed back to the host's formatter)" % (key, flags, expect)
    else:
        assert not any(flags), (key, route, flags)


def check(lib, oracle_lib, key, steps, routes=ROUTES, on_device=True, **kw):
    want, res = oracle(oracle_lib, key, steps, **kw)
    third_events_ok(key, res, steps, **kw)
    for route in routes:
        got, got_res = run_steps(lib, steps, **route, **kw)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, "%s %r: the text of step %d differs" % (key, route, i)
        assert [r.n_pos for r in got_res] == [r.n_pos for r in res]
        assert_routes(key, route, got_res, on_device)
    return want, res


def text_witness(sim_lib, steps, **kw):
    f = sim_lib.lib.brc_sim_text_witness; f.restype = ctypes.c_char_p
    f(1)
    try:
        run_steps(sim_lib, steps, device_text="chrS", **kw)
        return json.loads(f(0).decode())
    finally:
        f(-1)


def base_events_max(res):
    """the most base events of one (tile, library) of a result, from the oracle's dense planes: a bound on the events of its third-allele
    list whatever the order the bases arrived in (the slots belong to the first two distinct bases to arrive, not to the largest buckets;
    N and '=' events always go to the list — so nothing short of every event bounds the list without the arrival order)"""
    n = res.istat[:, :, 0, :].astype(np.int64).sum(axis=1)          # [L][P]
    pad = (-n.shape[1]) % 64
    return int(np.pad(n, ((0, 0), (0, pad))).reshape(n.shape[0], -1, 64).sum(axis=2).max(initial=0))


def third_events_ok(key, res, steps, **kw):
    """The hard limit of this file, asserted for EVERY batch (check() calls it): no (tile, library) bucket lists more than XEV_CAP third-
    allele events.  Where a tile's base events are no more than that, the planes prove it.  A deeper batch needs the count itself: the
    simulator's witness reports the longest (tile, library) list as the device builds it, in arrival order ("xev_bucket_max")."""
    if max(base_events_max(r) for r in res) <= XEV_CAP:
        return
    if key + "x" not in _want:
        ws = text_witness(SIM, steps, **kw)
        assert len(ws) == len(res)
        _want[key + "x"] = max(w["xev_bucket_max"] for w in ws)
        print("%s: up to %d base events in a (tile, library), of them at most %d on its third-allele list" % (key, max(base_events_max(r) for r in res), _want[key + "x"]))
    assert _want[key + "x"] <= XEV_CAP, (key, _want[key + "x"])


def lines_of(text):
    return [l.split(b"\t") for l in text.split(b"\n") if l]


# ------------------------------------------------------------------------------------------------ A. numbers

A1_DEPTHS = [3, 7, 8, 8, 8, 9, 10, 11, 16, 24, 40, 40, 40, 99, 100, 101, 125, 200]
FLOAT_FIELDS = ((1, "i", 1), (2, "i", 8), (3, "i", 2), (6, "f", 0), (7, "f", 2), (8, "i", 6), (10, "q2", 1), (11, "i", 7), (12, "f", 3))   # printed field -> plane (capi.I_NAMES / F_NAMES)


def case_a1():
    """clusters 128 positions apart, cluster i of A1_DEPTHS[i] reads of 30 aligned bases that all start on one position: one column depth
    each.  Map quality, base quality, clip lengths, NM, SM and strand step through residues of the read's and the column's number; which reads
    carry the second base depends on the column, so that every column splits its depth over the buckets differently."""
    ref = ref_of(128 * (len(A1_DEPTHS) + 2))
    R = Reads(ref)
    for i, d in enumerate(A1_DEPTHS):
        T = 128 * (i + 1)
        for j in range(d):
            lc, rc = (j * (i + 1)) % 8, (j * 3 + i) % 5
            ops = ([(4, lc)] if lc else []) + [(0, 30)] + ([(4, rc)] if rc else [])

            def edit(seq, qual, aq, ar, code, i=i, j=j):
                cols = np.arange(30)
                qual[aq] = 2 + (j * (cols + 1 + i) + cols * cols) % 39
                alt = ((j + 1) * (cols + 2 + i)) % 5 == 0
                seq[aq[alt]] = OTHER[code[ar[alt]]]
                third = (cols % 3 == (j // 17) % 3) & (j % 17 == 5)
                seq[aq[third]] = THIRD[code[ar[third]]]
            R.add(T, ops, flag=(0, 16, 99, 147)[(j + i) % 4], mapq=(j * 7 + i) % 61, nm=(j * (i + 2)) % 7, sm=(j * 5 + i) % 41, edit=edit)
    return ref, R.arrays(), (1, 128 * (len(A1_DEPTHS) + 1))


def py_f2(num, den):
    """'%.2f' of the fp32 quotient: CPython's correctly rounded conversion of the exact binary value"""
    return "%.2f" % float(np.float32(num) / np.float32(den))


def test_a1_rounding_ties_and_one_ulp_boundaries(dev_lib, oracle_lib):
    """A1.  On top of byte equality: every float field of the six base buckets recomputed from the oracle's dense planes with a formatter
    that shares nothing with the C++ ones; the batch must hold at least 200 exact ties (value x 100 has fractional part 1/2 as a Fraction)
    and at least 400 fields whose text changes when the quotient moves one ulp either way — counted here from the oracle's planes alone."""
    ref, arrs, region = case_a1()
    (want,), (res,) = oracle(oracle_lib, "A1", [(arrs, region)], ref=ref)
    ties = ulps = fields = 0
    depths = set()
    for tok in lines_of(want):
        k = int(tok[1]) - 1 - res.pos0
        depths.add(int(tok[3]))
        for b in range(6):
            f = tok[4 + b].split(b":")[1:]
            ist, fst = res.istat[0, b, :, k], res.fstat[0, b, :, k]
            n = int(ist[0])
            assert int(f[0]) == n
            if not n:
                continue
            for at, kind, idx in FLOAT_FIELDS:
                num, den = (ist[idx], n) if kind == "i" else (fst[idx], n) if kind == "f" else (fst[idx], int(ist[5]))
                if kind == "q2" and den == 0:
                    assert f[at] == b"0.00"
                    continue
                q = np.float32(num) / np.float32(den)
                assert f[at].decode() == py_f2(num, den), (tok[1], b, at, f[at], num, den)
                fields += 1
                ties += (Fraction(float(q)) * 100) % 1 == Fraction(1, 2)
                ulps += any("%.2f" % float(np.nextafter(q, np.float32(side))) != "%.2f" % float(q) for side in (-np.inf, np.inf))
    print("A1: %d float fields, %d exact ties, %d fields one ulp from another text; column depths %s" % (fields, ties, ulps, sorted(depths)))
    assert set(A1_DEPTHS) <= depths
    assert ties >= 200 and ulps >= 400, (ties, ulps)
    check(dev_lib, oracle_lib, "A1", [(arrs, region)], ref=ref)


A2_POSITIONS = [9, 10, 99, 100, 9_999, 10_000, 99_999, 100_000, 999_999, 1_000_000]


def case_a2_counts():
    """columns of 9, 10, 99, 100, 999 and 1000 reads; columns of 8, 98 and 998 reads and a deletion two (one) reads queued for them — the
    depth column is 10, 100, 1000 (9, 99, 999) there and crosses the digit count by the deletions alone; a bucket of one read"""
    ref = ref_of(4096)
    R = Reads(ref)
    T = 64
    for d in (9, 10, 99, 100, 999, 1000):
        for j in range(d):
            R.add(T, [(0, 4)], flag=(0, 16)[j & 1], edit=(lambda seq, qual, aq, ar, code: seq.__setitem__(aq[1], OTHER[code[ar[1]]])) if j == 0 else None)
        T += 64
    for d in (8, 98, 998):
        for extra in (1, 2):
            for j in range(d):
                R.add(T + 2, [(0, 2)], flag=(0, 16)[j & 1])
            for j in range(extra):
                R.add(T, [(0, 2), (2, 3), (0, 4)])                 # last base before the deletion at T + 1: due at T + 2
            T += 64
    return ref, R.arrays(), (1, T)


def test_a2_digit_counts_of_depth_and_read_counts(dev_lib, oracle_lib):
    ref, arrs, region = case_a2_counts()
    (want,), _ = check(dev_lib, oracle_lib, "A2-counts", [(arrs, region)], ref=ref)
    depth, counts, joined = set(), set(), set()
    for tok in lines_of(want):
        ns = [int(t.split(b":")[1]) for t in tok[4:10]]
        depth.add(int(tok[3])); counts.update(ns)
        dels = [int(t.split(b":")[1]) for t in tok[10:] if t.startswith(b"-")]
        if dels:
            joined.add((int(tok[3]) - sum(dels), int(tok[3])))
    assert {9, 10, 99, 100, 999, 1000} <= depth and {1, 9, 10, 99, 100, 999, 1000} <= counts
    print("A2: depth without and with the due deletions:", sorted(joined))
    assert any(len(str(a)) != len(str(b)) for a, b in joined), joined        # the deletions' read counts alone add a digit
    assert {10, 100, 1000} <= {b for a, b in joined if len(str(a)) != len(str(b))}, joined


def test_a2_digit_counts_of_positions_and_large_averages(dev_lib, oracle_lib):
    """1-based positions on both sides of 10, 100, 10^4, 10^5 and 10^6 (a reference of N with a short real stretch at each, regions of a
    few dozen positions); an average clipped length above 1000.00 and an NM average above 100.00 (the first is the length the soft clips
    LEAVE, the second NM over that length: 3000 aligned bases, and NM 400 over three; the 3' field is a fraction of the read's length and
    cannot reach 100); the literal 0.00 fields."""
    ref = np.full(1_004_000, ord("N"), np.uint8)
    real = ref_of(64)
    regions = []
    for p in A2_POSITIONS[1::2]:
        lo = max(p - 20, 0)
        ref[lo:lo + 40] = real[:40]
        regions.append((max(lo, 1) if lo else 0, lo + 40))
    R = Reads(ref, iupac=True)
    for j, p in enumerate(A2_POSITIONS[1::2]):
        lo = max(p - 20, 0)
        for s in range(3):
            R.add(lo + s, [(0, 36)], flag=(0, 16)[s & 1], nm=150 + 7 * s + j)
        R.add(lo + 2, [(4, 2000 + j), (0, 3000), (4, 500)], nm=3, edit=mismatches(range(3000)))      # the field is the average length LEFT by the clips: 3000.00 in its own bucket
        R.add(lo + 3, [(4, 3000), (0, 3)], nm=400, flag=16, edit=mismatches(range(3), THIRD))   # NM over 3 bases left: 133.33; a reverse read whose first base is not Q2: I_NQ2 == 0
        R.add(lo + 4, [(0, 10), (1, 2), (0, 10), (2, 2), (0, 6)], nm=4)
    arrs = R.arrays()
    steps = [(arrs, r) for r in regions]
    want, _ = check(dev_lib, oracle_lib, "A2-positions", steps, ref=ref, clear_queue=True)
    toks = lines_of(b"".join(want))
    assert set(A2_POSITIONS) <= {int(t[1]) for t in toks}
    clip = max(float(f.split(b":")[12]) for t in toks for f in t[4:10])
    nm = max(float(f.split(b":")[8]) for t in toks for f in t[4:10])
    assert clip >= 1000.0 and nm >= 100.0, (clip, nm)
    indel = [f.split(b":") for t in toks for f in t[10:]]
    assert indel and all(f[3] == b"0.00" for f in indel)                                     # an indel bucket's base-quality field
    assert any(f.split(b":")[10:12] == [b"0", b"0.00"] and f.split(b":")[1] != b"0" for t in toks for f in t[4:10])    # I_NQ2 == 0


# ------------------------------------------------------------------------------------------------ B. where a bucket's sums come from

B_TILES = 24                     # the tiles between the first and the (partial) last one
B_LAST = 37                      # lanes of the last tile
B_LANES = (0, 1, 62, 63)
BUCKETS = "=ACGTN"


def case_b(per_lib):
    """One-base reads, a pile per column.  The reference's character (A C G T N = in turn) names slot 0; the pile brings, in this order,
    two reads of the reference's base (where it is one of A C G T), two of a second base (slot 1), one each of the remaining bases (the
    third-allele table), an N and an '=' (the table, whatever the slots say: under a reference N or '=' a slot names the bucket and holds no
    read of it).  Which base comes second rotates.  Every lane of the first and of the partial last tile has a pile, and lanes 0, 1, 62, 63
    of the 24 tiles between them: each of the four lanes sees every (reference character, rotation).  Under -p the pile of a column belongs
    to library 0 or 2, the other one and library 1 own a lone read in some columns and none in the rest."""
    P = (B_TILES + 1) * 64 + B_LAST
    cols = {}
    for k in list(range(64)) + list(range((B_TILES + 1) * 64, P)):
        cols[k] = ((k % 64) % 6, ((k % 64) // 6) % 4)
    for t in range(1, B_TILES + 1):
        for li, lane in enumerate(B_LANES):
            cols[t * 64 + lane] = ((t + li) % 6, ((t - 1) // 6 + li) % 4)
    ref = np.full(P + 64, ord("A"), np.uint8)
    for k, (r, _) in cols.items():
        ref[k] = ord("ACGTN="[r])
    R = Reads(ref, iupac=True)

    def base(k, ch, lib):
        R.add(k, [(0, 1)], lib=lib, flag=(0, 16)[k & 1], edit=lambda seq, qual, aq, ar, code: seq.__setitem__(0, CODE[ch]))
    extra = []
    for k, (r, rot) in sorted(cols.items()):
        lib = (0, 2)[k & 1]
        others = [c for c in "ACGT" if c != "ACGTN="[r]]
        others = others[rot % len(others):] + others[:rot % len(others)]
        pile = (["ACGT"[r]] * 2 if r < 4 else []) + [others[0]] * 2 + others[1:] + ["N", "="]
        for ch in pile:
            base(k, ch, lib)
        if k % 3 == 0:
            extra.append((k, 2 - lib))
        if k % 7 == 0:
            extra.append((k, 1))
    for k, lib in extra:                                            # (behind the piles: a column's arrival order is the pile's)
        base(k, "ACGT"[k % 4], lib)
    arrs = R.arrays()
    kw = dict(per_lib=True, lib_names=["libA", "libB", "libC"]) if per_lib else dict()
    return ref, arrs, (0, P), kw


@pytest.mark.parametrize("per_lib", [False, True], ids=["merged", "per_library"])
def test_b_every_bucket_from_every_source_on_every_lane(dev_lib, sim_lib, oracle_lib, per_lib):
    ref, arrs, region, kw = case_b(per_lib)
    key = "B-%d" % per_lib
    (want,), (res,) = oracle(oracle_lib, key, [(arrs, region)], ref=ref, **kw)
    assert res.n_pos == (B_TILES + 1) * 64 + B_LAST
    if key + "w" not in _want:
        _want[key + "w"] = text_witness(sim_lib, [(arrs, region)], ref=ref, **kw)
    (w,) = _want[key + "w"]
    assert w["P"] == res.n_pos and w["last_tile_lanes"] == B_LAST and w["Lp"] == (3 if per_lib else 1)
    for what, sel in [("lane %d" % l, lambda v, l=l: [x[l] for x in v]) for l in B_LANES] + [("first tile", None), ("last tile", None)]:
        cells = w["cells"] if sel else w["first_tile" if what == "first tile" else "last_tile"]
        get = (lambda s: sel(cells[s])) if sel else (lambda s: cells[s])
        for b in range(1, 5):                                       # A C G T: a slot's own read counts, or the table
            for s in ("slot0", "slot1", "table"):
                assert get(s)[b] > 0, "%s: bucket %s never printed from %s" % (what, BUCKETS[b], s)
        for b in (0, 5):                                            # = N: the table, also when a slot names the bucket
            for s in ("table", "table_named"):
                assert get(s)[b] > 0, "%s: bucket %s never printed from %s" % (what, BUCKETS[b], s)
            assert get("slot0")[b] == 0 and get("slot1")[b] == 0
        assert not per_lib or sum(get("empty")) > 0              # (a lone read's block: five empty buckets)
    # the table's shape: records of many positions and several buckets in one (tile, library), so that the search skips others
    assert w["records_max"] >= (64 if per_lib else 128) and w["searched_max"] > w["records_max"], (w["records_max"], w["searched_max"])
    toks = lines_of(want)
    assert len(toks) == w["lines"]
    if per_lib:
        blocks = [sum(t == b"{" for t in tok) for tok in toks]
        assert {1, 2, 3} == set(blocks) and sum(blocks) == w["blocks"]      # a library without a read in the column has no block
    check(dev_lib, oracle_lib, key, [(arrs, region)], ref=ref, **kw)


# ------------------------------------------------------------------------------------------------ C. indel entries

C1_INS = ["A", "AC", "ACG", "ACGT", "ACGA", "ACGTA", "ANA", "A=A", "N", "=", "T", "TT", "TTG", "C", "=A", "NA", "G"]
C1_DELS = [1, 2, 3, 5, 9]


def ins_read(R, T, allele, **kw):
    def edit(seq, qual, aq, ar, code):
        seq[10:10 + len(allele)] = [CODE[c] for c in allele]
    R.add(T, [(0, 10), (1, len(allele)), (0, 10)], edit=edit, **kw)


def case_c1(n_libs):
    """position T + 9 carries 17 insertion alleles (proper prefixes of one another, alleles that differ first at their last base, inserted N
    and '=', equal alleles of different reads) and five deletion lengths; position T + 8 queues deletions for it"""
    ref = ref_of(1024)
    R = Reads(ref)
    T = 300
    order = [7, 3, 12, 0, 16, 9, 1, 5, 14, 2, 10, 6, 15, 4, 8, 13, 11]      # arrival order is not allele order
    for rep in range(3):
        for n, i in enumerate(order):
            if rep == 0 or (i + rep) % 3 == 0:
                ins_read(R, T, C1_INS[i], lib=(n + rep) % n_libs, flag=(0, 16)[(n + rep) & 1], mapq=20 + 3 * i + rep, nm=len(C1_INS[i]))
    for rep in range(2):
        for n, d in enumerate([5, 1, 9, 3, 2]):
            R.add(T, [(0, 10), (2, d), (0, 10)], lib=(n + rep) % n_libs, mapq=30 + d + rep, nm=d)
            R.add(T, [(0, 9), (2, d + 1), (0, 11)], lib=(n + 2 * rep) % n_libs, mapq=40 + d + rep, nm=d + 1)
    for l in range(n_libs):
        R.add(T, [(0, 40)], lib=l)
    kw = dict(per_lib=True, lib_names=["libA", "libB", "libC"][:n_libs]) if n_libs > 1 else dict()
    return ref, R.arrays(), (T, T + 40), kw


@pytest.mark.parametrize("n_libs", [1, 3])
def test_c1_allele_order_of_a_crowded_position(dev_lib, oracle_lib, n_libs):
    ref, arrs, region, kw = case_c1(n_libs)
    (want,), _ = check(dev_lib, oracle_lib, "C1-%d" % n_libs, [(arrs, region)], ref=ref, **kw)
    tok = [t for t in lines_of(want) if int(t[1]) == 310][0]
    if n_libs == 1:
        ins = [t.split(b":")[0].decode() for t in tok[10:] if t.startswith(b"+")]
        dels = [t.split(b":")[0] for t in tok[10:] if t.startswith(b"-")]
        assert ins == sorted("+" + a for a in C1_INS) and len(ins) >= 12            # std::map<std::string, ...> order: bytewise, a prefix first
        assert [len(d) - 1 for d in dels] == sorted(d + 1 for d in C1_DELS)          # queued by the position before: due here
        nxt = [t for t in lines_of(want) if int(t[1]) == 311][0]
        assert [len(t.split(b":")[0]) - 1 for t in nxt[10:] if t.startswith(b"-")] == sorted(C1_DELS)


def case_c2():
    """deletions over lower-case, IUPAC and N reference characters and past the end of the reference; an insertion that runs to the read's
    last base"""
    ref = ref_of(400)
    ref[100:120] = np.frombuffer(b"acgtnNRYKMSWBDHVryxA", np.uint8)
    R = Reads(ref, iupac=True)
    for s in (80, 85, 90):
        R.add(s, [(0, 60)])
    for n, d in enumerate((1, 4, 8, 20)):
        R.add(70 + n, [(0, 30 - n), (2, d), (0, 20)], nm=d)        # last base at 99: the allele spells ref[100 .. 100 + d)
        R.add(75, [(0, 30 + n), (2, d), (0, 12)], nm=d)            # ... and from inside the stretch
    R.add(370, [(0, 25), (2, 30), (0, 10)], nm=30)                  # deleted bases 395 .. 424: the reference ends at 400
    R.add(360, [(0, 38), (2, 8), (0, 4)], nm=8)
    R.add(350, [(0, 48)])
    R.add(200, [(0, 20), (1, 6)], edit=lambda seq, qual, aq, ar, code: seq.__setitem__(slice(20, 26), [1, 15, 0, 2, 4, 8]))
    R.add(200, [(0, 20), (1, 3), (0, 5)], edit=lambda seq, qual, aq, ar, code: seq.__setitem__(slice(20, 23), [1, 15, 0]))
    R.add(190, [(0, 40)])
    return ref, R.arrays(), [(60, 140), (190, 260), (340, 440)]


@pytest.mark.parametrize("with_ref", [True, False], ids=["reference", "no_reference"])
def test_c2_allele_spelling(dev_lib, oracle_lib, with_ref):
    ref, arrs, regions = case_c2()
    want, _ = check(dev_lib, oracle_lib, "C2-%d" % with_ref, [(arrs, r) for r in regions], ref=ref if with_ref else None, clear_queue=True)
    text = b"".join(want)
    if with_ref:
        assert b"\t-acgtnNRYKMSWBDHVryxA:" in text and b"\t-a:" in text
        assert re.search(rb"\t-[ACGT]{5}N{25}:", text)                              # 'N' where the reference has no character
        assert b"\t+AN=CGT:" in text and b"\t+AN=:" in text


C3_KS = sorted({m + d for m in (4, 16, 64, 128) for d in (-1, 0, 1)} | {1, 2})
C3_POS0 = 999


def case_c3():
    """two libraries under -p; for every k of C3_KS a deletion queued at plane index k - 1 and due at k (k = 1: queued by the lead position,
    which is never printed), alternating between the libraries; a second region whose plane index 0 is a printed line with no predecessor
    and queues a deletion itself"""
    ref = ref_of(2048)
    R = Reads(ref)
    for l in (0, 1):
        R.add(C3_POS0, [(0, 200)], lib=l)
    for n, k in enumerate(C3_KS):
        last = C3_POS0 + k - 1
        m = min(last - C3_POS0 + 1, 20)
        R.add(last - m + 1, [(0, m), (2, 1 + n % 3), (0, 12)], lib=n & 1, nm=1 + n % 3, mapq=30 + n)
        if k % 16 == 0:
            R.add(last - m + 1, [(0, m), (2, 2), (0, 12)], lib=1 - (n & 1), nm=2, mapq=50)
    for l in (0, 1):
        R.add(1500, [(0, 1), (2, 2 + l), (0, 30)], lib=l)           # the second region's index 0
        R.add(1500, [(0, 40)], lib=l)
    return ref, R.arrays(), [(C3_POS0 + 1, C3_POS0 + 200), (1400, 1540)], dict(per_lib=True, lib_names=["libA", "libB"])


@pytest.mark.parametrize("shift", [2, 4, 6])
def test_c3_deletions_due_across_bucket_and_tile_edges(knob_lib, sim_lib, oracle_lib, monkeypatch, shift):
    ref, arrs, regions, kw = case_c3()
    monkeypatch.setenv("BRC_IBUCKET_SHIFT", str(shift))
    steps = [(arrs, r) for r in regions]
    ws = text_witness(sim_lib, steps, ref=ref, **kw)
    assert [w["ibucket_shift"] for w in ws] == [shift, shift] and [w["pos0"] for w in ws] == [C3_POS0, 1500]
    want, res = check(knob_lib, oracle_lib, "C3", steps, ref=ref, **kw)
    assert res[0].pos0 == C3_POS0 == res[0].beg0 - 1 and res[1].pos0 == 1500 > res[1].beg0
    toks = {int(t[1]) - 1: t for t in lines_of(want[0])}
    assert C3_POS0 not in toks                                      # the lead position is never printed
    for k in C3_KS:
        assert any(t.startswith(b"-") for t in toks[C3_POS0 + k]), k
    second = lines_of(want[1])
    assert int(second[0][1]) == 1501 and not any(t.startswith(b"-") for t in second[0]) and sum(t.startswith(b"-") for t in second[1]) == 2


def case_c4():
    """-p with three libraries.  At X the deletion of libA's read is due and libA has no read in the column (the read ends with the deletion:
    libA's next column is 40 positions on, where the entry is dropped); at Y a read without a library abandons the due position, at Z the
    position that would have queued."""
    ref = ref_of(2048)
    R = Reads(ref)
    X, Y, Z = 300, 600, 900
    R.add(X - 40, [(0, 200)], lib=1)
    R.add(X - 20, [(0, 20), (2, 3)], lib=0, nm=3)                   # last base at X - 1, nothing behind the deletion
    R.add(X + 40, [(0, 30)], lib=0)
    for P0, cover in ((Y, Y), (Z, Z - 1)):
        for l in (0, 1, 2):
            R.add(P0 - 40, [(0, 100)], lib=l)
            R.add(P0 - 20, [(0, 20), (2, 2 + l), (0, 20)], lib=l, nm=2 + l)
        R.add(cover, [(0, 1)], lib=-1)
    return ref, R.arrays(), [(200, 1000)], dict(per_lib=True, lib_names=["libA", "libB", "libC"])


def test_c4_who_prints_a_due_deletion(dev_lib, oracle_lib):
    ref, arrs, regions, kw = case_c4()
    (want,), _ = check(dev_lib, oracle_lib, "C4", [(arrs, regions[0])], ref=ref, **kw)
    toks = {int(t[1]) - 1: t for t in lines_of(want)}
    # (a read that ends with its deletion is still a read of the deleted columns: libA has a block of six empty buckets at X and its entry)
    assert toks[300][3] == b"2" and b"libA" in toks[300] and sum(t.startswith(b"-") for t in toks[300]) == 1
    assert b"libA" in toks[302] and b"libA" not in toks[303] and not any(t.startswith(b"-") for t in toks[340])
    assert 600 not in toks and 899 not in toks                                                                         # abandoned positions print nothing
    assert not any(t.startswith(b"-") for t in toks[601]) and not any(t.startswith(b"-") for t in toks[900])


def test_c4_a_due_deletion_of_a_library_without_a_read_in_the_column(dev_lib, oracle_lib):
    """Inside one region a library that queued a deletion at k - 1 always has a read in column k (the read that carries the deletion spans
    the deleted bases), so the case needs two regions: libA's deletion is left pending, due at X; the next region's reads of libA start 40
    positions behind X.  The entry is not printed at X, not added to the depth, and dropped at libA's next column."""
    ref = ref_of(1024)
    X = 300
    A = Reads(ref); B = Reads(ref)
    A.add(X - 20, [(0, 20), (2, 3), (0, 10)], lib=0, nm=3); A.add(X - 30, [(0, 30)], lib=1)
    B.add(X - 10, [(0, 100)], lib=1); B.add(X + 40, [(0, 30)], lib=0); B.add(X + 20, [(0, 20), (2, 2), (0, 20)], lib=1, nm=2)
    steps = [dict(arrs=A.arrays(), region=(X - 10, X), fetch=False), dict(arrs=B.arrays(), region=(X - 5, X + 60), fetch=False)]
    want, _ = check(dev_lib, oracle_lib, "C4-absent", steps, ref=ref, per_lib=True, lib_names=["libA", "libB", "libC"])
    toks = {int(t[1]) - 1: t for t in lines_of(want[1])}
    assert toks[X][3] == b"1" and b"libA" not in toks[X] and not any(t.startswith(b"-") for t in toks[X])
    assert b"libA" in toks[X + 40] and toks[X + 40][3] == b"3" and sum(t.startswith(b"-") for t in toks[X + 40]) == 1      # (libB's own, due there)


def test_c4_insertion_centric_with_empty_base_buckets(dev_lib, oracle_lib):
    """-i with a base-quality threshold that only the base in front of every insertion passes — which -i does not count: the six buckets of
    the column are empty, the insertion entries remain"""
    ref = ref_of(1024)
    R = Reads(ref)
    T = 300

    def anchor(seq, qual, aq, ar, code):
        qual[:] = 20; qual[9] = 60
    for n, a in enumerate(C1_INS[:13]):
        R.add(T, [(0, 10), (1, len(a)), (0, 10)], flag=(0, 16)[n & 1], edit=lambda seq, qual, aq, ar, code, a=a: (seq.__setitem__(slice(10, 10 + len(a)), [CODE[c] for c in a]), anchor(seq, qual, aq, ar, code)))
    R.add(T, [(0, 40)], edit=lambda seq, qual, aq, ar, code: qual.__setitem__(slice(None), 20))
    (want,), _ = check(dev_lib, oracle_lib, "C4-i", [(R.arrays(), (T, T + 40))], ref=ref, insertion_centric=True, min_bq=50)
    tok = [t for t in lines_of(want) if int(t[1]) == T + 10][0]
    assert all(t.split(b":")[1] == b"0" for t in tok[4:10]) and sum(t[:1] == b"+" for t in tok[10:]) == 13


# ------------------------------------------------------------------------------------------------ D. geometry

D1_P = [1, 2, 255, 256, 257, 4095, 4096, 4097, 8191, 8193]


def case_d1(P):
    """a region of exactly P planes: under -p a one-base read without a library at index 0 and one at P - 1 stretch the region (their positions are abandoned: no line); the lines are
    short reads placed so that index 0 and P - 1 are empty, printed and empty positions alternate, and a lone line follows 300 empty ones"""
    ref = ref_of(P + 64)
    R = Reads(ref)
    if P > 2:
        R.add(0, [(0, 1)], lib=-1); R.add(P - 1, [(0, 1)], lib=-1)
    at = [k for k in range(1, min(P - 1, 40), 2)] + [k for k in (341, 342, 700, P - 258, P - 257, P - 256, P - 3, P - 2) if 40 < k < P - 1]
    if P <= 2:
        at = list(range(P))
    for n, k in enumerate(sorted(set(at))):
        R.add(k, [(0, 1)], flag=(0, 16)[n & 1])
        if n % 5 == 0:
            R.add(k, [(0, 1)], edit=lambda seq, qual, aq, ar, code: seq.__setitem__(0, OTHER[code[ar[0]]]))
    if P > 4000:
        for s in range(1000, 1600, 3):
            R.add(s, [(0, 2), (2, 2), (0, 3)] if s % 9 == 0 else [(0, 5)])
    return ref, R.arrays(), (0, P)


D1_KW = dict(per_lib=True, lib_names=["libA"])


@pytest.mark.parametrize("P", D1_P)
def test_d1_plane_counts_around_every_launch_boundary(dev_lib, oracle_lib, P):
    """k_text_len writes P + 1 entries, the scan works in chunks of SCAN_CHUNK: the grid's last block, the scan's vector path against its
    tail path and the second-level aggregate change over at these P"""
    ref, arrs, region = case_d1(P)
    (want,), (res,) = check(dev_lib, oracle_lib, "D1-%d" % P, [(arrs, region)], ref=ref, **D1_KW)
    assert res.n_pos == P and res.pos0 == 0
    printed = {int(t[1]) - 1 for t in lines_of(want)}
    assert printed and (P <= 2 or (0 not in printed and P - 1 not in printed))
    if P > 700:
        assert 700 in printed and not any(400 <= k < 700 for k in printed)          # a lone line after 300 empty positions
    assert (P + 1 + SCAN_CHUNK - 1) // SCAN_CHUNK == {1: 1, 2: 1, 255: 1, 256: 1, 257: 1, 4095: 1, 4096: 2, 4097: 2, 8191: 2, 8193: 3}[P]


def test_d1_a_region_whose_every_read_is_filtered(dev_lib, oracle_lib):
    """-q above every read's map quality: the columns are still columns (every line is printed, with depth 0 and six empty buckets).  Reads
    without a library under -p (every position abandoned) leave a region of 257 planes without a byte: total 0, no parts."""
    ref, arrs, region = case_d1(257)
    (want,), (res,) = check(dev_lib, oracle_lib, "D1-filtered", [(arrs, region)], ref=ref, min_mapq=61, **D1_KW)
    assert res.n_pos == 257 and want and all(t[3] == b"0" for t in lines_of(want))
    arrs = dict(arrs, lib=np.full_like(arrs["lib"], -1))
    (want,), (res,) = check(dev_lib, oracle_lib, "D1-no_column", [(arrs, region)], ref=ref, **D1_KW)
    assert res.n_pos == 257 and want == b""


def test_d1_a_shorter_region_after_a_longer_one(dev_lib, oracle_lib):
    """two regions back to back on one engine, the second shorter: the stale tail of the offsets and of the text, and the two download
    slots, must not show — then the long one again"""
    long_, short = case_d1(4097), case_d1(257)
    assert long_[0][:300].tobytes() == short[0][:300].tobytes()    # (ref_of: one reference, two lengths)
    steps = [(long_[1], long_[2]), (short[1], short[2]), (short[1], (1, 2)), (long_[1], long_[2])]
    want, res = check(dev_lib, oracle_lib, "D1-back_to_back", steps, ref=long_[0], clear_queue=True, **D1_KW)
    assert [r.n_pos for r in res] == [4097, 257, 2, 4097] and want[0] == want[3] and want[1] and want[2] and want[1] != want[0]


D2_PLACES = ["P-1", "P-256", "P-257", "P-512", "0"]


def case_d2(P, place, twin, pending_c=False):
    """-p, three libraries, regions on one engine that starts with clean queues.  A region of P planes from 1000 on: libB's reads run to
    its end; libA's last processed column j carries a deletion — behind it a read without a library abandons the columns libA's read goes
    on to (k_last_processed must not count them) —; the twin's read of libA is longer than the abandoned stretch: libA is processed once
    more, without a deletion, and its queue is empty.  The next region starts at libA's due position X = 1000 + j + 1 with plain reads of
    all three libraries.  The queues being clean, the region of P planes is formatted without the line patcher: what it leaves in libA's
    queue is decided by the last_processed the backend reports and by nothing else (format_device_text), and the next region prints it.
    pending_c: a first region of libC alone leaves its deletion pending, due at X + 1 — the region of P planes then starts from busy
    queues and goes through the patcher, which keeps the queues itself."""
    j = {"P-1": P - 1, "P-256": P - 256, "P-257": P - 257, "P-512": P - 512, "0": 0}[place]
    X = 1000 + j + 1
    ref = ref_of(3000)
    R0 = Reads(ref); R1 = Reads(ref); R2 = Reads(ref)
    R0.add(X - 9, [(0, 10), (2, 4), (0, 10)], lib=2, nm=4)          # libC: last base at X, due at X + 1; the region ends there
    for s in range(1000, 1000 + P, 50):
        R1.add(s, [(0, min(50, 1000 + P - s))], lib=1)
    m = min(j + 1, 20)
    tail = 60 if twin else 20
    R1.add(1000 + j - m + 1, [(0, m), (2, 3), (0, tail)], lib=0, nm=3)
    if place != "P-1":
        R1.add(X, [(0, 40)], lib=-1)
    for l in (0, 1, 2):
        R2.add(X + (1 if l == 2 else 0), [(0, 30)], lib=l)
    steps = [dict(arrs=R1.arrays(), region=(1000, 1000 + P), fetch=False), dict(arrs=R2.arrays(), region=(X, X + 20), fetch=False)]
    if pending_c:
        steps.insert(0, dict(arrs=R0.arrays(), region=(X - 8, X + 1), fetch=False))
    return ref, steps, j, X, dict(per_lib=True, lib_names=["libA", "libB", "libC"])


def d2_check(dev_lib, sim_lib, oracle_lib, P, place, twin, pending_c):
    ref, steps, j, X, kw = case_d2(P, place, twin, pending_c)
    key = "D2-%d-%s-%d-%d" % (P, place, twin, pending_c)
    want, res = check(dev_lib, oracle_lib, key, steps, ref=ref, **kw)
    assert res[-2].n_pos == P and res[-2].pos0 == 1000
    if key + "w" not in _want:
        _want[key + "w"] = text_witness(sim_lib, steps, ref=ref, **kw)
    w = _want[key + "w"][-2]                                        # (the batch as built: the simulator's serial loop, not the kernel)
    assert w["last_processed"] == [j + 41 + 22 if twin else j, P - 1, -1], (w["last_processed"], j)
    first, second = lines_of(want[-1])[:2]
    assert int(first[1]) == X + 1 and int(second[1]) == X + 2
    a_block = first[first.index(b"libA"):first.index(b"libB")]
    assert any(t.startswith(b"-") for t in a_block) != twin        # libA's deletion is printed / its queue was emptied
    c_block = second[second.index(b"libC"):]
    assert sum(t.startswith(b"-") for t in c_block) == pending_c    # libC, never processed in between, kept its entry


@pytest.mark.parametrize("P", [768, 700])
@pytest.mark.parametrize("place", D2_PLACES)
def test_d2_last_processed_column_of_every_library(dev_lib, sim_lib, oracle_lib, P, place):
    """k_last_processed (a back-to-front loop in chunks of 256), observed through what the next region prints: from clean queues, so that
    the region of P planes takes format_device_text's direct path — the only reader of the kernel's answer.  A last_processed that is
    wrong for libA (a column of the abandoned stretch, a column of another chunk, none) leaves libA's queue empty where the oracle prints
    its deletion; the twin catches an answer that stops at the deletion's column."""
    for twin in (False, True):
        if not (twin and place == "P-1"):
            d2_check(dev_lib, sim_lib, oracle_lib, P, place, twin, False)


@pytest.mark.parametrize("P,place", [(768, "P-256"), (700, "P-257")])
def test_d2_a_library_never_processed_keeps_its_queue(dev_lib, sim_lib, oracle_lib, P, place):
    """libC's deletion, left pending by a region before, survives a region of P planes in which libC is never processed and is printed by
    the region behind it; libA's and libB's queues as above, here kept by the line patcher (the queues are busy from the start)"""
    for twin in (False, True):
        d2_check(dev_lib, sim_lib, oracle_lib, P, place, twin, True)


def test_d3_hand_back_one_byte_below_the_total(knob_lib, sim_lib, oracle_lib, monkeypatch):
    """BRC_DEVICE_TEXT_LIMIT one byte below a region's total and exactly at it: formatted on the host below, on the device at it, the same
    text both times.  The route is read off the result of the library under test: planes below the limit, none at it (the simulator's
    witness, which leaves no record of a handed-back region, agrees)"""
    ref, arrs, region, kw = case_c1(3)
    assert arrs["pos"].min() == region[0]      # (no lead position: every line the device writes is printed, the total is the text's length)
    (want,), _ = oracle(oracle_lib, "D3", [(arrs, region)], ref=ref, **kw)
    (w,) = text_witness(sim_lib, [(arrs, region)], ref=ref, **kw)
    total = w["total"]
    assert total == len(want) > 3000
    for limit, records in ((total - 1, 0), (total, 1)):
        monkeypatch.setenv("BRC_DEVICE_TEXT_LIMIT", str(limit))
        assert len(text_witness(sim_lib, [(arrs, region)], ref=ref, **kw)) == records
        # the product's own route: the planes came with the result below the limit (the host formatted it) and did not at it
        check(knob_lib, oracle_lib, "D3", [(arrs, region)], routes=ROUTES[:1], on_device=limit == total, ref=ref, **kw)


# ------------------------------------------------------------------------------------------------ E. the host side across regions

def test_e1_a_region_cut_into_pieces(dev_lib, oracle_lib):
    """BRC_OPT_CONTINUES_PREVIOUS for every piece but the first, as the command line runs: cut at every boundary of C3 (the due position
    the first of its piece, the queueing position the lead), at cuts whose lead position is empty and inside an empty stretch"""
    ref, arrs, regions, kw = case_c3()
    beg0, end = regions[0][0], 1540
    whole, res = oracle(oracle_lib, "E1", [(arrs, (beg0, end)), (arrs, (beg0, end))], ref=ref, **kw)
    third_events_ok("E1", res, [(arrs, (beg0, end))] * 2, ref=ref, **kw)
    assert whole[0] == whole[1]                                     # (the region leaves nothing pending)
    assert whole[0].count(b"\n") > 200
    for shiftby in (0, 1):
        cuts = sorted({C3_POS0 + k + shiftby for k in C3_KS if k + shiftby > 1} | {1300, 1350, 1499, 1500, 1501})      # (1200 .. 1499 hold no read)
        edges = [beg0] + cuts + [end]
        steps = [dict(arrs=arrs, region=(a, b), continues=n > 0) for n, (a, b) in enumerate(zip(edges[:-1], edges[1:]))]
        steps.append(dict(arrs=arrs, region=(beg0, end)))          # and the region once more, in one piece and continuing nothing: every
        for route in ROUTES:                                        # piece must have left the queues the whole region leaves (here: empty ones)
            got, got_res = run_steps(dev_lib, steps, ref=ref, **route, **kw)
            assert_routes("E1", route, got_res)
            assert b"".join(got[:-1]) == whole[0], (shiftby, route)
            assert got[-1] == whole[0], (shiftby, route, "the pieces left something in the queues")


E2 = queue_scenarios()


@pytest.mark.parametrize("name", list(E2))
def test_e2_queues_that_did_not_start_clean(dev_lib, oracle_lib, name):
    ref, steps, kw = E2[name]
    want, _ = check(dev_lib, oracle_lib, "E2-" + name, steps, ref=ref, **kw)
    queue_expectations(name, want)


def case_e3_long():
    """40 deletion alleles of 5 .. 200 bases left pending by a region that ends at their due position; the next region's reads are plain:
    the device's line at the due position holds no indel entry, the rewritten one about 6 KB of them — more than the 4096 bytes of slack the
    patcher asks for at a time.  Three times over, 100 positions apart, each behind a region that ends there; the last time 400 alleles of
    1 .. 400 bases: one line of about 100 KB, more than the 64 KiB the patch buffer starts with, so the buffer itself is regrown while the
    line is written (tests/sim/host_check.cpp runs the same line under the host sanitizers, whose realloc always moves)"""
    ref = ref_of(2048)
    steps = []
    plain = Reads(ref)
    for s in range(300, 1100, 40):
        plain.add(s, [(0, 80)])
    plain = plain.arrays()
    for D in (500, 600, 700):
        R = Reads(ref)
        for d in (range(5, 205, 5) if D < 700 else range(1, 401)):
            R.add(D - 20, [(0, 20), (2, d), (0, 10)], nm=d, mapq=20 + d % 40)
        steps += [(R.arrays(), (D - 10, D)), (plain, (D - 5, D + 5))]
    return ref, steps


def test_e3_a_patched_line_outgrows_its_buffer(dev_lib, oracle_lib):
    ref, steps = case_e3_long()
    want, _ = check(dev_lib, oracle_lib, "E3-long", steps, ref=ref)
    for D, text in zip((500, 600, 700), want[1::2]):
        line = [l for l in text.split(b"\n") if l.startswith(b"chrS\t%d\t" % (D + 1))][0]
        short = [l for l in text.split(b"\n") if l.startswith(b"chrS\t%d\t" % (D + 2))][0]
        assert line.count(b"\t-") == (40 if D < 700 else 400) and len(line) > len(short) + (4096 + 1024 if D < 700 else 65536 + 16384)


E3_MANY = 24


def test_e3_patched_lines_regrow_the_buffer_mid_line(dev_lib, oracle_lib):
    """the same 40 alleles pending in each of 24 libraries (a library's queue is touched only where the library is processed), due at 24
    successive positions of one last region: its rewritten lines add up to about 150 KB, so the patch buffer — which grows by 64 KiB and
    more at a time — is regrown in the middle of a line, with lines already in it"""
    ref = ref_of(2048)
    names = ["L%02d" % l for l in range(E3_MANY)]
    steps = []
    last = Reads(ref)
    for l in range(E3_MANY):
        D = 500 + l
        R = Reads(ref)
        for d in range(5, 205, 5):
            R.add(D - 20, [(0, 20), (2, d), (0, 10)], nm=d, lib=l, mapq=20 + d % 40)
        steps.append(dict(arrs=R.arrays(), region=(D - 10, D), fetch=False))
        last.add(480, [(0, 80)], lib=l)
    steps.append(dict(arrs=last.arrays(), region=(490, 540), fetch=False))
    want, _ = check(dev_lib, oracle_lib, "E3-many", steps, ref=ref, per_lib=True, lib_names=names)
    lines = want[-1].split(b"\n")
    assert sum(l.count(b"\t-") == 40 for l in lines) == E3_MANY and len(want[-1]) > 2 * 65536


def test_e3_depth_changes_its_digit_count_in_the_patch(dev_lib, oracle_lib):
    """the device's line counts its own due deletions into the depth; the queue's truth differs: 9 <-> 10 and 99 <-> 100 both ways"""
    ref = ref_of(4096)
    steps = []
    for n, base in enumerate((9, 99)):
        for grows in (True, False):
            D = 500 + 800 * n + 300 * grows
            A = Reads(ref); B = Reads(ref)
            if grows:                                               # pending entry due at D joins: base -> base + 1
                A.add(D - 20, [(0, 20), (2, 2), (0, 10)], nm=2)
                first = (D - 10, D)
            else:                                                   # a pending entry due far behind blocks the region's own deletion: base + 1 -> base
                A.add(D + 100, [(0, 20), (2, 2), (0, 10)], nm=2)
                first = (D + 110, D + 120)
                B.add(D - 20, [(0, 20), (2, 2)], nm=2)
            for j in range(base):
                B.add(D - 5, [(0, 30)], flag=(0, 16)[j & 1])
            steps += [dict(arrs=A.arrays(), region=first, fetch=False), dict(arrs=B.arrays(), region=(D - 3, D + 3), fetch=False)]
    want, _ = check(dev_lib, oracle_lib, "E3-depth", steps, ref=ref, clear_queue=False)
    depth = []
    for n, base in enumerate((9, 99)):
        for grows in (True, False):
            D = 500 + 800 * n + 300 * grows
            text = want[2 * (2 * n + (0 if grows else 1)) + 1]
            depth.append([int(t[3]) for t in lines_of(text) if int(t[1]) == D + 1][0])
    assert depth == [10, 9, 100, 99], depth


E3_NAMES = ["+A", "-", "z" * 300, "{", "}"]


def test_e3_library_names_that_look_like_syntax(dev_lib, oracle_lib):
    """-p with libraries named like the tokens the patcher parses (bytewise sorted, as brc_create demands) and a 300-byte name, through a
    region whose queues are busy: every line is parsed and rewritten"""
    assert E3_NAMES == sorted(E3_NAMES, key=lambda s: s.encode())
    ref = ref_of(1024)
    R = Reads(ref)
    for l in range(5):
        for s in range(200, 500, 30):
            R.add(s, [(0, 60)], lib=l)
        R.add(280, [(0, 20), (2, 2 + l), (0, 20)], lib=l, nm=2 + l)      # last base 299: due at 300
        R.add(330, [(0, 20), (2, 1 + l), (0, 20)], lib=l, nm=1 + l)      # 349 / 350
        ins_read(R, 355, "ACG"[:1 + l % 3], lib=l)
    arrs = R.arrays()
    steps = [(arrs, (250, 300)), (arrs, (260, 420)), (arrs, (295, 305))]
    want, _ = check(dev_lib, oracle_lib, "E3-names", steps, ref=ref, per_lib=True, lib_names=E3_NAMES)
    line = [l for l in want[1].split(b"\n") if l.startswith(b"chrS\t301\t")][0]
    assert line.count(b"\t-") == 10 + 1 and b"\t}\t{\t" in line and b"\t{\t{\t" in line and b"\t-\t{\t" in line
