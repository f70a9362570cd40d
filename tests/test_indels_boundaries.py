"""brc_indels_gather over hand-made views (tests/handmade_views.py): the two device scans with their carry round (I1: windows up to
131 073 positions; I2: up to 65 537 records, the record count on 255 / 256 / 257, equal to the slot count, and a multiple of 256 below
it), the order inside one position with equal records in it (I3), every rule that spells an allele (I4) and the window's edges (I5).
The reference is indel_table_reference — the contract of include/brc.h in plain Python — compared as bytes: integers, float bit
patterns, the thirteen metric columns, offsets and text.

Every body runs on [sim] (tests/sim_indels, CPU suite) and on [hip] (the product's library, gpu-marked).  The two scans are device
code of their own (k_scan_reduce, k_scan_parts, k_scan_apply; the CPU build has a serial loop): for them the [hip] ids of I1 and I2
are the test.  DESIGN.md 5, "Hand-made views at the edges of the dense, panel and indel libraries", has the census and the mutants."""
import numpy as np
import pytest

from bam_readcount_amd import capi
import handmade_views as hv
from route import Route
import test_indels as ti

DESTS = ti.DESTS
TILE = 256


@pytest.fixture(scope="module", params=["sim", pytest.param("hip", marks=pytest.mark.gpu)])
def route(request):
    return Route(request.param, ("indels",))


_cache = {}


def cached(key, make):
    """a case and its reference, computed once and shared by the routes"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def reference(key, I, k0, n):
    return cached(("want", key, k0, n), lambda: hv.indel_table_reference(I, I["pos0"] + k0, n))


def check(route, v, key, I, k0, n, what, short=False, slack=0):
    """the two-call protocol on one window: the counts alone, then every destination with exact (+ slack) capacities — the two count
    words and allele_off[M] among what is compared; short: once more with both capacities one short"""
    want, order = reference(key, I, k0, n)
    m, nb = want["pos"].shape[1], int(want["alleles"].size)
    rc, counts, _ = ti.gather(route, v, k0, n, 0, 0, dests=())
    assert rc == 0, (what, route.indels.lib.brc_indels_last_error(route.indels.h))
    assert counts.tolist() == [m, nb], (what, counts.tolist(), [m, nb])
    rc, counts, got = ti.gather(route, v, k0, n, m + slack, nb + slack)
    assert rc == 0 and counts.tolist() == [m, nb], what
    ti.assert_table(got, want, m + slack, nb + slack, what)
    assert int(got["allele_off"][m]) == nb
    if short and m:
        for cap, acap in ((m - 1, nb), (m, nb - 1)):
            rc, counts, got = ti.gather(route, v, k0, n, cap, acap)
            assert rc == 0 and counts.tolist() == [m, nb], (what, cap, acap)
            ti.assert_table(got, want, cap, acap, "%s, capacities %d %d" % (what, cap, acap))
    return want, order, got


# the reads every view of this file spells its insertions from (seq_off[0] == 1: odd)
ALL16 = list(range(16))
TEXT = "ACGTN=ATANA=ACT"
READS = [ALL16 + [1, 2, 4, 8],                         # 0: every code from q = 0 (even)
         [1] + ALL16 + [2],                            # 1: every code from q = 1 (odd); seq_off 11
         [],                                           # 2: l_qseq == 0
         [hv.CODE[c] for c in TEXT],                   # 3: the texts of I3
         [hv.CODE[c] for c in "ACGT"],                 # 4: "AC" once more, from another read
         [(1, 2, 4, 8, 15, 0)[(7 * j + j // 6) % 6] for j in range(310)]]  # 5: a long one
# (rep_read, rep_qpos, len) of I3's insertion texts in read 3
SPELL = {"+A": (3, -1, 1), "+AC": (3, -1, 2), "+ACG": (3, -1, 3), "+ACT": (3, 11, 3), "+AN": (3, 7, 2), "+AT": (3, 5, 2), "+A=": (3, 9, 2), "+=": (3, 4, 1)}


# ------------------------------------------------------------------------------------------------ I1 the first scan (positions)

I1_N = (1, 255, 256, 257, 512, 513, 65535, 65536, 65537, 131072, 131073)


def i1_case(n):
    """a view of n + 1 positions, 40 live records: on the first and the last position of the window [0, n) and of [1, n + 1), and on both
    sides of every 256-position edge near the start, near position 65 536 and near the end"""
    P = n + 1
    edges = [0, 1, n - 1, n] + [e + d for e in (256, 512, 768, 65280, 65536, 65792, 131072, (n // TILE) * TILE, (n // TILE - 1) * TILE) for d in (-1, 0, 1)]
    at = sorted({p for p in edges if 0 <= p < P})
    at += [p for p in range(2, min(P, 40), 3) if p not in at][:max(10 - len(at), 0)]      # (a small window: further positions, up to ten)
    slots = []
    for r in range(4):                                                    # four records a position at the most
        for p in at:
            if len(slots) < 40:
                slots.append(hv.slot(100 + p, r % 3, r + 1 if r % 2 == 0 else -(r + 1), 3, -1, tag=len(slots)))
    slots = [slots[i] for i in np.random.default_rng(n).permutation(len(slots))]
    return hv.indel_arrays(slots, READS, pos0=100, n_pos=P, n_lib=3)


@pytest.mark.parametrize("n", I1_N)
def test_i1_the_position_scan_and_its_carry(route, n):
    I = cached(("i1", n), lambda: i1_case(n))
    assert len(I["slots"]) == (40 if n >= 255 else 8) and I["run"] <= 4 and (I["slots"][:, 2] != 0).all()
    v, keep = hv.make_indels(route, I)
    for k0 in (0, 1):
        want, order, got = check(route, v, ("i1", n), I, k0, n, "I1 n %d k0 %d" % (n, k0))
        pos = want["pos"][0].astype(np.int64) - I["pos0"] - k0
        if n > 65536 + 257:                                               # records behind partial 256, 257 and 512: their index is the carry's
            assert (pos // TILE == 256).any() and (pos // TILE == 257).any() and (pos // TILE >= 511).any() and (pos < TILE).any()


# ------------------------------------------------------------------------------------------------ I2 the second scan and k_emit (records)

def i2_full(S):
    """S live records of S slots: four at most per position, lengths 1 .. 3 and both signs, in shuffled slot order"""
    rng = np.random.default_rng(S)
    slots = [hv.slot(50 + s // 4, s % 2, (1 + s % 3) * (-1 if s % 4 == 3 else 1), 5, int(s % 300), tag=s % 60000) for s in range(S)]
    slots = [slots[i] for i in rng.permutation(S)]
    return hv.indel_arrays(slots, READS, ref=b"ACGTTGCA" * 8, ref_lo=40, pos0=50, n_pos=(S + 3) // 4 + 2, n_lib=2)


def i2_some(M, S=1000):
    """M live records inside the window [500, 1100) of a view of 2000 positions, among S slots: the others dead (len == 0, with a
    body) or outside the window, interleaved"""
    slots = []
    for s in range(S):
        if s < M:
            slots.append(hv.slot(500 + (s * 7) % 600, s % 2, 1 + s % 3 if s % 2 else -(1 + s % 5), 5, s % 200, tag=s))
        elif s % 2:
            slots.append(hv.slot(500 + s % 600, 1, 0, 5, 3, tag=s))                                  # dead, inside the window
        else:
            slots.append(hv.slot((s % 500) if s % 4 else 1100 + s % 900, 0, 2, 5, 3, tag=s))         # live, outside it
    slots = [slots[i] for i in np.random.default_rng(M).permutation(S)]
    return hv.indel_arrays(slots, READS, ref=b"ACGTTGCA" * 8, ref_lo=480, pos0=0, n_pos=2000, n_lib=2)


@pytest.mark.parametrize("S", [1, 255, 256, 257, 512, 65536, 65537])
def test_i2_every_slot_live(route, S):
    """M == n_slots: k_emit's closing lane M is the first lane behind the slots — at 256, 512 and 65 536 in a workgroup of its own"""
    I = cached(("i2", S), lambda: i2_full(S))
    assert I["run"] <= 4
    v, keep = hv.make_indels(route, I)
    want, order, got = check(route, v, ("i2", S), I, 0, I["n_pos"], "I2 M = S = %d" % S, short=True)
    assert want["pos"].shape[1] == S and sorted(order.tolist()) == list(range(S))


@pytest.mark.parametrize("M", [0, 1, 256, 257])
def test_i2_some_slots_live(route, M):
    """M of 1000: at 256 the scan's closing element i + 1 == count falls on lane 255 of the first tile and the later tiles are idle"""
    I = cached(("i2some", M), lambda: i2_some(M))
    v, keep = hv.make_indels(route, I)
    want, order, got = check(route, v, ("i2some", M), I, 500, 600, "I2 M = %d of 1000" % M, short=True, slack=2)
    assert want["pos"].shape[1] == M
    check(route, v, ("i2some", M), I, 0, 2000, "I2 M = %d of 1000, every position" % M)


# ------------------------------------------------------------------------------------------------ I3 order

X = 7000                                      # the position of I3's records: behind the reference (every deleted base spells N)


def i3_slots(n_lib=3):
    """libraries 2, 0, 1 in that order; per library the eleven texts, one slot twice byte for byte, and "+AC" from another read"""
    slots, t = [], 0
    for lib in (2, 0, 1)[:n_lib]:
        for text in ("+ACT", "+A", "-NNNNN", "+=", "+ACG", "+AN", "-N", "+AT", "+AC", "+A=", "-NN"):
            t += 1
            if text[0] == "+":
                rr, rq, ln = SPELL[text]
                slots.append(hv.slot(X, lib, ln, rr, rq, tag=t))
            else:
                slots.append(hv.slot(X, lib, 1 - len(text), 0, 0, tag=t))
        slots.append(list(slots[-3]))                                     # "+AC" byte for byte (the same tag)
        t += 1; slots.append(hv.slot(X, lib, 2, 4, -1, tag=t))            # "+AC" spelled by read 4
        t += 1; slots.append(hv.slot(X, lib, -2, 9, 9, tag=t))            # "-NN" with another body
    return slots


def i3_case(order):
    slots = i3_slots()
    S = len(slots)
    perm = {"ascending": list(range(S)), "descending": list(range(S))[::-1], "shuffled": list(np.random.default_rng(3).permutation(S))}[order]
    return hv.indel_arrays([slots[i] for i in perm], READS, ref=b"ACGT", ref_lo=0, pos0=X - 3, n_pos=10, n_lib=3, max_run=S)


def assert_permutation_in_slot_order(I, want, order, got, m):
    rows = np.concatenate([got[k][:hv.DEST_PLANES[k] * m].reshape(hv.DEST_PLANES[k], m) for k in ("pos", "lib", "len", "rep_read", "rep_qpos", "istat", "fstat")]).T
    live = I["slots"][I["slots"][:, 2] != 0]
    assert sorted(map(bytes, rows)) == sorted(map(bytes, live)), "the output is no permutation of the live slots"
    text = [bytes(want["alleles"][want["allele_off"][r]:want["allele_off"][r + 1]]) for r in range(m)]
    keys = [(int(want["pos"][0, r]), int(want["lib"][0, r]), text[r]) for r in range(m)]
    ties = [r for r in range(m - 1) if keys[r] == keys[r + 1]]
    assert all(order[r] < order[r + 1] for r in ties)
    return len(ties)


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_i3_order_inside_one_position(route, order):
    I = cached(("i3", order), lambda: i3_case(order))
    v, keep = hv.make_indels(route, I)
    want, perm, got = check(route, v, ("i3", order), I, 0, I["n_pos"], "I3 " + order)
    m = want["pos"].shape[1]
    assert m == 42 and want["lib"][0].tolist() == [0] * 14 + [1] * 14 + [2] * 14
    text = [bytes(want["alleles"][want["allele_off"][r]:want["allele_off"][r + 1]]).decode() for r in range(14)]
    assert text == ["+=", "+A", "+A=", "+AC", "+AC", "+AC", "+ACG", "+ACT", "+AN", "+AT", "-N", "-NN", "-NN", "-NNNNN"]     # bytes order, not bucket order
    assert assert_permutation_in_slot_order(I, want, perm, got, m) == 3 * 3


def i3_wave_case():
    """72 records at one position (more than a wave ranks the run): 4 libraries x 9 texts, every text twice with different bodies"""
    slots, t = [], 0
    for lib in range(4):
        for text in ("+ACT", "+A", "+=", "+ACG", "+AN", "+AT", "+AC", "+A="):
            for _ in range(2):
                t += 1
                rr, rq, ln = SPELL[text]
                slots.append(hv.slot(X, lib, ln, rr, rq, tag=t))
        for _ in range(2):
            t += 1; slots.append(hv.slot(X, lib, -3, 0, 0, tag=t))
    slots = [slots[i] for i in np.random.default_rng(72).permutation(len(slots))]
    return hv.indel_arrays(slots, READS, pos0=X, n_pos=1, n_lib=4, max_run=72)


def test_i3_a_run_across_a_wave_with_equal_pairs(route):
    I = cached("i3wave", i3_wave_case)
    assert I["run"] == 72
    v, keep = hv.make_indels(route, I)
    want, perm, got = check(route, v, "i3wave", I, 0, 1, "I3 72 records")
    assert assert_permutation_in_slot_order(I, want, perm, got, 72) == 36


# ------------------------------------------------------------------------------------------------ I4 spelling

I4_P = 72100
RAW = b"ACGTacgtnRYKNM\xe9*"


def i4_case(pos0, with_ref=True, ref_len_short=True):
    """one record per position: every insertion rule, every deletion rule.  The slice [ref_lo, ref_hi) = pos0 + [1000, 72000) holds raw
    upper- and lower-case, IUPAC and 0xE9 bytes and one NUL; ref_len lies 10 below ref_hi (or 100 above)."""
    lo, hi = pos0 + 1000, pos0 + 72000
    rl = hi - 10 if ref_len_short else hi + 100
    ref = bytearray(RAW * ((hi - lo) // len(RAW) + 1))[:hi - lo]
    ref[52] = 0
    lq0, lq3 = len(READS[0]), len(READS[3])
    n_reads = len(READS)
    ins = [(16, 0, -1), (16, 1, 0),                                             # all 16 codes from an even and an odd q
           (3, 3, -1), (3, 3, -2), (3, 3, lq3 - 2), (2, 3, lq3 - 1), (4, 3, lq3 - 3), (2, 3, -5), (3, 0, lq0 - 1),
           (2, n_reads - 1, 0), (2, n_reads, 0), (2, hv.U32, 0), (2, 1 << 31, 0),    # the last read, one behind it, 0xFFFFFFFF
           (2, 2, -1), (1, 2, 0),                                               # a read with l_qseq == 0
           (300, 5, 4), (300, 5, 20)]                                           # text offsets beyond 2^16 behind the long deletion
    dels = [(lo - 3, 5), (lo - 1, 1), (lo - 2, 1), (hi - 3, 5), (rl - 3, 5), (rl - 1, 1), (rl - 2, 1), (lo + 49, 5), (lo + 51, 1), (lo + 100, 33),
            (lo + 10, 70000), (pos0 + 1, 3), (pos0 + I4_P - 1, 4)]
    slots, t = [], 0
    for j, (ln, rr, rq) in enumerate(ins):
        t += 1; slots.append(hv.slot(pos0 + 3 * j, j % 2, ln, rr, rq, tag=t))
    for j, (p, ln) in enumerate(dels):
        t += 1; slots.append(hv.slot(p, j % 2, -ln, 0, 0, tag=t))
    slots = [slots[i] for i in np.random.default_rng(4).permutation(len(slots))]
    return hv.indel_arrays(slots, READS, ref=bytes(ref) if with_ref else None, ref_lo=lo if with_ref else 0, ref_len=rl if with_ref else 0, pos0=pos0, n_pos=I4_P, n_lib=2)


I4_VARIANTS = {"pos0_0": (0, True, True), "pos0_high": (2 ** 31 - 1 - I4_P, True, True), "ref_len_above": (0, True, False), "no_ref": (0, False, True)}


def test_i4_the_reference_spells_what_the_rules_say():
    """the constructed texts, spelled out by hand for the rules that matter most (so the reference itself is held)"""
    I = cached(("i4", "pos0_0"), lambda: i4_case(*I4_VARIANTS["pos0_0"]))
    want, order = reference(("i4", "pos0_0"), I, 0, I4_P)
    text = {int(want["pos"][0, r]): bytes(want["alleles"][want["allele_off"][r]:want["allele_off"][r + 1]]) for r in range(want["pos"].shape[1])}
    assert text[0] == b"+=ACNGNNNTNNNNNNN" and text[3] == text[0]             # "=ACMGRSVTWYHKDBN": ten of the sixteen codes spell N
    assert text[6] == b"+ACG" and text[9] == b"+NAC" and text[12] == b"+TNN" and text[15] == b"+NN" and text[18] == b"+CTNN" and text[21] == b"+NN"
    assert text[24] == b"+NNN" and text[27] == ("+" + "".join(hv.NIBBLE[c] for c in READS[5][1:3])).encode() != b"+NN"
    assert text[30] == text[33] == text[36] == b"+NN" and text[39] == b"+NN" and text[42] == b"+N"
    assert text[997] == b"-NNACG" and text[999] == b"-A" and text[998] == b"-N"                              # ref_lo - 1 | ref_lo
    rl = I["ref_len"]
    assert text[rl - 3] == b"-" + bytes(I["ref"][rl - 2 - 1000:rl - 1000]) + b"NNN" and text[rl - 1] == b"-N" and len(text[rl - 2]) == 2 and text[rl - 2] != b"-N"
    assert text[71997] == b"-NNNNN"                                                                       # behind ref_len although the slice has bytes
    assert text[1051] == b"-N" and text[1049][3:4] == b"N" and b"\xe9" in text[1100] and b"a" in text[1100] and b"R" in text[1100]
    assert len(text[1010]) == 70001 and int(want["allele_off"][-1]) > 2 ** 16 and text[0 + I4_P - 1] == b"-NNNN"
    above = reference(("i4", "ref_len_above"), cached(("i4", "ref_len_above"), lambda: i4_case(*I4_VARIANTS["ref_len_above"])), 0, I4_P)[0]
    t2 = {int(above["pos"][0, r]): bytes(above["alleles"][above["allele_off"][r]:above["allele_off"][r + 1]]) for r in range(above["pos"].shape[1])}
    assert t2[71997][:3] == b"-" + bytes(I["ref"][70998:71000]) and t2[71997][3:] == b"NNN"                 # ref_hi - 1 | ref_hi


@pytest.mark.parametrize("variant", list(I4_VARIANTS))
def test_i4_every_rule_that_spells_an_allele(route, variant):
    I = cached(("i4", variant), lambda: i4_case(*I4_VARIANTS[variant]))
    v, keep = hv.make_indels(route, I)
    want, order, got = check(route, v, ("i4", variant), I, 0, I4_P, "I4 " + variant, short=True)
    assert want["pos"].shape[1] == len(I["slots"])
    if variant == "no_ref":
        text = bytes(want["alleles"])
        assert v.ref is None and text.count(b"-" + b"N" * 70000) == 1


# ------------------------------------------------------------------------------------------------ I5 window edges

def i5_case():
    """a window [first, first + n) = pos0 + [20, 50): records on first - 1, first, first + n - 1 and first + n, a dead one inside"""
    slots = [hv.slot(1019, 0, 2, 3, -1, tag=1), hv.slot(1020, 0, 2, 3, -1, tag=2), hv.slot(1049, 1, -2, 0, 0, tag=3), hv.slot(1050, 1, 3, 3, 0, tag=4),
             hv.slot(1030, 0, 0, 3, -1, tag=5), hv.slot(1020, 1, -1, 0, 0, tag=6), hv.slot(1049, 0, 1, 3, 4, tag=7)]
    return hv.indel_arrays(slots, READS, ref=b"ACGTACGTAC" * 8, ref_lo=1000, pos0=1000, n_pos=80, n_lib=2)


I5_WINDOWS = [(20, 30), (19, 1), (20, 1), (49, 1), (50, 1), (19, 32), (21, 28), (30, 1), (0, 80), (79, 1)]


def test_i5_window_edges_empty_windows_and_views_without_slots(route):
    I = cached("i5", i5_case)
    v, keep = hv.make_indels(route, I)
    for k0, n in I5_WINDOWS:
        want, order, got = check(route, v, "i5", I, k0, n, "I5 window %r" % ((k0, n),), slack=1)
    assert [reference("i5", I, k0, n)[0]["pos"].shape[1] for k0, n in I5_WINDOWS] == [4, 1, 2, 2, 1, 6, 0, 0, 6, 0]
    # n == 0 and n_slots == 0: the counts and allele_off[0] are cleared, nothing else is written
    none = capi.DeviceIndels.from_buffer_copy(v); none.n_slots = 0; none.slots = None
    for view, k0, n in ((v, 25, 0), (v, 80, 0), (none, 20, 30)):
        rc, counts, got = ti.gather(route, view, k0, n, 4, 16, ws_bytes=0)
        assert rc == 0 and counts.tolist() == [0, 0], (k0, n)
        assert got["allele_off"][0] == 0 and (got["allele_off"][1:] == hv.SENT).all()
        assert all((got[k] == (hv.SENT8 if k == "alleles" else hv.SENT)).all() for k in DESTS if k != "allele_off")


# ------------------------------------------------------------------------------------------------ the host sanitizers

def test_handmade_views_under_the_host_sanitizers(tmp_path):
    """I3 (shuffled), I4, I5 and I2 at M = S = 257 through indels_check_asan: sources of exactly the view's sizes, a scratch of exactly
    brc_indels_workspace bytes, destinations of exactly the contract's sizes; exact capacities and capacities one short."""
    cases = [(("i3", "shuffled"), lambda: i3_case("shuffled"), [(0, 10)]), (("i4", "pos0_0"), lambda: i4_case(*I4_VARIANTS["pos0_0"]), [(0, I4_P)]),
             (("i4", "no_ref"), lambda: i4_case(*I4_VARIANTS["no_ref"]), [(0, I4_P)]),
             (("i4", "ref_len_above"), lambda: i4_case(*I4_VARIANTS["ref_len_above"]), [(0, I4_P)]),     # (a deletion across ref_hi: one byte further is outside the slice)
             ("i5", i5_case, I5_WINDOWS), (("i2", 257), lambda: i2_full(257), [(0, 67), (1, 64)])]
    for key, make, windows in cases:
        I = cached(key, make)
        calls = []
        for k0, n in windows:
            want, _ = reference(key, I, k0, n)
            m, nb = want["pos"].shape[1], int(want["alleles"].size)
            calls += [(k0, n, m, nb)] + ([(k0, n, m - 1, nb - 1)] if m else [])
        d = hv.run_checker("indels", hv.serialize_indels(I, calls), tmp_path, "%d calls" % len(calls))
        o = 0
        for k0, n, cap, acap in calls:
            want, _ = reference(key, I, k0, n)
            assert d[o:o + 4].view(np.int32)[0] == 0; o += 4
            assert d[o:o + 8].view(np.uint32).tolist() == [want["pos"].shape[1], want["alleles"].size]; o += 8
            got = {}
            for k in DESTS:
                nbytes = acap if k == "alleles" else 4 * (cap + 1 if k == "allele_off" else hv.DEST_PLANES[k] * cap)
                got[k] = d[o:o + nbytes] if k == "alleles" else d[o:o + nbytes].view(np.uint32); o += nbytes
            ti.assert_table(got, want, cap, acap, "asan %r %r" % (key, (k0, n, cap, acap)))
        assert o == d.size
