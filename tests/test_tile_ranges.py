"""The stage between the annotators and k_pileup2 — the piece range [lo, hi) of every (64-position tile, library) (k_reach_blockmax,
k_scan_aggregates<OpMaxU64>, k_tiles_all, k_narrow_tiles) and the tile-major copy of the live pieces (k_count_piece_tiles /
k_compact_tiles<true>, scan<OpSumU32>, k_compact_reads / k_compact_tiles<false>) — at the boundaries of its own index arithmetic, on batches
written down by hand (constructed.Reads; the one large family builds its arrays with numpy).  Families: T ranges (piece counts around a
thread's 4, a wave's 256 and a block's 1024 pieces; the running maximum carried by lanes, waves and block aggregates; tile arithmetic; gaps;
libraries; more than 1024 block aggregates), S the sum scan at 16- and 4096-element boundaries, C compaction (the 64-ary search, reads per
group, the group of 8 tiles, copy rounds, rare records, announced windows, the range walk, the life of an engine, the product's own rule).

Every batch is pushed WHOLE for every region it is run over (the read stream, and with it every piece index against thread, wave and block
boundaries, is the same for all of them): the whole region, then — on every small batch — every single-tile region of it.  Routes, in this
order: (1) CPU: oracle == [sim], and the cells the batch was built for asserted from the simulator's WITNESS; (2) the bounds-checked build
(it reads BRC_COMPACT_TILES: 1 and 2); (3) the test-knobs library with BRC_COMPACT_TILES = 1 (one library: k_compact_reads), 2
(k_compact_tiles) and 0 (no compaction); (4) the product library, which compacts by its own rule (more than 12 pieces per read).  All
comparisons are equalities of bits and bytes: planes, indel lists, text, device text.

A range that is too wide changes no compared byte (k_pileup2 skips pieces that do not touch the tile), so every device route also asserts
eng.piece_steps() == the witness's (ranged, live_clipped | live) of the same region — per single-tile region too, so that errors cannot
compensate inside a sum.  The witness (tests/sim/brc_sim.cpp: brc_sim_witness) speaks for the device because tile_range2 is the stated
definition that k_tiles_all inverts, the trimming is k_narrow_tiles' two loops, and walk_pieces, piece_off, lib_base and wanted_tiles come
from the same host code for both backends.

Two cells the design names cannot be built, and the tests assert the opposite instead (DESIGN.md §5 has the argument): a tile whose range
STARTS behind its neighbour's (range_starts_behind_next is 0 for every batch, announced windows included), and an empty-range tile between
two tiles the same read is live in (a read's extents have no gaps: it is in the middle tile's range).  Left out: the second round of
k_scan_aggregates<OpSumU32> (268 M positions) and k_compact_reads' overflow flag (no input reaches it when the kernels are right)."""
import ctypes
import json
import os

import numpy as np
import pytest

import parity
from bam_readcount_amd import capi
from conftest import ROOT
from constructed import OTHER, THIRD, Reads, ACGT_CODE, checked_lib, mismatches, ref_of  # noqa: F401  (checked_lib: fixture)

TILE, TR_ITEMS, TR_WAVE, TR_CHUNK, SCAN_ITEMS, SCAN_CHUNK, CR_GROUP, PRODUCT_RULE = 64, 4, 256, 1024, 16, 4096, 8, 12
LONG = [(4, 250), (0, 100), (4, 250)]                                 # 600 bases (PF_HUGE), soft-clipped to 100 aligned ones
NAMES3 = ["libA", "libB", "libC"]


class Case:
    def __init__(self, ref, arrs, region, cells, opts=None, names=(), windows=None, singles=True, passes=1, check_warn=True, extra_regions=(), knob0=True, min_lines=1):
        self.ref, self.arrs, self.region, self.cells = ref, arrs, region, cells
        self.opts, self.names, self.windows, self.singles, self.passes, self.check_warn = opts or {}, names, windows, singles, passes, check_warn
        self.extra_regions, self.knob0, self.min_lines = list(extra_regions), knob0, min_lines


# ------------------------------------------------------------------------------------------------ the ranges, stated in numpy

def pieces_of(arrs):
    """(key, reach) of every piece of a one-library batch of counting reads without -i, as walk_pieces cuts them: one piece per M operator,
    its column running to the next M operator's start (a leading deletion: a column-only piece)"""
    key, reach = [], []
    for i in range(len(arrs["pos"])):
        pos = int(arrs["pos"][i]); x = pos; starts = []
        for c in arrs["cigar"][int(arrs["cigar_off"][i]):int(arrs["cigar_off"][i]) + int(arrs["n_cigar"][i])]:
            op, l = int(c) & 15, int(c) >> 4
            if op in (0, 7, 8) and l:
                if not starts and x > pos:
                    starts.append(pos)
                starts.append(x)
            if op in (0, 2, 3, 7, 8):
                x += l
        if not (int(arrs["flag"][i]) & 4) and (starts or x > pos) and not (int(arrs["n_cigar"][i]) == 1 and not starts):
            starts = starts or [pos]
            key += [pos] * len(starts); reach += starts[1:] + [x]
    return np.array(key, np.int64), np.array(reach, np.int64)


def ranges_np(key, reach, pos0, P):
    ntiles = (P + TILE - 1) // TILE
    p0 = pos0 + TILE * np.arange(ntiles, dtype=np.int64)
    prefmax = np.maximum.accumulate(reach) if len(reach) else reach
    lo = np.searchsorted(prefmax, p0, "right")
    hi = np.maximum(lo, np.searchsorted(key, p0 + TILE - 1, "right"))
    return lo, hi


def formula_holds(case, ws, key=None, reach=None):
    """the numpy statement of the ranges == the witness, on every region of the batch"""
    if key is None:
        key, reach = pieces_of(case.arrs)
    assert len(key) == ws[0]["n_pieces"]
    for w in ws:
        lo, hi = ranges_np(key, reach, w["pos0"], w["P"])
        assert (int((hi - lo).sum()), int((hi - lo).max(initial=0))) == (w["ranged"], w["range_max"]), (w["pos0"], w["P"])
    return ranges_np(key, reach, ws[0]["pos0"], ws[0]["P"])


def plain(R, pos, j=0, L=3, **kw):
    kw.setdefault("flag", (0, 16)[j & 1])
    R.add(pos, [(0, L)], edit=mismatches([0], OTHER) if j % 5 == 1 else None, nm=j % 3, sm=(7 * j) % 50, **kw)


# ------------------------------------------------------------------------------------------------ T. ranges

T1_COUNTS = [1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2049]


def case_t1(n):
    """n reads of one piece, four to a position: load_keyreach4's 16-byte path and its tail, the next thread's key at b + 4 == n, at a wave
    and at a block boundary"""
    ref = ref_of(1024); R = Reads(ref)
    for j in range(n):
        plain(R, 70 + j // 4, j)

    def cells(ws):
        assert ws[0]["n_pieces"] == n and ws[0]["Lp"] == 1 and ws[0]["pos0"] == 70
        formula_holds(case, ws)
    case = Case(ref, R.arrays(), (1, 1000), cells)
    return case


T2_FIRST = [0, 3, 4, 255, 256, 1023, 1024]


def case_t2(k):
    """k reads, then 1M 600D 1M as piece k, then 2200 reads of one piece under its deletion, all reaching less: lo of the tiles under the
    deletion is piece k across more than two blocks of pieces — the running maximum carried by lanes, by waves (sh[w]) and by agg[]"""
    ref = ref_of(2048); R = Reads(ref)
    for j in range(k):
        plain(R, 100 + j // 8, j)
    R.add(300, [(0, 1), (2, 600), (0, 1)])
    for j in range(2200):
        plain(R, 301 + j // 4, j, L=2)

    def cells(ws):
        assert ws[0]["n_pieces"] == k + 2 + 2200
        lo, hi = formula_holds(case, ws)
        under = lo == k
        assert under.sum() >= 9 and int((hi[under] - k).max()) > 2 * TR_CHUNK        # piece k opens ranges that end more than two blocks behind it
        assert ws[0]["range_max"] > 2 * TR_CHUNK
    case = Case(ref, R.arrays(), (1, 1500), cells)
    return case


def case_t3(o):
    """pos0 % 64 == o; reads wholly before the region, from before it into it, reaching 64 k and 64 k + 1 behind pos0, starting on p1(t)
    and p1(t) + 1, wholly behind the region; the region ends inside a tile"""
    ref = ref_of(2048); R = Reads(ref)
    pos0 = 640 + o; end = pos0 + 5 * TILE + 20
    for j in range(6):
        plain(R, 100 + 40 * j, j, L=10)                              # wholly before
    R.add(pos0 - 30, [(0, 50)]); R.add(pos0 - 70, [(0, 70)]); R.add(pos0 - 70, [(0, 71)])      # into the region; reaching pos0 and pos0 + 1
    R.add(pos0 + 54, [(0, 10)]); R.add(pos0 + 54, [(0, 11)])        # reach - pos0 == 64, 65
    R.add(pos0 + 100, [(0, 5), (2, 23), (0, 5)]); R.add(pos0 + 100, [(0, 5), (2, 24), (0, 5)])      # ... of a first piece: 128, 129
    R.add(pos0 + 2 * TILE + 63, [(0, 8)]); R.add(pos0 + 3 * TILE, [(0, 8)])      # key == p1(2), p1(2) + 1
    R.add(pos0 + 3 * TILE + 63, [(0, 8)]); R.add(pos0 + 4 * TILE, [(0, 8)])
    R.add(end - 5, [(0, 30)])                                        # over the region's end
    R.add(end + 3, [(0, 9)])                                         # behind the region, inside its last tile
    for j in range(5):
        plain(R, end + 100 + 70 * j, j, L=10)                        # wholly behind

    def cells(ws):
        w = ws[0]
        assert w["pos0"] == pos0 and w["pos0"] % TILE == o and w["P"] == end - pos0 and w["P"] % TILE == 20 and w["ntiles"] == 6
        key, reach = pieces_of(case.arrs)
        assert {pos0, pos0 + 1, pos0 + 64, pos0 + 65, pos0 + 128, pos0 + 129} <= set(reach.tolist())
        assert {pos0 + 2 * TILE + 63, pos0 + 3 * TILE, pos0 + 3 * TILE + 63, pos0 + 4 * TILE} <= set(key.tolist())
        assert (reach <= pos0).sum() >= 7 and (key >= end).sum() >= 6 and (key < pos0).sum() >= 9 and ((key < pos0) & (reach > pos0)).sum() >= 2
        formula_holds(case, ws, key, reach)
    case = Case(ref, R.arrays(), (pos0 + 1, end), cells)
    return case


def case_t4():
    """a read without a match operator at the region's start, three empty tiles, one piece, 300 empty tiles, one piece, three empty tiles up
    to a second read without a match operator: one piece owns hundreds of tiles' hi, the next their lo; the r == s0 and r == s1 - 1 fills"""
    ref = ref_of(22_000); R = Reads(ref)
    a = 200 + 3 * TILE + 10; b = a + 300 * TILE + 7; z = b + 3 * TILE + 40
    R.add(200, [(4, 5)]); R.add(a, [(0, 5)]); R.add(b, [(0, 5)], edit=mismatches([1], OTHER)); R.add(z, [(4, 5)])

    def cells(ws):
        w = ws[0]
        assert w["n_pieces"] == 2 and w["n_reads"] == 4 and w["pos0"] == 200 and w["P"] == z - 200 and w["ntiles"] > 300
        lo, hi = formula_holds(case, ws)
        assert (hi[:3] == 0).all() and (lo[-3:] == 2).all() and ((lo == 1) & (hi == 1)).sum() >= 299 and w["ranged"] == 2
    case = Case(ref, R.arrays(), (1, 21_000), cells)
    return case


T5_SIZES = [(5, 6, 7), (6, 2, 9), (7, 4, 4), (256, 768, 3), (255, 769, 3), (0, 7, 5), (7, 0, 5), (7, 5, 0), (1, 9, 1)]


def case_t5(sizes):
    """-p with three names: library l has sizes[l] pieces.  The first library's second read is 1M 500D 1M, so that every reach of the later
    libraries is below an earlier library's maximum; two library-less reads among them"""
    ref = ref_of(2048); R = Reads(ref)
    for l, n in enumerate(sizes):
        j = 0; left = n
        while left > 0:
            if l == 0 and j == 1 and left >= 2:
                R.add(100 + j, [(0, 1), (2, 500), (0, 1)], lib=l); left -= 2
            else:
                plain(R, 100 + 11 * l + j, j, L=4, lib=l); left -= 1
            j += 1
    R.add(130, [(0, 20)], lib=-1); R.add(400, [(0, 20)], lib=-1)
    bounds = np.cumsum(sizes)[:2]

    def cells(ws):
        w = ws[0]
        assert w["Lp"] == 3 and w["n_pieces"] == sum(sizes) and w["n_reads"] == len(case.arrs["pos"])
        assert (np.bincount(case.arrs["lib"][case.arrs["lib"] >= 0], minlength=3) > 0).tolist() == [n > 0 for n in sizes]
    case = Case(ref, R.arrays(), (1, 1500), cells, opts=dict(per_lib=True), names=NAMES3, check_warn=False)
    case.bounds = bounds
    return case


def t5_census():
    """the library boundaries of the T5 batches: on each of a thread's 4 pieces, on a wave and on a block boundary"""
    b = np.concatenate([np.cumsum(s)[:2] for s in T5_SIZES if min(s) > 0])
    assert set((b % TR_ITEMS).tolist()) == {0, 1, 2, 3} and TR_WAVE in b and TR_CHUNK in b and (TR_WAVE - 1) in b
    assert {tuple(int(n == 0) for n in s) for s in T5_SIZES} >= {(1, 0, 0), (0, 1, 0), (0, 0, 1)} and (1, 9, 1) in T5_SIZES


def case_t6(first):
    """`first` reads of one base (1M), 15 to a position; then 1M 600D 1M, whose first piece is piece `first` — the last piece of block
    aggregate 1023 or the first of aggregate 1024 —; then more than 8 blocks of 1M reads under its deletion.  k_scan_aggregates' second round
    of 1024 and its carry.  Built vectorised."""
    n = first + 1 + 8800
    ar = np.arange(n, dtype=np.int64)
    pos = 100 + ar // 15
    isd = ar == first
    ref = ref_of(int(pos[-1]) + 2000); code = ACGT_CODE[ref]
    L = np.where(isd, 2, 1)
    nc = np.where(isd, 3, 1)
    cigar = np.full(n + 2, 1 << 4, np.int64); cigar[first + 1] = (600 << 4) | 2
    b0 = code[pos].astype(np.int64)
    b0[ar % 7 == 3] = OTHER[b0[ar % 7 == 3]]
    seq4 = b0 << 4
    seq4[first] |= int(code[pos[first] + 601])
    qual = np.insert(20 + (ar * 3) % 21, first + 1, 33)
    arrs = dict(pos=pos, flag=np.where(ar % 2 == 0, 16, 0), mapq=np.array([60, 47, 29])[ar % 3], lib=np.zeros(n), l_qseq=L, n_cigar=nc, cigar_off=np.cumsum(nc) - nc,
                seq_off=ar, qual_off=np.cumsum(L) - L, nm=ar % 2, sm=(ar * 7) % 61, tags=np.full(n, 3), cigar=cigar, seq4=seq4, qual=qual)
    arrs = {k: np.asarray(arrs[k]).astype(dt) for k, dt in capi.BATCH_DTYPES.items()}
    key = np.insert(pos, first + 1, pos[first]); reach = key + 1; reach[first] = pos[first] + 601; reach[first + 1] = pos[first] + 602

    def cells(ws):
        w = ws[0]
        assert w["n_pieces"] == n + 1 > TR_CHUNK * 1024 + 8 * TR_CHUNK and first // TR_CHUNK in (1023, 1024) and first % TR_CHUNK in (TR_CHUNK - 1, 0)
        lo, hi = formula_holds(case, ws, key, reach)
        under = lo == first
        assert under.sum() >= 9 and int((hi[under] - first).max()) > 8 * TR_CHUNK and w["range_max"] > 8 * TR_CHUNK
    case = Case(ref, arrs, (1, int(pos[-1]) + 100), cells, singles=False, min_lines=60_000)
    return case


# ------------------------------------------------------------------------------------------------ S. scan<OpSumU32>

S_SHAPES = [(1, 0), (1, 1), (1, 14), (1, 15), (1, 16), (1, 4094), (1, 4095), (1, 4096), (1, 8192), (3, 0), (3, 5), (3, 6), (3, 1365), (3, 1366)]


def case_s(Lp, ntiles):
    """a sparse region of ntiles tiles and Lp libraries (ntiles Lp + 1 compaction counts: 1, 2, 15, 16, 17, 4095, 4096, 4097, 8193 with one
    library; 1, 16, 19, 4096, 4099 with three — 3 t + 1 takes no other of those values): live pieces, a third-allele event, a deletion and
    an insertion of every library in the first tile, the last two tiles and the tiles on both sides of every 16- and 4096-element boundary
    of both slot orders (library-major: the compaction counts; tile-major: the third-allele counts)"""
    pos0 = 300
    ref = ref_of(pos0 + TILE * max(ntiles, 4) + 1000); R = Reads(ref)
    if ntiles == 0:                                                   # no read reaches the region: no tile, one scan element
        for l in range(Lp):
            plain(R, 100 + l, l, L=20, lib=l)
        region = (5000, 5100) if len(ref) > 5200 else (1200, 1250)
    else:
        nslot = ntiles * Lp
        edges = [s for e in range(SCAN_ITEMS, nslot + 2, SCAN_ITEMS) if e % SCAN_CHUNK == 0 or e <= 2 * SCAN_ITEMS for s in (e - 1, e)]
        tiles = {0, ntiles - 1, max(ntiles - 2, 0)} | {s % ntiles for s in edges if s < nslot} | {s // Lp for s in edges if s < nslot}
        for t in sorted(tiles):
            p = pos0 + TILE * t + (0 if t == 0 else 5)
            for l in range(Lp):
                R.add(p, [(0, 30)], lib=l); R.add(p, [(0, 30)], lib=l, edit=mismatches([3], OTHER), flag=16); R.add(p, [(0, 30)], lib=l, edit=mismatches([3], THIRD))
                R.add(p, [(0, 10), (2, 3), (0, 10)], lib=l); R.add(p, [(0, 10), (1, 2), (0, 10)], lib=l, flag=16)
        region = (pos0 + 1, pos0 + TILE * (ntiles - 1) + 30)
        if ntiles > 1:
            assert pos0 + TILE * (ntiles - 1) + 5 + 30 >= region[1]    # the last cluster reaches the region's end

    def cells(ws):
        w = ws[0]
        assert (w["Lp"], w["ntiles"]) == (Lp, ntiles) and w["n_reads"] <= 600
        if ntiles:
            assert w["pos0"] == pos0 and w["live"] >= 7 * Lp * min(len(tiles), ntiles)
    kw = dict(opts=dict(per_lib=True), names=NAMES3) if Lp == 3 else {}
    return Case(ref, R.arrays(), region, cells, singles=False, min_lines=0 if ntiles == 0 else 20, **kw)


# ------------------------------------------------------------------------------------------------ C. compaction

C1_READS = [1, 2, 63, 64, 65, 4095, 4096, 4097]


def case_c1(n):
    """n reads (those without pieces included); the groups of 8 tiles begin in chosen reads: the first, the last, and the reads on the
    stride boundaries of the 64-ary search's levels; runs of three reads without pieces (unmapped; without a match operator) directly before
    and behind them"""
    stride = (n + 63) // 64
    targets = sorted({0, 1, n // 2, n - 2, n - 1} | {s * stride + d for s in (1, 2, 63) for d in (-2, -1, 0, 1)} | {stride + stride // 64 + d for d in (-1, 0, 1)})
    targets = [t for t in targets if 0 <= t < n]
    firsts = [t for i, t in enumerate(targets) if i == 0 or t >= targets[i - 1] + 1]
    ref = ref_of(512 * (len(firsts) + 2) + 600); R = Reads(ref)
    kinds = np.ones(n, np.int64)                                      # 1: a read of one piece; 0: a read without pieces
    if n >= 63:
        for f in firsts:
            if f >= 4 and not set(range(f - 3, f)) & set(firsts):
                kinds[f - 3:f] = 0
            if f + 4 < n and not set(range(f + 1, f + 4)) & set(firsts):
                kinds[f + 1:f + 4] = 0
    g = -1; at = 0
    for i in range(n):
        if g + 1 < len(firsts) and i == firsts[g + 1]:
            g += 1; at = 0
        p = 100 + 512 * g + 10 + at // 12
        if kinds[i]:
            plain(R, p, i)
        elif i & 1:
            R.add(p, [(4, 5)])
        else:
            R.add(p, [(0, 3)], flag=4)
        at += 1

    def cells(ws):
        w = ws[0]
        assert w["n_reads"] == n and w["n_pieces"] == int(kinds.sum()) and w["Lp"] == 1
        # every single-tile region's range starts in the read its tile was built to start in: the first slots the search was asked for
        owner = np.nonzero(kinds)[0]                                  # piece -> read
        key, reach = pieces_of(case.arrs)
        starts = set()
        for x in ws[1:]:
            lo, hi = ranges_np(key, reach, x["pos0"], x["P"])
            starts |= {int(owner[a]) for a, b in zip(lo, hi) if a < b}
        assert set(firsts) <= starts, sorted(set(firsts) - starts)
        assert {0, n - 1} <= set(firsts)
        if n >= 63:
            f = np.array(firsts)
            before = [x for x in f if x >= 3 and not kinds[x - 3:x].any()]; behind = [x for x in f if x + 3 < n and not kinds[x + 1:x + 4].any()]
            assert len(before) >= 2 and len(behind) >= 2 and kinds[f].all()
    case = Case(ref, R.arrays(), (1, 100 + 512 * len(firsts) + 40), cells)
    return case


C2_READS = [64, 65, 128, 129]


def case_c2(n):
    """10 reads in the first group of 8 tiles, n in the second — the first 64 of them end before the group's third tile, where the others
    begin —, 40 in the third: rounds of 64 reads, the round behind the last useful one cut by the a0 < gy ballot"""
    ref = ref_of(2200); R = Reads(ref)
    T = 128                                                           # pos0: the first read's position
    for j in range(10):
        R.add(T + 20 * j, [(0, 5), (2, 2), (0, 5)])
    for j in range(n):
        R.add(T + 512 + (j if j < 64 else 128 + 2 * (j - 64)), [(0, 6), (2, 3), (0, 6), (1, 1), (0, 6)])
    for j in range(40):
        R.add(T + 1024 + 5 * j, [(0, 5), (2, 2), (0, 5)])

    def cells(ws):
        w = ws[0]
        assert w["pos0"] == T and w["reads_max"] == n and w["n_reads"] == n + 50 and w["n_pieces"] == 20 + 3 * n + 80
    return Case(ref, R.arrays(), (1, 2000), cells)


def rare_reads(R, pos, q):
    """C5: a soft-clipped read, a read with an escape base (wide), a read long enough for PF_HUGE, a read that is not counted (a column-only
    piece), a duplicate (in the column, not counted) — one piece each, all covering pos + 3 .. pos + 19"""
    def nbase(seq, qual, aq, ar, code):
        seq[aq[4]] = 15
    R.add(pos, [(4, 7), (0, 20), (4, 9)]); R.add(pos + 1, [(0, 20)], edit=nbase); R.add(pos + 2, LONG); R.add(pos + 3, [(0, 20)], mapq=q - 1); R.add(pos + 3, [(0, 20)], flag=1024)
    return 5


def has_rare_reads(arrs, q):
    op = arrs["cigar"] & 15
    sq = arrs["seq4"]
    return bool((op == 4).any() and ((sq >> 4) == 15).any() and (arrs["l_qseq"] >= 600).any() and (arrs["mapq"] < q).any() and (arrs["flag"] & 1024).any())


C3_TILES = [8, 31, 33]


def case_c3(ntiles):
    """ntiles % 8 = 0, 7, 1 (% 32: 8, 31, 1).  In the first group: a read that enters the group at its third tile; one piece live in three
    consecutive tiles; pieces whose extents end on p0 and on p0 + 1, a piece that starts on p1; an empty tile inside the group; the rare
    records.  The region ends inside its last tile, where a read's second piece starts behind the region's last position: live_clipped != live"""
    q = 20
    T = 192; end = T + TILE * (ntiles - 1) + 30
    ref = ref_of(end + 1500); R = Reads(ref)
    R.add(T, [(0, 8), (2, 4), (0, 8)]); R.add(T + 3, [(0, 8), (1, 2), (0, 8)])
    R.add(T + 2 * TILE + 40, [(0, 10), (2, 5), (0, 150), (2, 3), (0, 10)])           # enters at the third tile; its 150-base piece is live in tiles 2 .. 5
    R.add(T + 3 * TILE - 15, [(0, 10), (2, 5), (0, 10)])                             # first piece's extent ends on p0(3), the second starts there (p1 of tile 2)
    R.add(T + 3 * TILE - 14, [(0, 10), (2, 5), (0, 10)])                             # ... on p0(3) + 1
    rare_reads(R, T + 3 * TILE + 10, q)
    # (tile 6 stays empty; tile 7 closes the group)
    for t in range(7, ntiles - 1):
        for j in range(3):
            R.add(T + TILE * t + 9 * j, [(0, 5), (2, 2), (0, 5), (1, 1), (0, 5)], flag=(0, 16)[j & 1], edit=mismatches([1], THIRD) if j == 2 else mismatches([1], OTHER) if j else None)
    R.add(end - 12, [(0, 10), (2, 5), (0, 10)])                                      # its second piece starts on end + 3: behind the region, inside its last tile
    R.add(end - 30, [(0, 25)])

    def cells(ws):
        w = ws[0]
        assert (w["pos0"], w["ntiles"], w["P"] % TILE) == (T, ntiles, 30) and (ntiles % CR_GROUP, ntiles % (4 * CR_GROUP)) in ((0, 8), (7, 31), (1, 1))
        assert w["live_clipped"] == w["live"] - 1                     # the one piece behind the region's last position
        assert has_rare_reads(case.arrs, q)
        key, reach = pieces_of(case.arrs)
        assert {T + 3 * TILE, T + 3 * TILE + 1} <= set(reach.tolist())
        by_tile = {x["pos0"]: x for x in ws[1:]}
        assert by_tile[T + 6 * TILE]["ranged"] == 0 and by_tile[T + 5 * TILE]["live"] > 0 and by_tile[T + 7 * TILE]["live"] > 0      # an empty range inside the group
        assert by_tile[T + 2 * TILE]["live_max_read"] == 2            # the read that enters at the third tile: two of its five pieces
        assert all(by_tile[T + t * TILE]["live"] >= 1 for t in (2, 3, 4, 5))
    case = Case(ref, R.arrays(), (T + 1, end), cells, opts=dict(min_mapq=q, min_bq=5))
    return case


C4_LIVE = {63: (20, 40, 3), 64: (20, 40, 4), 65: (25, 40, 0), 128: (30, 54, 44), 129: (30, 54, 45)}


def case_c4():
    """-i; five tiles, each in a group of its own, with 63, 64, 65, 128 and 129 live pieces: `before` one-piece reads, then one read of
    1M1I x 64 of which 40 or 54 pieces lie in the tile — its lane's run straddles the end of a copy round where the tile has more than 64 —,
    then one-piece reads; the rare records among them"""
    q = 20
    ref = ref_of(512 * 7); R = Reads(ref)
    for g, (total, (before, big, after)) in enumerate(sorted(C4_LIVE.items())):
        p0 = 128 + 512 * (g + 1)                                      # (pos0 = 128: the filler read below)
        for j in range(before):
            plain(R, p0 + (j * (TILE - big)) // before, j, L=4)
        R.add(p0 + TILE - big, [(0, 1), (1, 1)] * 63 + [(0, 1)], flag=(0, 16)[g & 1])
        j = 0
        if after >= 20:
            j = rare_reads(R, p0 + TILE - big, q)
        for j in range(j, after):
            plain(R, p0 + TILE - big + j % 8, j, L=4)
    R.add(128, [(0, 30)])

    def cells(ws):
        w = ws[0]
        assert w["pos0"] == 128 and w["live_max_read"] == 54 and w["live_max"] == 129 and has_rare_reads(case.arrs, q)
        by_tile = {x["pos0"]: x for x in ws[1:]}
        for g, (total, (before, big, after)) in enumerate(sorted(C4_LIVE.items())):
            x = by_tile[128 + 512 * (g + 1)]
            assert (x["live_max"], x["live_max_read"]) == (total, big) and (total <= 64 or before < 64 < before + big)
    case = Case(ref, R.arrays(), (1, 512 * 6 + 400), cells, opts=dict(min_mapq=q, min_bq=5, insertion_centric=True))
    return case


def case_c6(n_libs):
    """announced windows over reads of five pieces: on lane 0, on lane 63, on both lanes of one tile, inside a tile whose reads end before
    the window (its range is empty after trimming), on a tile between unannounced ones"""
    T = 256
    ref = ref_of(T + TILE * 20 + 500); R = Reads(ref)
    for j in range(110):
        p = T + 9 * j
        if T + 10 * TILE <= p < T + 11 * TILE + 30:                  # tile 10 holds reads on its first lanes only, tile 11 none
            continue
        R.add(p, [(0, 7), (2, 3), (0, 7), (1, 2), (0, 7), (2, 4), (0, 7), (3, 9), (0, 7)], lib=j % n_libs, flag=(0, 16)[j & 1],
              edit=mismatches([2], THIRD) if j % 7 == 3 else mismatches([2], OTHER) if j % 3 == 1 else None)
    for l in range(n_libs):
        R.add(T + 10 * TILE, [(0, 6), (2, 2), (0, 6)], lib=l); R.add(T + 10 * TILE + 2, [(0, 6), (2, 2), (0, 6)], lib=l)
    w = lambda t, a, b=None: (T + TILE * t + a + 1, T + TILE * t + (a if b is None else b) + 1)      # a window over lanes a .. b of tile t
    windows = [w(1, 0), w(2, 63), w(4, 0), w(4, 63), w(5, 10, 11), w(6, 30), w(7, 62, 63 + 2), w(10, 58, 59), w(13, 0, 63), w(14, 5)]

    def cells(ws):
        x = ws[0]
        assert x["windows"] and x["Lp"] == n_libs and x["pos0"] == T
        by_tile = {y["pos0"]: y for y in ws[1:]}
        assert by_tile[T + 10 * TILE]["ranged"] == 0 and by_tile[T + 10 * TILE]["windows"]      # empty after trimming ...
        assert by_tile[T + 3 * TILE]["ranged"] > 0 and not by_tile[T + 3 * TILE]["windows"]      # (a tile nobody announced keeps its whole range)
        assert all(y["range_starts_behind_next"] == 0 for y in ws)    # (cannot be otherwise: see the file's docstring)
    kw = dict(opts=dict(per_lib=True, min_bq=5), names=NAMES3[:n_libs]) if n_libs > 1 else dict(opts=dict(min_bq=5))
    case = Case(ref, R.arrays(), (T + 1, T + TILE * 16 + 10), cells, windows=windows, **kw)
    return case


C7_RANGES = [0, 1, 63, 64, 65, 129]


def case_c7(n_libs):
    """tile 2 k + 1 holds C7_RANGES[k] reads of one piece of one library (the other libraries: one read each), tile 2 k is empty: tile
    ranges of 0, 1, 63, 64, 65 and 129 pieces for k_compact_tiles' walk in rounds of 64; ntiles % 4 = 1 with one library (under knob 2),
    3 with three"""
    ntiles = 13 if n_libs == 1 else 15
    T = 320
    ref = ref_of(T + TILE * ntiles + 500); R = Reads(ref)
    plain(R, T, 0, L=10, lib=0)
    for k, n in enumerate(C7_RANGES):
        for j in range(n):
            R.add(T + TILE * (2 * k + 1) + (40 * j) // n, [(0, 8)], lib=k % n_libs, flag=(0, 16)[j & 1], edit=mismatches([1], OTHER) if j % 4 == 1 else None)
        for l in range(n_libs):
            if l != k % n_libs and n:
                R.add(T + TILE * (2 * k + 1) + 45, [(0, 8)], lib=l)
    plain(R, T + TILE * (ntiles - 1) + 20, 1, L=30, lib=n_libs - 1)

    def cells(ws):
        w = ws[0]
        assert (w["pos0"], w["ntiles"], w["Lp"], w["ntiles"] % 4) == (T, ntiles, n_libs, 1 if n_libs == 1 else 3)
        by_tile = {x["pos0"]: x for x in ws[1:]}
        assert [by_tile[T + TILE * (2 * k + 1)]["range_max"] for k in range(len(C7_RANGES))] == C7_RANGES
        assert [by_tile[T + TILE * 2 * k]["ranged"] for k in range(1, len(C7_RANGES))] == [0] * (len(C7_RANGES) - 1)
    kw = dict(opts=dict(per_lib=True), names=NAMES3) if n_libs > 1 else {}
    return Case(ref, R.arrays(), (T + 1, T + TILE * ntiles - 14), cells, **kw)


def case_c8():
    """the life of an engine: the C3 batch with two passes per region (the second reuses compact_sized), one engine running a small region,
    a larger one, a smaller one, then the whole and every tile"""
    case = case_c3(31)
    T = 192
    case.passes = 2
    case.extra_regions = [(T + 3 * TILE + 1, T + 4 * TILE), (T + 1, T + 20 * TILE), (T + 8 * TILE + 1, T + 9 * TILE)]
    return case


def case_c9(extra):
    """4 reads of 12 pieces — exactly 12 n_reads pieces: the product does not compact —, or one of them of 13: it does"""
    ref = ref_of(2048); R = Reads(ref)
    for j in range(4):
        R.add(200 + 40 * j, [(0, 5), (2, 1)] * (11 + (extra and j == 2)) + [(0, 5)], flag=(0, 16)[j & 1], edit=mismatches([7], OTHER) if j else None)

    def cells(ws):
        w = ws[0]
        assert w["n_reads"] == 4 and w["n_pieces"] == PRODUCT_RULE * 4 + extra and w["ranged"] > w["live"] > 0
        assert expected(w, "product") == ((w["ranged"], w["live_clipped"]) if extra else (0, 0))
    return Case(ref, R.arrays(), (1, 1000), cells)


# ------------------------------------------------------------------------------------------------ the cases and the routes

BUILDERS = {}
BUILDERS.update({"T1-pieces_%d" % n: (lambda n: lambda: case_t1(n))(n) for n in T1_COUNTS})
BUILDERS.update({"T2-carried_from_piece_%d" % k: (lambda k: lambda: case_t2(k))(k) for k in T2_FIRST})
BUILDERS.update({"T3-pos0_mod64_%d" % o: (lambda o: lambda: case_t3(o))(o) for o in (0, 1, 63)})
BUILDERS["T4-gaps"] = case_t4
BUILDERS.update({"T5-libraries_%d_%d_%d" % s: (lambda s: lambda: case_t5(s))(s) for s in T5_SIZES})
BUILDERS.update({"T6-aggregate_%d" % (f // TR_CHUNK): (lambda f: lambda: case_t6(f))(f) for f in (TR_CHUNK * 1024 - 1, TR_CHUNK * 1024)})
BUILDERS.update({"S-libs%d_tiles%d" % s: (lambda s: lambda: case_s(*s))(s) for s in S_SHAPES})
BUILDERS.update({"C1-reads_%d" % n: (lambda n: lambda: case_c1(n))(n) for n in C1_READS})
BUILDERS.update({"C2-reads_in_group_%d" % n: (lambda n: lambda: case_c2(n))(n) for n in C2_READS})
BUILDERS.update({"C3-tiles_%d" % n: (lambda n: lambda: case_c3(n))(n) for n in C3_TILES})
BUILDERS["C4-copy_rounds"] = case_c4
BUILDERS.update({"C6-windows_libs%d" % n: (lambda n: lambda: case_c6(n))(n) for n in (1, 2)})
BUILDERS.update({"C7-range_walk_libs%d" % n: (lambda n: lambda: case_c7(n))(n) for n in (1, 3)})
BUILDERS["C8-engine_life"] = case_c8
BUILDERS.update({"C9-product_rule_12n+%d" % x: (lambda x: lambda: case_c9(x))(x) for x in (0, 1)})
_cases = {}


def witness_of(sim_lib):
    f = sim_lib.lib.brc_sim_witness; f.restype = ctypes.c_char_p
    return json.loads(f(0).decode())


def expected(w, knob):
    """piece_steps() of a region whose witness is w: BRC_COMPACT_TILES = 0 / 1 / 2, or "product" (its own rule)"""
    on = w["n_reads"] > 0 and w["n_pieces"] > PRODUCT_RULE * w["n_reads"] if knob == "product" else knob != 0 and w["n_pieces"] > 0
    if not on:
        return (0, 0)
    return (w["ranged"], w["live_clipped"] if w["Lp"] == 1 and knob != 2 else w["live"])


def windows_of(case, region):
    """the announced windows of a region: the case's, cut to it"""
    if not case.windows:
        return []
    beg0, end = region
    return [(max(b, beg0), min(e, end)) for b, e in case.windows if max(b, beg0) <= min(e, end) and max(b, beg0) - 1 < min(e, end)]


def run(lib, case, regions, device_text=False):
    """one engine over all regions, the WHOLE batch pushed for each; per region (text, result, piece_steps)"""
    hip = lib.kind().startswith("hip")
    eng = capi.Engine(lib, lib_names=case.names, device_text="chrS" if device_text else None, **case.opts)
    out = []
    try:
        for region in regions:
            eng.begin_region(0, region[0], region[1], case.ref); eng.push_reads(case.arrs)
            wins = windows_of(case, region)
            if wins:
                eng.region_windows(np.array([w[0] for w in wins], np.int32), np.array([w[1] for w in wins], np.int32))
            if hip and case.passes > 1:
                eng.upload(); eng.compute_n(case.passes); res = eng.fetch_result()
            else:
                res = eng.end_region()
            steps = eng.piece_steps() if hip else None
            text = b"".join(eng.format_window("chrS", b, e, 0) for b, e in wins) if wins else eng.format_region("chrS")
            eng.clear_indel_queue()
            out.append((text, res, steps))
    finally:
        eng.close()
    return out


def oracle_of(oracle_lib, case):
    """the reference of every region: the oracle over the whole batch; of a region with announced windows, every window as a region of its
    own over the reads that overlap it (its text) and the whole region (its planes)"""
    plain_case = Case(case.ref, case.arrs, case.region, None, opts=case.opts, names=case.names)
    want = run(oracle_lib, plain_case, case.regions)
    for i, region in enumerate(case.regions):
        wins = windows_of(case, region)
        if wins:
            text = b""
            for b, e in wins:
                t, _ = parity.run_engine(oracle_lib, case.arrs, [(b, e)], ref=case.ref, lib_names=case.names, **case.opts)
                text += t
            want[i] = (text, want[i][1], wins)
    return want


def compare(got, case, what):
    assert len(got) == len(case.want)
    for i, ((text, res, _), (wtext, wres, wins)) in enumerate(zip(got, case.want)):
        at = "%s region %d %r" % (what, i, case.regions[i])
        if wins:
            assert (res.pos0, res.n_pos, res.n_lib) == (wres.pos0, wres.n_pos, wres.n_lib), at
            asked = np.zeros(res.n_pos, bool)
            for b, e in wins:
                asked[max(b - 1 - res.pos0, 0):max(e - res.pos0, 0)] = True
            for g, w in ((res.ncol, wres.ncol), (res.depth, wres.depth), (res.istat, wres.istat), (res.fstat.view(np.uint32), wres.fstat.view(np.uint32))):
                np.testing.assert_array_equal(g[..., asked], w[..., asked], err_msg=at)
        else:
            parity.assert_results_equal(res, wres, at)
            if case.check_warn:
                assert res.warn[:3] == wres.warn[:3], at
        assert text == wtext, at + ": text differs"
    assert got[0][0].count(b"\n") >= case.min_lines


def prepared(name, sim_lib, oracle_lib):
    """the case, built once: its regions (the whole one; every single-tile one), the batch through the simulator with the witness on,
    [sim] == oracle, and the cells it was built to hit asserted — before anything goes to a device route"""
    if name in _cases:
        return _cases[name]
    case = BUILDERS[name]()
    assert (np.diff(case.arrs["pos"].astype(np.int64)) >= 0).all()
    sim_lib.lib.brc_sim_witness.restype = ctypes.c_char_p
    sim_lib.lib.brc_sim_witness(1)
    first = run(sim_lib, case, [case.region])
    (w,) = witness_of(sim_lib)
    singles = []
    if case.singles:
        for t in range(w["ntiles"]):
            singles.append((w["pos0"] + TILE * t + 1, min(w["pos0"] + TILE * (t + 1), w["pos0"] + w["P"])))
    case.regions = case.extra_regions + [case.region] + singles
    n_extra = len(case.extra_regions)
    sim_lib.lib.brc_sim_witness(1)
    got = run(sim_lib, case, case.regions)
    ws = witness_of(sim_lib)
    assert len(ws) == len(case.regions) and ws[n_extra] == w and got[n_extra][0] == first[0][0]
    for x, (beg0, end) in zip(ws[n_extra + 1:], singles):
        assert (x["pos0"], x["P"], x["ntiles"]) == (beg0 - 1, end - beg0 + 1, 1)        # a single tile, on the whole region's grid
    case.ws = ws
    case.want = oracle_of(oracle_lib, case)
    compare(got, case, "[sim]")
    case.cells(ws[n_extra:])
    assert all(x["range_starts_behind_next"] == 0 for x in ws)
    print("census %-28s %7d reads %8d pieces %5d tiles %d libraries: ranged %d, live %d (clipped %d), largest range %d, most live %d (of one read %d), reads per group %d; %d regions" % (
        name, w["n_reads"], w["n_pieces"], w["ntiles"], w["Lp"], w["ranged"], w["live"], w["live_clipped"], w["range_max"], w["live_max"], w["live_max_read"], w["reads_max"], len(case.regions)))
    _cases[name] = case
    return case


def device_route(lib, case, knob, what, device_text=True):
    got = run(lib, case, case.regions)
    compare(got, case, what)
    for i, ((_, _, steps), w) in enumerate(zip(got, case.ws)):
        assert steps == expected(w, knob), "%s region %d %r: piece_steps %r, the witness says %r" % (what, i, case.regions[i], steps, expected(w, knob))
    if device_text and not case.windows:
        text = run(lib, case, case.regions[:len(case.extra_regions) + 1], device_text=True)
        assert [t[0] for t in text] == [t[0] for t in case.want[:len(text)]], what + ": device text differs"


@pytest.fixture(scope="module")
def knobs_hip_lib():
    """libbrc_hip_testknobs.so as build() left it (a missing library is an error)"""
    path = os.path.join(ROOT, "bam_readcount_amd", "csrc", "libbrc_hip_testknobs.so")
    if not os.path.exists(path):
        raise RuntimeError("libbrc_hip_testknobs.so is not built (make -C bam_readcount_amd/csrc)")
    return capi.Library(path)


def test_library_boundaries_of_the_T5_batches():
    t5_census()


@pytest.mark.parametrize("name", list(BUILDERS))
def test_sim_equals_oracle_and_the_witness_holds_the_cells(sim_lib, oracle_lib, name):
    case = prepared(name, sim_lib, oracle_lib)
    assert len(case.ws) == len(case.regions) == len(case.want)


# (the checked route stands first: in file order, and in the GPU job, the other libraries run a batch only after the bounds-checked build did)
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BUILDERS))
def test_checked_build_reports_no_violation(checked_lib, sim_lib, oracle_lib, monkeypatch, name):
    case = prepared(name, sim_lib, oracle_lib)
    for knob in (1, 2):
        monkeypatch.setenv("BRC_COMPACT_TILES", str(knob))
        device_route(checked_lib, case, knob, "checked build, BRC_COMPACT_TILES=%d" % knob, device_text=False)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BUILDERS))
def test_knobs_library_compacted_read_wise_by_range_walk_and_not(knobs_hip_lib, sim_lib, oracle_lib, monkeypatch, name):
    case = prepared(name, sim_lib, oracle_lib)
    for knob in (1, 2, 0) if case.knob0 else (1, 2):
        monkeypatch.setenv("BRC_COMPACT_TILES", str(knob))
        device_route(knobs_hip_lib, case, knob, "test-knobs library, BRC_COMPACT_TILES=%d" % knob)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BUILDERS))
def test_product_library_by_its_own_rule(hip_lib, sim_lib, oracle_lib, name):
    case = prepared(name, sim_lib, oracle_lib)
    device_route(hip_lib, case, "product", "product library")
