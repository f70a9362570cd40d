"""The side path that carries a region's rare events from k_pileup2 to the results — the 1024 third-allele sub-lists and their compaction
(k_pileup2's shard rule, k_xev_compact, k_xev_scatter, finish_passes' grow-and-recompute), the fold (k_xev_fold: fold_xev_bucket), the
indel reduce (k_indel_scatter, k_indel_reduce: sort_indel_events, reduce_indel_bucket, indel_bucket, indel_bucket_shift; k_unavail) and the
counters (k_finalize / k_finalize_sum) — at the boundaries of its own data structures, on batches written down by hand (constructed.Reads;
no make_batch, no random batch).  Families: A sub-lists and compaction, B the fold, C the indel reduce, D the position counter.

Routes: (1) CPU: oracle == [sim], the cells a batch was built for asserted from the simulator's WITNESS (tests/sim/brc_sim.cpp) and from
the oracle's own results; (2) the bounds-checked build; (3) the product library, or — a batch that names a test knob — the test-knobs
library; both also through the device's text.  Every comparison is an equality of bits and bytes (planes, indel lists, unavail, warning
counts, text), and for EVERY region of the file Engine.counts()[1] == the number of lines the oracle prints for it.

What cannot be seen from outside is asserted through brc_region_passes (Engine.passes()): how often the last compute ran the pipeline and
the capacity a sub-list has now.  The witness's "xev_sublist_max" — the fullest of the 1024 sub-lists the device would fill, a RESTATEMENT
of the shard rule in the simulator — decides what the device must report: above the capacity 2 passes and a capacity of twice that load,
otherwise 1 pass and the capacity unchanged, carried along from region to region of an engine.  If k_pileup2's rule and the restatement
drift apart, one of the two directions fails.  The simulator is held to the same statement over its one list ("n_xev" against its size).

The hard condition of this file, asserted for every batch before any device route runs it: at most XEV_BUCKET third-allele events per
(tile, library) bucket ("xev_bucket_max": fold_xev_bucket is quadratic on one lane)."""
import contextlib
import ctypes
import json
import os

import numpy as np
import pytest

import parity
from bam_readcount_amd import capi
from conftest import ROOT
from constructed import OTHER, THIRD, Reads, checked_lib, mismatches, ref_of, run_steps  # noqa: F401  (checked_lib: fixture)

XEV_BUCKET = 512                 # the most third-allele events of one (tile, library) bucket in this file
XEV_CAP0 = 256                   # brc_engine.hip: the product's sub-list capacity for a region of fewer than 2 M pieces
SIM_CAP0 = 1024                  # tests/sim/brc_sim.cpp: the simulator's one list
FOURTH = np.full(16, 4, np.uint8); FOURTH[[1, 2, 4, 8]] = [8, 1, 2, 4]       # the base that is none of reference, OTHER, THIRD
A_, C_, G_, T_, N_, EQ_ = 1, 2, 4, 8, 15, 0                                    # 4-bit base codes
I_N = 0
BUCKETS = "=ACGTN"


class Case:
    def __init__(self, ref, steps, kw=None, env=None, n_xev=None, sub_max=None, cells=None, windows=None, check_warn=True, lines=None, hip_passes=None):
        self.ref, self.steps, self.kw, self.env = ref, steps, kw or {}, env or {}
        self.n_xev, self.sub_max, self.cells, self.windows, self.check_warn, self.lines, self.hip_passes = n_xev, sub_max, cells, windows, check_warn, lines, hip_passes


def libs(n):
    return dict(per_lib=True, lib_names=["lib%c" % (65 + i) for i in range(n)]) if n > 1 else {}


def n_ref(n):
    return np.full(n, ord("N"), np.uint8)


def all_bases(b):
    def edit(seq, qual, aq, ar, code):
        seq[aq] = b
    return edit


def lut_bases(lut, q=None):
    def edit(seq, qual, aq, ar, code):
        seq[aq] = lut[code[ar]]
        if q is not None:
            qual[aq] = q
    return edit


def pinned(ref, region, iupac=False):
    """Reads over `ref` for `region` = (beg0, end), with a one-base read on the lead position beg0 - 1 and one on end - 1: the planes of a
    region reach from its first to its last read, so these two pin plane index 0 to beg0 - 1 and P to end - beg0 + 1 — the tile, bucket and
    group-of-four arithmetic of every case below counts from there"""
    R = Reads(ref, iupac=iupac)
    R.add(region[0] - 1, [(0, 1)]); R.add(region[1] - 1, [(0, 1)])
    return R


def fill(R, pos, count, lib=0, base=C_, salt=0):
    """Cheap events: `count` third-allele events of library `lib` on the positions [pos, pos + 64) of a reference of N.  A read of 64 A comes
    first (slot 0 is the reference's N, which no read carries; slot 1 the first other base, A), then reads of `base`, 64 events each and
    one for the rest; mapping quality, strand, clip, NM and SM step with the read's number."""
    R.add(pos, [(0, 64)], lib=lib)
    j = 0
    while count > 0:
        n = min(count, 64); clip = (j + salt) % 3
        R.add(pos, ([(4, clip)] if clip else []) + [(0, n)], lib=lib, flag=(0, 16)[(j + salt) & 1], mapq=20 + (7 * j + salt) % 41, nm=(j + salt) % 5, sm=(3 * j + salt) % 60,
              edit=all_bases(base))
        count -= n; j += 1


def fill_at(R, pos, n, base, lib=0):
    """n third-allele events on ONE position of a reference of N (a one-base read of A first)"""
    R.add(pos, [(0, 1)], lib=lib)
    for j in range(n):
        R.add(pos, [(0, 1)], lib=lib, flag=(0, 16)[j & 1], mapq=30 + j, edit=all_bases(base))


# ------------------------------------------------------------------------------------------------ A. sub-lists and compaction

def case_a1(total, spread):
    """One workgroup's four tiles (a region of 256 planes) carry `total` events: spread over the four tiles, whose four waves append to
    sub-list 0 concurrently, or all in tile 1.  255 | 256 | 257 stand around the product's capacity, 512 is twice it."""
    R = pinned(n_ref(320), (1, 256), True)
    per = [total // 4 + (1 if t < total % 4 else 0) for t in range(4)] if spread else [0, total, 0, 0]
    for t, n in enumerate(per):
        if n:
            fill(R, 64 * t, n, salt=t)

    def cells(ws, want, res):
        assert (ws[0]["ntiles"], ws[0]["xev_bucket_max"]) == (4, max(per))
    return Case(R.ref, [(R.arrays(), (1, 256))], n_xev=[total], sub_max=[total], cells=cells, hip_passes=[{255: (1, 256), 256: (1, 256), 257: (2, 514), 512: (2, 1024)}[total]])


def case_a2():
    """One engine, four regions of four tiles each: 600 events in one sub-list (the product's lists grow from 256 to 1200), 10 events,
    400 (they fit the grown lists, not the original ones: one pass), 1320 (they grow again, to 2640; the simulator's one list of 1024
    grows here)."""
    R = pinned(n_ref(1900), (1, 1792), True)
    for t in range(4):
        fill(R, 64 * t, 150, salt=t)
        fill(R, 64 * (16 + t), 100, salt=t, base=G_)
        fill(R, 64 * (24 + t), 330, salt=t, base=T_)
    fill(R, 64 * 8, 10)
    arrs = R.arrays()
    steps = [(arrs, (1, 256)), (arrs, (513, 768)), (arrs, (1025, 1280)), (arrs, (1537, 1792))]
    return Case(R.ref, steps, n_xev=[600, 10, 400, 1320], sub_max=[600, 10, 400, 1320], hip_passes=[(2, 1200), (1, 1200), (1, 1200), (2, 2640)])


def with_every_library(R, n):
    for l in range(n):
        R.add(10 + 3 * l, [(0, 30)], lib=l)


def case_a3_five(env=None):
    """Five libraries, 1280 planes: library 4's workgroup 0 (tiles 0 - 3) and library 0's workgroup 4 (tiles 16 - 19) append to sub-list
    (0 + 4 * 257) & 1023 = 4 = (4 + 0 * 257) & 1023.  200 events each: either bucket fits the capacity of 256, both together do not."""
    R = pinned(n_ref(1400), (1, 1280), True)
    with_every_library(R, 5)
    fill(R, 64 * 1, 200, lib=4); fill(R, 64 * 17, 200, lib=0, base=G_, salt=1)

    def cells(ws, want, res):
        assert (ws[0]["Lp"], ws[0]["ntiles"], ws[0]["xev_bucket_max"]) == (5, 20, 200)
    return Case(R.ref, [(R.arrays(), (1, 1280))], kw=libs(5), env=env, n_xev=[400], sub_max=[400], cells=cells)


def case_a3_two():
    """Two libraries, a region that reaches tile 1028: library 1's workgroup 0 and library 0's workgroup 257 share sub-list 257"""
    R = pinned(n_ref(65856 + 64), (1, 65856), True)
    with_every_library(R, 2)
    fill(R, 64 * 2, 200, lib=1); fill(R, 64 * 1028, 200, lib=0, base=T_, salt=2)
    return Case(R.ref, [(R.arrays(), (1, 65856))], kw=libs(2), n_xev=[400], sub_max=[400])


def case_a3_wrap():
    """One library, 262 400 planes, two clusters of reads: workgroup 1024 (tiles 4096 - 4099) wraps to sub-list 0, that of tiles 0 - 3"""
    R = pinned(n_ref(262400 + 64), (1, 262400), True)
    for t in range(4):
        fill(R, 64 * t, 50, salt=t); fill(R, 64 * (4096 + t), 50, salt=t + 1, base=G_)

    def cells(ws, want, res):
        assert ws[0]["ntiles"] == 4100 and ws[0]["xev_bucket_max"] == 50
    return Case(R.ref, [(R.arrays(), (1, 262400))], n_xev=[400], sub_max=[400], cells=cells)


def case_a4_last_sublist():
    """events only in sub-list 1023, whose block of k_xev_compact leaves the total: library 3, workgroup 252 (252 + 3 * 257 = 1023)"""
    R = pinned(n_ref(64768 + 64), (1, 64768), True)
    with_every_library(R, 4)
    for t in range(4):
        fill(R, 64 * (1008 + t), 40, lib=3, salt=t)
    return Case(R.ref, [(R.arrays(), (1, 64768))], kw=libs(4), n_xev=[160], sub_max=[160])


def case_a4_255_256():
    """events in sub-lists 255 and 256 only: the last cursor a thread of k_xev_compact reads in its first round, the first of its second"""
    R = pinned(n_ref(65792 + 64), (1, 65792), True)
    fill(R, 64 * 1023, 30); fill(R, 64 * 1024, 35, base=T_, salt=1)
    return Case(R.ref, [(R.arrays(), (1, 65792))], n_xev=[65], sub_max=[35])


def case_a4_ends():
    """165 planes: events on lanes 0 and 63 of tile 1 and on plane index P - 1, lane 36 of the partial last tile"""
    R = pinned(n_ref(200), (1, 165), True)
    fill_at(R, 64, 3, C_); fill_at(R, 127, 3, G_); fill_at(R, 164, 3, N_)

    def cells(ws, want, res):
        assert ws[0]["P"] == 165 and [int(t.split(b"\t")[1]) for t in want[0].split(b"\n") if t] == [65, 128, 165]
    return Case(R.ref, [(R.arrays(), (1, 165))], n_xev=[9], sub_max=[9], cells=cells)


def case_a4_none():
    """no event at all: two bases per position at the most"""
    ref = ref_of(300); R = pinned(ref, (1, 256))
    for s in range(0, 230, 10):
        R.add(s, [(0, 40)], flag=(0, 16)[(s // 10) & 1], edit=mismatches([3, 17], OTHER) if s % 20 else None)
    return Case(ref, [(R.arrays(), (1, 256))], n_xev=[0], sub_max=[0])


A5_TILES = (3, 17, 18, 39)


def case_a5_windows():
    """brc_region_windows over 40 tiles, four of them listed: slots 0 - 3 of the tile list are ONE workgroup, so that all four append to
    sub-list 0 (by tile they would be workgroups 0, 4, 4 and 9) — 100 events each; events in a tile nobody listed.  The witness's
    sub-list load does not describe this launch: bits only."""
    R = pinned(n_ref(2560 + 64), (1, 2560), True)
    for t in A5_TILES + (10,):
        fill(R, 64 * t, 100, salt=t)
    return Case(R.ref, [(R.arrays(), (1, 2560))], windows=[(64 * t + 5, 64 * t + 50) for t in A5_TILES])


# ------------------------------------------------------------------------------------------------ B. the fold

def one_base(R, pos, b=None, lut=None, **kw):
    R.add(pos, [(0, 1)], edit=(lambda seq, qual, aq, ar, code: seq.__setitem__(0, lut[code[ar[0]]] if lut is not None else b)), **kw)


def case_b1():
    """One bucket (tile 1).  Read j (j <= 31) starts at lane j and carries its third allele on lane 63 - j: the events arrive in the reverse
    of the order the fold sorts them into.  Lanes 5, 20 and 63 add events of three and four buckets, N and '=' read bases among them."""
    ref = ref_of(256); R = Reads(ref); T = 64
    R.add(T, [(0, 64)]); R.add(T, [(0, 64)], edit=mismatches(range(64), OTHER), flag=16)
    for j in range(32):
        R.add(T + j, [(0, 64 - j)], edit=mismatches([63 - 2 * j], THIRD, q=3 + j), mapq=5 + j, flag=(0, 16)[j & 1], nm=1 + j % 4)
    for lane, bases in ((5, (FOURTH, N_, EQ_)), (20, (THIRD, FOURTH, N_, EQ_, THIRD)), (63, (FOURTH, N_, EQ_))):
        for j, b in enumerate(bases):
            one_base(R, T + lane, **(dict(lut=b) if isinstance(b, np.ndarray) else dict(b=b)), mapq=40 + j, flag=(0, 16)[j & 1])

    def cells(ws, want, res):
        assert ws[0]["xev_bucket_max"] == ws[0]["n_xev"] == 43
    return Case(ref, [(R.arrays(), (1, 128))], n_xev=[43], sub_max=[43], cells=cells)


B2_FLOOR = 20


def case_b2(reverse=False):
    """Order matters.  Three groups of six reads that share a start (and so can be swapped without leaving the sorted order); every base of
    theirs is a third allele, and the reads differ in mapping quality, base quality, clips, length (read position) and NM.  reverse: every
    group of equal-start reads in the opposite order."""
    ref = ref_of(256); R = Reads(ref); T = 64
    R.add(T, [(0, 64)]); R.add(T, [(0, 64)], edit=mismatches(range(64), OTHER), flag=16)
    for g in range(3):
        group = []
        for r in range(6):
            n = 18 + 2 * r; lc, rc = r % 3, (2 * r + g) % 5

            def edit(seq, qual, aq, ar, code, r=r, g=g):
                seq[aq] = THIRD[code[ar]]
                qual[aq] = 5 + (11 * r + 3 * np.arange(len(aq)) + g) % 50
            group.append(dict(pos=T + 2 + 14 * g, ops=([(4, lc)] if lc else []) + [(0, n)] + ([(4, rc)] if rc else []), edit=edit, mapq=10 + 9 * r + g, nm=1 + r, sm=7 * r + g,
                              flag=(0, 16)[r & 1]))
        for kw in (group[::-1] if reverse else group):
            R.add(kw.pop("pos"), kw.pop("ops"), **kw)
    return Case(ref, [(R.arrays(), (1, 128))])


def third_cells_that_differ(ref, ra, rb):
    """(position, bucket) cells of the third-allele buckets whose fp32 sums differ between two results"""
    code = {65: 1, 67: 2, 71: 4, 84: 8}
    n = 0
    for k in range(ra.n_pos):
        c = code[int(ref[ra.pos0 + k])]
        for b in range(6):
            if b in (BUCKETS.index("ACGT"[(1, 2, 4, 8).index(c)]), BUCKETS.index("ACGT"[(1, 2, 4, 8).index(int(OTHER[c]))])):
                continue
            n += not np.array_equal(ra.fstat[0, b, :, k].view(np.uint32), rb.fstat[0, b, :, k].view(np.uint32))
    return n


def case_b3():
    """Records.  Tile 1: eight events on eight lanes, every event a record of its own.  Tile 2: 40 events of one base on one lane, ONE
    record and 39 slots of the run marked unused, which the host's fetch and the device's text must skip.  Tile 3: a reference N and a
    reference '=' under read bases N and '=' — records of a bucket that slot 0 names (the text witness's `table_named`)."""
    ref = ref_of(320).copy(); ref[192 + 40] = ord("N"); ref[192 + 41] = ord("=")
    R = Reads(ref, iupac=True)
    for T in (64, 128, 192):
        R.add(T, [(0, 64)]); R.add(T, [(0, 64)], edit=mismatches(range(64), OTHER), flag=16)
    for j in range(8):
        one_base(R, 64 + 1 + 8 * j, lut=THIRD, mapq=20 + j, flag=(0, 16)[j & 1])
    for j in range(40):
        one_base(R, 128 + 18, lut=THIRD, mapq=3 + j, flag=(0, 16)[j % 3 == 0], nm=j % 4)
    for j in range(3):
        one_base(R, 192 + 40, b=N_, mapq=30 + j); one_base(R, 192 + 41, b=EQ_, mapq=33 + j); one_base(R, 192 + 40, b=G_, mapq=36 + j)

    def cells(ws, want, res):
        assert ws[0]["n_xev"] == 8 + 40 + 9 and ws[0]["xev_bucket_max"] == 40
    return Case(ref, [(R.arrays(), (1, 256))], n_xev=[57], sub_max=[57], cells=cells)


# ------------------------------------------------------------------------------------------------ C. the indel reduce

C1_SIZES = (1, 2, 47, 48, 49, 50, 200)


def c1_anchor(idx):
    return 512 * idx + 256


def case_c1(n_libs, env=None):
    """Seven indel buckets of exactly 1, 2, 47, 48, 49, 50 and 200 events (sort_indel_events changes algorithm between 48 and 49), all of
    the LAST library, on the four positions G .. G + 3 of a 64-aligned G — one bucket at 4, 16 and 64 positions per bucket.  Read i starts
    at its cluster's S + i and has its indel behind position G + 3 - i % 4: the reads arrive sorted by start, their keys fall while
    the read index rises.  The other libraries have two events each on G + 1 (keys of all libraries interleave: key = plane * Lp + library)."""
    ref = ref_of(512 * len(C1_SIZES) + 64); R = pinned(ref, (1, 512 * len(C1_SIZES)))
    last = n_libs - 1
    for idx, n in enumerate(C1_SIZES):
        G = c1_anchor(idx); S = G - n - 8
        for i in range(n):
            a = G + 3 - i % 4
            op = ((1, 2), (2, 1), (2, 3), (1, 1))[(i // 4 + i) % 4]

            def edit(seq, qual, aq, ar, code, i=i, m=a - (S + i) + 1, op=op):
                if op[0] == 1:
                    seq[m:m + op[1]] = [(1, 2, 4, 8)[(i // 8) % 4]] * op[1]
                qual[:] = 10 + (np.arange(len(qual)) * 5 + i) % 45
            R.add(S + i, [(0, a - (S + i) + 1), op, (0, 12)], lib=last, flag=(0, 16)[(i // 2) & 1], mapq=10 + (i * 13) % 50, nm=op[1] + i % 3, sm=(i * 3) % 70, edit=edit)
        for l in range(last):
            for j in range(2):
                R.add(G - 20 - j, [(0, 22 + j), (1, 1 + j), (0, 9)], lib=l, flag=(0, 16)[j])

    def cells(ws, want, res):
        for idx, n in enumerate(C1_SIZES):
            G = c1_anchor(idx)
            got = sum(int(x["i"][I_N]) for x in res[0].indels if G <= x["pos"] < G + 4 and x["lib"] == last)
            assert got == n, (idx, n, got)
            assert len({(x["pos"], x["lib"]) for x in res[0].indels if G <= x["pos"] < G + 4}) == min(n, 4) + last
        if env:
            assert ws[0]["ibucket_shift"] == int(env["BRC_IBUCKET_SHIFT"])
    return Case(ref, [(R.arrays(), (1, 512 * len(C1_SIZES)))], kw=libs(n_libs), env=env, cells=cells)


C2_SHIFT = {"x64": 4, "x64-1": 6, "x2": 2, "x2-1": 4}


def case_c2(n_libs, which):
    """The thresholds of indel_bucket_shift, without a knob: 640 planes, n_indel_ops * 64 == P * Lp (16 positions per bucket) and one
    operator fewer (64); n_indel_ops * 2 == P * Lp (4) and one fewer (16).  One insertion per read."""
    ref = ref_of(720); R = pinned(ref, (1, 640))
    cells_ = 640 * n_libs
    n = (cells_ // 64 if which.startswith("x64") else cells_ // 2) - which.endswith("-1")
    for i in range(n):
        R.add(3 + (i * 7) % 600, [(0, 5), (1, 1), (0, 5)], lib=i % n_libs, flag=(0, 16)[i & 1], mapq=20 + i % 40)

    def cells(ws, want, res):
        assert ws[0]["P"] == 640 and ws[0]["Lp"] == n_libs and ws[0]["ibucket_shift"] == C2_SHIFT[which], (ws[0]["ibucket_shift"], which)
        assert sum(int(x["i"][I_N]) for x in res[0].indels) == n
    return Case(ref, [(R.arrays(), (1, 640))], kw=libs(n_libs), cells=cells)


C3_PLANES = (0, 3, 4, 15, 16, 63, 64, 191, 192, 199)


def case_c3(env=None):
    """Three libraries, 200 planes from position 64 on: an insertion and a deletion of every library behind plane index 0 (the lead
    position beg0 - 1), 3 | 4, 15 | 16, 63 | 64 (both sides of a bucket edge of every size), 191 | 192 (the partial last bucket of 16 and
    of 64 positions) and P - 1; the last library of the last bucket is the cursor n_indel_slots is read from."""
    ref = ref_of(400); R = pinned(ref, (65, 264))
    for k in C3_PLANES:
        p = 64 + k
        for l in range(3):
            R.add(p - 5, [(0, 6), (1, 2), (0, 6)], lib=l, flag=(0, 16)[(k + l) & 1], mapq=20 + k % 30 + l, edit=lambda seq, qual, aq, ar, code, l=l: seq.__setitem__(slice(6, 8), (2, (1, 4, 8)[l])))
            R.add(p - 3, [(0, 4), (2, 2 + l), (0, 6)], lib=l, mapq=25 + l, nm=2 + l)

    def cells(ws, want, res):
        assert (ws[0]["pos0"], ws[0]["P"], ws[0]["Lp"]) == (64, 200, 3)
        assert {(x["pos"] - 64, x["lib"]) for x in res[0].indels} == {(k, l) for k in C3_PLANES for l in range(3)}
        if env:
            assert ws[0]["ibucket_shift"] == int(env["BRC_IBUCKET_SHIFT"])
    return Case(ref, [(R.arrays(), (65, 264))], kw=libs(3), env=env, cells=cells)


def case_c4():
    """Slots that stay unused (min_mapq 10, min_bq 15; the window is [100, 200)): I / D / P operators behind a base before beg0 - 1 or
    at end and later, of a read below the mapping quality, behind a base below the base quality, in secondary / failed / duplicate reads —
    each beside a read whose operators count, a padded insertion among them."""
    ref = ref_of(300); R = pinned(ref, (101, 200))
    ins = [(0, 11), (1, 2), (0, 20)]                       # from 140: behind position 150
    R.add(140, ins); R.add(140, ins, flag=16)
    R.add(90, [(0, 10), (1, 2), (0, 30)])                  # behind 99: before the lead position
    R.add(92, [(0, 9), (1, 2), (0, 30)])                   # behind 100: the lead position itself counts
    R.add(190, [(0, 16), (2, 2), (0, 5)])                  # behind 205: past the end
    R.add(190, [(0, 10), (2, 2), (0, 5)])                  # behind 199: the last position
    R.add(140, ins, mapq=9); R.add(140, ins, mapq=10)
    R.add(140, ins, edit=lambda seq, qual, aq, ar, code: qual.__setitem__(10, 14))
    R.add(140, ins, edit=lambda seq, qual, aq, ar, code: qual.__setitem__(10, 15))
    for f in (0x100, 0x200, 0x400):
        R.add(140, ins, flag=f)
    R.add(141, [(0, 10), (6, 1), (1, 2), (0, 10)])         # P .. I behind 150
    R.add(141, [(0, 10), (6, 1), (0, 10)])                 # a pad that announces nothing
    R.add(120, [(0, 5), (1, 1), (0, 5), (2, 3), (0, 5), (1, 2), (0, 70), (2, 1), (0, 30)])      # four operators, the last behind 207: three count

    def cells(ws, want, res):
        by = {}
        for x in res[0].indels:
            by[x["pos"]] = by.get(x["pos"], 0) + int(x["i"][I_N])
        assert by == {150: 5, 100: 1, 199: 1, 124: 1, 129: 1, 137: 1}, by
    return Case(ref, [(R.arrays(), (101, 200))], kw=dict(min_mapq=10, min_bq=15), cells=cells)


def ins_read(R, pos, bases, quals=None, tail=10, **kw):
    def edit(seq, qual, aq, ar, code):
        seq[10:10 + len(bases)] = bases
        if quals:
            qual[10:10 + len(bases)] = quals
    R.add(pos, [(0, 10), (1, len(bases))] + ([(0, tail)] if tail else []), edit=edit, **kw)


def case_c5():
    """Alleles of one key (position 309), in first-seen order: insertions that differ only in their last base, an inserted N, inserted
    bases of quality 0 and >= 63 (escape bytes: the base comes from the wide stream) that must join the alleles of plain quality, an
    insertion that runs to the read's end, deletions of two lengths; counts on both strands."""
    ref = ref_of(400); R = Reads(ref)
    order = [((A_, C_), None), ((A_, G_), None), ((A_, C_), (0, 70)), ((N_,), None), ((A_, G_), (63, 0)), ((A_, C_, T_), None), ((A_, C_), None), ((A_, N_), None), ((A_, G_), (93, 20))]
    for j, (bases, quals) in enumerate(order):
        ins_read(R, 300, bases, quals, flag=(0, 16)[j & 1], mapq=20 + 4 * j, nm=len(bases))
        if j % 3 == 0:
            ins_read(R, 300, bases, quals, tail=0, flag=(16, 0)[j & 1], mapq=50 - j, nm=len(bases))      # ... to the read's end
    for j, d in enumerate((2, 5, 2, 5, 5)):
        R.add(300, [(0, 10), (2, d), (0, 10)], flag=(0, 16)[j & 1], mapq=30 + j, nm=d)

    def cells(ws, want, res):
        at = [x for x in res[0].indels if x["pos"] == 309]
        assert sorted(x["allele"] for x in at if x["len"] > 0) == ["+AC", "+ACT", "+AG", "+AN", "+N"] and sorted(x["len"] for x in at if x["len"] < 0) == [-5, -2]
        assert sum(int(x["i"][I_N]) for x in at) == len(order) + 3 + 5
        assert all(int(x["i"][3]) and int(x["i"][4]) for x in at if x["allele"] in ("+AC", "+AG"))      # both strands
    return Case(ref, [(R.arrays(), (250, 360))], cells=cells)


def case_c6():
    """Abandoned positions (-p, reads without a library), two libraries, the window [100, 300): a library-less read over position 150,
    which has indel keys in both libraries (skipped, their slots emptied) beside position 170, whose keys count; k_unavail's clamps (a read
    from 80, before pos0; a read from 290 to 330, behind pos0 + P); library-less reads that do not enter (unmapped; no reference operator)
    over position 200, whose keys count; two library-less reads over 245 .. 259 (the smaller index wins)."""
    ref = ref_of(400); R = pinned(ref, (101, 300))
    for p in (150, 170, 200, 250):
        for l in range(2):
            R.add(p - 9, [(0, 10), (1, 2), (0, 10)], lib=l, flag=(0, 16)[l]); R.add(p - 9, [(0, 10), (2, 3), (0, 10)], lib=l)
    R.add(145, [(0, 11)], lib=-1)
    R.add(80, [(0, 30)], lib=-1); R.add(290, [(0, 40)], lib=-1)
    R.add(195, [(0, 11)], lib=-1, flag=4); R.add(195, [(4, 11)], lib=-1); R.add(196, [(1, 5)], lib=-1)
    R.add(240, [(0, 20)], lib=-1); R.add(245, [(0, 20)], lib=-1)

    def cells(ws, want, res):
        u = res[0].unavail
        free = np.nonzero(u == 0xffffffff)[0] + 100
        taken = sorted(set(range(100, 300)) - set(free.tolist()))
        assert taken == list(range(100, 110)) + list(range(145, 156)) + list(range(240, 265)) + list(range(290, 300)), taken
        assert len(set(u[140:160].tolist())) == 1 and u[140] < u[160] == u[164] != 0xffffffff      # 240 .. 259: the first of the two reads, also where both lie (245 .. 259)
        assert {x["pos"] for x in res[0].indels} == {170, 200}
    return Case(ref, [(R.arrays(), (101, 300))], kw=libs(2), cells=cells, check_warn=False)


# ------------------------------------------------------------------------------------------------ D. the position counter

def case_d(n_libs, r, merged=False, only_last=False):
    """k_finalize counts the printed positions of a multi-library region four per thread: P = 132 + r planes from position 10 on.  The
    lead position has a read of its own and nothing else (it must not count); one position is covered by the last library alone; a run of
    three positions crosses a group of four in front of the tail; plane P - 1 has a read.  only_last: nothing but that one.  merged: the
    same batch as one library (the tiles' own counters)."""
    ref = ref_of(300); R = Reads(ref)
    P = 132 + r; pos0 = 10; last = n_libs - 1
    R.add(pos0 + P - 1, [(0, 1)], lib=last)
    R.add(pos0, [(0, 1)], lib=0)
    if not only_last:
        R.add(pos0 + 7, [(0, 1)], lib=last)
        R.add(pos0 + 20, [(0, 30)], lib=0); R.add(pos0 + 40, [(0, 30)], lib=1 % n_libs, flag=16)
        R.add(pos0 + P - 6, [(0, 3)], lib=0)

    def cells(ws, want, res):
        assert (ws[0]["pos0"], ws[0]["P"], ws[0]["Lp"]) == (pos0, P, 1 if merged else n_libs)
    return Case(ref, [(R.arrays(), (pos0 + 1, pos0 + P))], kw={} if merged else libs(n_libs), cells=cells, lines=[1 if only_last else 1 + 50 + 3 + 1])


# ------------------------------------------------------------------------------------------------ the cases and the routes

BUILDERS = {}
for _total in (255, 256, 257, 512):
    for _spread in (True, False):
        BUILDERS["A1-%d-%s" % (_total, "four_tiles" if _spread else "one_tile")] = (lambda t, s: lambda: case_a1(t, s))(_total, _spread)
BUILDERS["A2-one_engine_four_regions"] = case_a2
BUILDERS["A3-five_libraries"] = case_a3_five
BUILDERS["A3-two_libraries_tile_1028"] = case_a3_two
BUILDERS["A3-workgroup_1024_wraps"] = case_a3_wrap
BUILDERS["A4-last_sublist"] = case_a4_last_sublist
BUILDERS["A4-sublists_255_256"] = case_a4_255_256
BUILDERS["A4-lanes_and_last_plane"] = case_a4_ends
BUILDERS["A4-no_event"] = case_a4_none
BUILDERS["A5-tile_list"] = case_a5_windows
for _k in (1, 2, 3):
    BUILDERS["A6-five_libraries-BRC_XEV_CAP=%d" % _k] = (lambda k: lambda: case_a3_five(env={"BRC_XEV_CAP": str(k)}))(_k)
BUILDERS["B1-arrival_against_sorted"] = case_b1
BUILDERS["B2-order_matters"] = case_b2
BUILDERS["B3-records"] = case_b3
for _l in (1, 2, 3, 5):
    BUILDERS["C1-bucket_sizes-Lp%d" % _l] = (lambda l: lambda: case_c1(l))(_l)
    for _s in (2, 4, 6):
        BUILDERS["C1-bucket_sizes-Lp%d-BRC_IBUCKET_SHIFT=%d" % (_l, _s)] = (lambda l, s: lambda: case_c1(l, env={"BRC_IBUCKET_SHIFT": str(s)}))(_l, _s)
for _l in (1, 3):
    for _w in C2_SHIFT:
        BUILDERS["C2-threshold-Lp%d-%s" % (_l, _w)] = (lambda l, w: lambda: case_c2(l, w))(_l, _w)
BUILDERS["C3-edges"] = case_c3
for _s in (2, 4, 6):
    BUILDERS["C3-edges-BRC_IBUCKET_SHIFT=%d" % _s] = (lambda s: lambda: case_c3(env={"BRC_IBUCKET_SHIFT": str(s)}))(_s)
BUILDERS["C4-unused_slots"] = case_c4
BUILDERS["C5-alleles"] = case_c5
BUILDERS["C6-abandoned"] = case_c6
for _r in range(4):
    for _l in (2, 3):
        BUILDERS["D-Lp%d-P%%4=%d" % (_l, _r)] = (lambda l, r: lambda: case_d(l, r))(_l, _r)
    BUILDERS["D-merged-P%%4=%d" % _r] = (lambda r: lambda: case_d(2, r, merged=True))(_r)
    BUILDERS["D-only_the_last_plane-Lp2-P%%4=%d" % _r] = (lambda r: lambda: case_d(2, r, only_last=True))(_r)
BUILDERS["D-only_the_last_plane-merged"] = lambda: case_d(2, 1, merged=True, only_last=True)
KNOBBED = [n for n in BUILDERS if "BRC_" in n]
PLAIN = [n for n in BUILDERS if "BRC_" not in n]
_cases = {}


@contextlib.contextmanager
def knobs(env):
    """the test knobs of a case in the environment (read by the simulator, the test-knobs library and the checked build; the product
    library and the oracle do not know them)"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def run_windows(lib, case, observe, route):
    """the one region of a case with announced windows: the text of every window, the planes of the region"""
    (arrs, (beg0, end)), = case.steps
    eng = capi.Engine(lib, **route, **case.kw)
    try:
        eng.begin_region(0, beg0, end, case.ref); eng.push_reads(arrs)
        eng.region_windows(np.array([w[0] for w in case.windows], np.int32), np.array([w[1] for w in case.windows], np.int32))
        res = eng.end_region()
        text = b"".join(eng.format_window("chrS", b, e, 0) for b, e in case.windows)
        observe(eng)
        return [text], [res]
    finally:
        eng.close()


def run(lib, case, route=None):
    """texts, results and, per region, (Engine.counts()[1], Engine.passes()) of a case on one engine"""
    seen = []
    has = hasattr(lib.lib, "brc_region_passes")

    def observe(eng):
        seen.append((eng.counts()[1], eng.passes() if has else None))
    with knobs(case.env):
        if case.windows:
            texts, results = run_windows(lib, case, observe, route or {})
        else:
            texts, results = run_steps(lib, case.steps, ref=case.ref, observe=observe, **(route or {}), **case.kw)
    return texts, results, seen


def oracle_of(oracle_lib, case):
    texts, results, seen = run(oracle_lib, Case(case.ref, case.steps, kw=case.kw))
    assert all(s[1] == (1, 0) for s in seen)                        # the oracle: one pass, no lists
    if case.windows:
        (arrs, _), = case.steps
        texts = [b"".join(parity.run_engine(oracle_lib, arrs, [w], ref=case.ref, **case.kw)[0] for w in case.windows)]
    return texts, results


def compare(got, case, what, cap0, load, planes=True):
    """bits and bytes of every region against the oracle; the position counter against the oracle's lines; the passes and the capacity
    against the witness's `load` ("xev_sublist_max": the device's 1024 sub-lists; "n_xev": the simulator's one list), from capacity cap0 on"""
    texts, results, seen = got
    assert len(texts) == len(case.want[0]) == len(seen)
    cap = cap0
    for i, (text, res, (n_positions, passes)) in enumerate(zip(texts, results, seen)):
        at = "%s, region %d" % (what, i)
        wtext, wres = case.want[0][i], case.want[1][i]
        assert (res.pos0, res.n_pos, res.n_lib) == (wres.pos0, wres.n_pos, wres.n_lib), at
        if case.windows:
            asked = np.zeros(res.n_pos, bool)
            for b, e in case.windows:
                asked[b - 1 - res.pos0:e - res.pos0] = True
            for g, w in ((res.ncol, wres.ncol), (res.depth, wres.depth), (res.istat, wres.istat), (res.fstat.view(np.uint32), wres.fstat.view(np.uint32))):
                np.testing.assert_array_equal(g[..., asked], w[..., asked], err_msg=at)
        elif planes:
            parity.assert_results_equal(res, wres, at)
            if case.check_warn:
                assert res.warn[:3] == wres.warn[:3], at
        assert text == wtext, at + ": text differs"
        if case.windows:
            continue                                                # (bits only: neither the counter nor the witness's load describe this launch)
        assert n_positions == wtext.count(b"\n"), "%s: n_positions %d, the oracle prints %d lines" % (at, n_positions, wtext.count(b"\n"))
        expect = 1
        if case.ws[i][load] > cap:
            expect, cap = 2, 2 * case.ws[i][load]
        assert passes == (expect, cap), "%s: (passes, capacity) %r, the witness (%s = %d) says %r" % (at, passes, load, case.ws[i][load], (expect, cap))
        if case.hip_passes and load == "xev_sublist_max":
            assert passes == case.hip_passes[i], at                  # ... and as the case states them for the device's 256 entries a sub-list


def witness_of(sim_lib):
    f = sim_lib.lib.brc_sim_witness; f.restype = ctypes.c_char_p
    return json.loads(f(0).decode())


def sim_cap0(case):
    return int(case.env.get("BRC_XEV_CAP", SIM_CAP0))


def hip_cap0(case):
    return int(case.env.get("BRC_XEV_CAP", XEV_CAP0))


def prepared(name, sim_lib, oracle_lib):
    """the case, built once: the oracle's texts and results, the batch through the simulator with the witness on, [sim] == oracle, the
    hard limit on a bucket's events and the cells the batch was built to hit — before anything goes to a device route"""
    if name in _cases:
        return _cases[name]
    case = BUILDERS[name]()
    for arrs, _ in case.steps:
        assert (np.diff(arrs["pos"].astype(np.int64)) >= 0).all()
    case.want = oracle_of(oracle_lib, case)
    sim_lib.lib.brc_sim_witness.restype = ctypes.c_char_p
    sim_lib.lib.brc_sim_witness(1)
    got = run(sim_lib, case)
    case.ws = ws = witness_of(sim_lib)
    assert len(ws) == len(case.steps)
    assert max(w["xev_bucket_max"] for w in ws) <= XEV_BUCKET, [w["xev_bucket_max"] for w in ws]
    assert all(w["windows"] == bool(case.windows) for w in ws)
    if case.n_xev is not None:
        assert [w["n_xev"] for w in ws] == case.n_xev and [w["xev_sublist_max"] for w in ws] == case.sub_max, [(w["n_xev"], w["xev_sublist_max"]) for w in ws]
    if case.lines is not None:
        assert [t.count(b"\n") for t in case.want[0]] == case.lines
    compare(got, case, "[sim]", sim_cap0(case), "n_xev")
    if case.cells:
        case.cells(ws, case.want[0], case.want[1])
    _cases[name] = case
    return case


def device_route(lib, case, what):
    compare(run(lib, case), case, what, hip_cap0(case), "xev_sublist_max")
    if not case.windows:
        compare(run(lib, case, dict(device_text="chrS")), case, what + ", device text", hip_cap0(case), "xev_sublist_max", planes=False)


@pytest.fixture(scope="module")
def knobs_hip_lib():
    """libbrc_hip_testknobs.so as build() left it (a missing library is an error)"""
    path = os.path.join(ROOT, "bam_readcount_amd", "csrc", "libbrc_hip_testknobs.so")
    if not os.path.exists(path):
        raise RuntimeError("libbrc_hip_testknobs.so is not built (make -C bam_readcount_amd/csrc)")
    return capi.Library(path)


@pytest.mark.parametrize("name", list(BUILDERS))
def test_sim_equals_oracle_and_the_witness_holds_the_cells(sim_lib, oracle_lib, name):
    case = prepared(name, sim_lib, oracle_lib)
    if not case.windows:
        compare(run(sim_lib, case, dict(device_text="chrS")), case, "[sim], device text", sim_cap0(case), "n_xev", planes=False)


def test_b2_the_order_of_the_sums_matters_on_the_oracle_alone(oracle_lib):
    """B2, shown on the reference alone: the oracle on the batch and on the batch with every group of equal-start reads reversed differ in
    the fp32 sums of the third-allele buckets at no fewer than B2_FLOOR (position, bucket) cells — a condition the batch was built to
    exceed about twice (counted: 39 cells), so that a fold that adds in another order than the column's cannot equal the first run."""
    a, b = case_b2(), case_b2(reverse=True)
    (_, (ra,)), (_, (rb,)) = oracle_of(oracle_lib, a), oracle_of(oracle_lib, b)
    np.testing.assert_array_equal(ra.istat, rb.istat)               # the same events: integer sums do not care
    n = third_cells_that_differ(a.ref, ra, rb)
    print("B2: %d (position, bucket) cells of the third-allele buckets differ in their fp32 sums when equal-start reads swap" % n)
    assert n >= B2_FLOOR, n


def test_b3_both_consumers_read_the_table(sim_lib, oracle_lib):
    """B3: the text looks up the table records — `table` cells (a third base) and `table_named` cells (an N / '=' read base under a
    reference N / '=': slot 0 names the bucket and holds nothing) of the text witness; the dense planes come from the host's fetch."""
    case = prepared("B3-records", sim_lib, oracle_lib)
    f = sim_lib.lib.brc_sim_text_witness; f.restype = ctypes.c_char_p
    f(1)
    try:
        texts, _, _ = run(sim_lib, case, dict(device_text="chrS"))
        (w,) = json.loads(f(0).decode())
    finally:
        f(-1)
    assert texts == case.want[0]
    table, named = w["cells"]["table"], w["cells"]["table_named"]
    assert sum(table[b][18] for b in range(1, 5)) == 1 and sum(sum(table[b][1::8]) for b in range(1, 5)) >= 8
    assert named[5][40] == 1 and named[0][41] == 1 and table[3][40] == 1
    assert w["xev_bucket_max"] == 40 and w["records_max"] >= 8


@pytest.mark.parametrize("n_libs", [1, 3])
@pytest.mark.parametrize("which", list(C2_SHIFT))
def test_c2_the_text_witness_reports_the_natural_bucket_size(sim_lib, oracle_lib, n_libs, which):
    """C2 once more through the text route: the text witness repeats DevCfg.ibucket_shift of the region its lines were written from"""
    case = prepared("C2-threshold-Lp%d-%s" % (n_libs, which), sim_lib, oracle_lib)
    f = sim_lib.lib.brc_sim_text_witness; f.restype = ctypes.c_char_p
    f(1)
    try:
        texts, _, _ = run(sim_lib, case, dict(device_text="chrS"))
        (w,) = json.loads(f(0).decode())
    finally:
        f(-1)
    assert texts == case.want[0] and w["ibucket_shift"] == C2_SHIFT[which] == case.ws[0]["ibucket_shift"]


# (the checked route stands first: in file order, and in the GPU job, the other libraries run a batch only after the bounds-checked build did)
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BUILDERS))
def test_checked_build_reports_no_violation(checked_lib, sim_lib, oracle_lib, name):
    case = prepared(name, sim_lib, oracle_lib)
    compare(run(checked_lib, case), case, "checked build", hip_cap0(case), "xev_sublist_max")


@pytest.mark.gpu
@pytest.mark.parametrize("name", PLAIN)
def test_product_library(hip_lib, sim_lib, oracle_lib, name):
    device_route(hip_lib, prepared(name, sim_lib, oracle_lib), "product library")


@pytest.mark.gpu
@pytest.mark.parametrize("name", KNOBBED)
def test_knobs_library(knobs_hip_lib, sim_lib, oracle_lib, name):
    device_route(knobs_hip_lib, prepared(name, sim_lib, oracle_lib), "test-knobs library")
