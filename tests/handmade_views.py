"""Hand-made brc_device_view / brc_device_indels views for the three root side libraries (dense, panel, indels) and two references in
plain Python.  Nothing here computes a region: a view is written down in its compact form — ncol, depth, slotid, si [L][2][9],
sf [L][2][4], unavail, a list of XAgg records, the stride; for indels the 72-byte slot records, seq4 / seq_off / l_qseq and the
reference slice — and placed in the route's memory: numpy for [sim], torch device tensors for [hip].

  expand_reference        expand_slots (brc_host.cpp) as loops — zero, slot 0, slot 1 (integers where non-zero, floats always), then every
                          used record with l < Lp, b < 6, k < P — and the thirteen columns of BasicStat.cpp:117-140, every average
                          np.float32(np.float64(np.float32(sum)) / np.float64(np.float32(count))): a double quotient of two fp32 values
                          rounded once to fp32 is the correctly rounded fp32 quotient (53 >= 2 * 24 + 2)
  indel_table_reference   the contract of include/brc.h (brc_device_indels): live slots of the window, '+' / '-' and the characters by the
                          stated rules, sorted() over (pos, lib, text bytes, slot index)

Neither calls a library under test or reads its core headers.  Floats travel as uint32 bit patterns throughout (`sf`, `fstat`,
`metrics`): a NaN or a -0.0 stays what it was written as."""
import os
import struct
import subprocess
from fractions import Fraction

import numpy as np

from bam_readcount_amd import capi
import abi_side as side
from route import SENT, SENT8

U32 = 0xFFFFFFFF
NONE32 = U32
POISON = 0xDEADBEEF                    # what the stride's padding [P, PS) of every source plane holds
PAD = 3                                # words of every destination behind what the contract lets a call touch
NB, NI, NF, NM = 6, 9, 4, 13
I_N, I_SMQ, I_SSE, I_PLUS, I_MINUS, I_NQ2, I_SMMQ, I_SCLIP, I_SBQ = range(9)
F_SEV, F_SQ2, F_SNM, F_S3P = range(4)
KINDS = ("ncol", "depth", "unavail", "istat", "fstat", "metrics")
OOR, DESC = capi.PANEL_OUT_OF_RANGE, capi.PANEL_NOT_ASCENDING


def planes_of(kind, L):
    return {"ncol": L, "depth": L, "unavail": 1, "istat": L * NB * NI, "fstat": L * NB * NF, "metrics": L * NB * NM}[kind]


def f32bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the dense / panel view

def record(k, lib, bucket, i, f, pad=0):
    """one XAgg record as 16 words: k, library << 8 | bucket, 9 integers, 4 float bit patterns, the pad word"""
    assert len(i) == NI and len(f) == NF
    return [int(k) & U32, ((int(lib) << 8) | int(bucket)) & U32] + [int(x) & U32 for x in i] + [int(x) & U32 for x in f] + [pad & U32]


def records_array(records):
    rec = np.array(records, np.uint32).reshape(len(records), 16)
    used = rec[rec[:, 0] != NONE32]
    keys = [(int(k), int(lb)) for k, lb in used[:, :2]]
    assert len(set(keys)) == len(keys), "two used records of one (position, library, bucket): the device order would be undefined"
    return rec


def make_view(route, A, records=(), stride=None, pos0=0):
    """A = {ncol, depth, slotid [L, P], si [L, 2, 9, P], sf [L, 2, 4, P] (uint32 bit patterns), unavail [P] | None}, all uint32 ->
    (capi.DeviceView, keep-alive buffers).  Source planes have exactly the view's sizes; the stride's padding holds POISON."""
    L, P = A["ncol"].shape
    PS = P if stride is None else stride
    assert PS >= P and A["si"].shape == (L, 2, NI, P) and A["sf"].shape == (L, 2, NF, P) and A["sf"].dtype == np.uint32

    def planes(a, rows):
        out = np.full((rows, PS), POISON, np.uint32)
        out[:, :P] = np.asarray(a, np.uint32).reshape(rows, P)
        return route.copy_bytes(out)
    rec = records_array(records)
    keep = {"ncol": planes(A["ncol"], L), "depth": planes(A["depth"], L), "slotid": planes(A["slotid"], L), "si": planes(A["si"], L * 2 * NI),
            "sf": planes(A["sf"], L * 2 * NF), "xagg": route.copy_bytes(rec)}
    if A.get("unavail") is not None:
        keep["unavail"] = planes(A["unavail"], 1)
    v = capi.DeviceView(route.mem, 0, L, pos0, P, PS, *[route.ptr(keep[k]) for k in ("ncol", "depth", "slotid", "si")],
                        route.ptr(keep["unavail"]) if "unavail" in keep else None, route.ptr(keep["sf"]), route.ptr(keep["xagg"]) if len(rec) else None, len(rec))
    return v, keep


def quotient(s, c):
    """the correctly rounded fp32 quotient of two fp32 arrays, through one double division"""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        return (np.asarray(s, np.float32).astype(np.float64) / np.asarray(c, np.float32).astype(np.float64)).astype(np.float32)


def metrics_reference(i, f):
    """the thirteen columns of BasicStat.cpp:117-140 from integer sums i [..., 9, m] and float-sum bit patterns f [..., 4, m] ->
    float32 bit patterns [..., 13, m]; all zero where the count is, the Q2 column zero where I_NQ2 is"""
    i = np.asarray(i, np.uint32); f = np.asarray(f, np.uint32).view(np.float32)
    ic = i.astype(np.float32)                                    # (float)uint32: round to nearest even
    c = ic[..., I_N, :]
    cols = [c, quotient(ic[..., I_SMQ, :], c), quotient(ic[..., I_SBQ, :], c), quotient(ic[..., I_SSE, :], c), ic[..., I_PLUS, :], ic[..., I_MINUS, :],
            quotient(f[..., F_SEV, :], c), quotient(f[..., F_SNM, :], c), quotient(ic[..., I_SMMQ, :], c), ic[..., I_NQ2, :],
            np.where(i[..., I_NQ2, :] != 0, quotient(f[..., F_SQ2, :], ic[..., I_NQ2, :]), np.float32(0)), quotient(ic[..., I_SCLIP, :], c),
            quotient(f[..., F_S3P, :], c)]
    m = np.stack([np.asarray(x, np.float32) for x in cols], axis=-2)
    m[np.broadcast_to((i[..., I_N, :] == 0)[..., None, :], m.shape)] = 0
    return m.view(np.uint32)


def expand_reference(A, records=()):
    """{kind: uint32 words [planes, P]} of the whole view (a window is a slice of columns)"""
    L, P = A["ncol"].shape
    ist = np.zeros((L, NB, NI, P), np.uint32); fst = np.zeros((L, NB, NF, P), np.uint32)
    for l in range(L):
        for s in (0, 1):
            bk = (A["slotid"][l] >> (8 * s)) & 0xFF
            for b in range(NB):
                at = bk == b
                put = at[None, :] & (A["si"][l, s] != 0)
                ist[l, b][put] = A["si"][l, s][put]
                fst[l, b][:, at] = A["sf"][l, s][:, at]
    for r in records_array(records) if len(records) else ():
        k, l, b = int(r[0]), int(r[1]) >> 8, int(r[1]) & 0xFF
        if k == NONE32 or l >= L or b >= NB or k >= P:
            continue
        ist[l, b, :, k] = r[2:11]; fst[l, b, :, k] = r[11:15]
    un = A["unavail"] if A.get("unavail") is not None else np.full(P, NONE32, np.uint32)
    d = {"ncol": A["ncol"], "depth": A["depth"], "unavail": np.asarray(un, np.uint32)[None, :], "istat": ist, "fstat": fst, "metrics": metrics_reference(ist, fst)}
    out = {k: np.ascontiguousarray(np.asarray(v, np.uint32).reshape(planes_of(k, L), P)) for k, v in d.items()}
    for v in out.values():
        v.setflags(write=False)
    return out


def assert_equals_fp32_division(want, L):
    """the CPU cross-check of the two statements of the metrics: expand_reference's double quotient == test_dense.metrics_of's fp32
    division, bit for bit on every cell that is no NaN (and NaN where the other is); returns the number of NaN cells"""
    import test_dense as td
    P = want["istat"].shape[1]
    other = td.metrics_of(want["istat"].reshape(L, NB, NI, P), want["fstat"].view(np.float32).reshape(L, NB, NF, P)).reshape(L * NB * NM, P)
    mine = want["metrics"].view(np.float32)
    nan = np.isnan(mine)
    assert np.array_equal(nan, np.isnan(other))
    assert np.array_equal(mine.view(np.uint32)[~nan], other.view(np.uint32)[~nan])
    return int(nan.sum())


def _destinations(route, sizes, skew):
    """{kind: (buffer, byte offset)}: sentinel-filled, PAD words behind the contract size; skew: the base lies 4 bytes behind a
    256-byte boundary"""
    out = {}
    for k, words in sizes.items():
        buf = route.sentinel_bytes(4 * (words + PAD) + (260 if skew else 0))
        off = ((-route.ptr(buf)) % 256 + 4) if skew else 0
        assert not skew or (route.ptr(buf) + off) % 256 == 4
        out[k] = (buf, off)
    return out


def _collect(route, bufs, sizes, L, ds):
    out = {}
    for k, (buf, off) in bufs.items():
        w = route.host(buf)[off:off + 4 * (sizes[k] + PAD)].view(np.uint32)
        assert (w[sizes[k]:] == SENT).all(), "%s: written behind the contract size" % k
        out[k] = w[:sizes[k]].reshape(planes_of(k, L), ds)
    return out


def run_dense(route, view, k0, n, ds, kinds=KINDS, skew=False):
    """brc_dense_expand into sentinel-filled destinations of [planes][ds] -> (rc, {kind: uint32 [planes, ds]})"""
    L = int(view.n_lib)
    sizes = {k: planes_of(k, L) * ds for k in kinds}
    bufs = _destinations(route, sizes, skew)
    rc = route.dense.expand_raw(view, k0, n, ds, **{k: route.ptr(b) + off for k, (b, off) in bufs.items()})
    return rc, _collect(route, bufs, sizes, L, ds)


def run_panel(route, view, idx, ds, kinds=KINDS, status=True, skew=False):
    """brc_panel_gather of the list -> (rc, status word, {kind: uint32 [planes, ds]})"""
    L = int(view.n_lib)
    sizes = {k: planes_of(k, L) * ds for k in kinds}
    bufs = _destinations(route, sizes, skew)
    st = route.sentinel_bytes(4)
    ibuf = route.copy_bytes(np.asarray(idx, np.int32))
    rc = route.panel.gather_raw(view, route.ptr(ibuf), len(idx), ds, status=route.ptr(st) if status else None,
                                **{k: route.ptr(b) + off for k, (b, off) in bufs.items()})
    return rc, int(route.host(st)[:4].view(np.uint32)[0]), _collect(route, bufs, sizes, L, ds)


def assert_planes(got, want_cols, n, what, nan_cells=0):
    """got {kind: [planes, ds]} == want_cols {kind: [planes, n]} as bit patterns, the padding [n, ds) still the sentinel; the
    metrics cells whose reference is a NaN (exactly nan_cells of them) must be NaNs and are left out of the bit comparison"""
    for k, g in got.items():
        w = want_cols[k]
        if k == "metrics":
            nan = np.isnan(w.view(np.float32))
            assert int(nan.sum()) == nan_cells, (what, int(nan.sum()))
            assert np.isnan(g[:, :n].view(np.float32)[nan]).all(), "%s: a NaN sum gave no NaN" % what
            g = g.copy(); g[:, :n][nan] = w[nan]
        assert np.array_equal(g[:, :n], w), "%s: %s differs at %r" % (what, k, np.argwhere(g[:, :n] != w)[:4].tolist())
        assert (g[:, n:] == SENT).all(), "%s: %s wrote into the padding" % (what, k)


def panel_columns(want, idx):
    """the reference's columns at the listed indices; an index outside the planes is an empty position"""
    idx = np.asarray(idx, np.int64)
    P = want["ncol"].shape[1]
    col = np.where((idx >= 0) & (idx < P), idx, P)
    return {k: np.concatenate([w, np.full((w.shape[0], 1), NONE32 if k == "unavail" else 0, np.uint32)], axis=1)[:, col] for k, w in want.items()}


# ------------------------------------------------------------------------------------------------ the views of the dense / panel families

def unique_arrays(L, P, unavail=True):
    """every cell of every source plane holds a value unique to its (plane, library, position): below 2^24, so its float form is exact
    and unique too, and never zero"""
    def ids(plane0, rows):
        pl = (plane0 + np.arange(rows))[None, :, None]; l = np.arange(L)[:, None, None]; k = np.arange(P)[None, None, :]
        return (pl * (1 << 18) + l * (1 << 10) + k + 1).astype(np.uint32)
    assert L < 256 and P < 1023
    k = np.arange(P)
    b0 = k % NB; b1 = (b0 + 1 + (k // NB) % (NB - 1)) % NB
    A = {"ncol": ids(0, 1)[:, 0], "depth": ids(1, 1)[:, 0], "slotid": np.broadcast_to((b0 | (b1 << 8)).astype(np.uint32), (L, P)).copy(),
         "si": ids(2, 2 * NI).reshape(L, 2, NI, P), "sf": f32bits(ids(20, 2 * NF).astype(np.float32)).reshape(L, 2, NF, P),
         "unavail": (ids(28, 1)[0, 0] if unavail else None)}
    assert (b0 != b1).all()
    cells = np.concatenate([A["ncol"].ravel(), A["depth"].ravel(), A["si"].ravel(), A["sf"].view(np.float32).astype(np.uint32).ravel()] +
                           ([A["unavail"]] if unavail else []))
    assert np.unique(cells).size == cells.size and cells.min() > 0 and cells.max() < (1 << 24), "cell values are not unique"
    return A


D2_KINDS = 10


def d2_arrays(L=2, P=D2_KINDS + 65):
    """D2: per (library, position) one of ten slot situations, rotating with the position (and shifted per library), on unique cell
    values.  A window of 65 positions from k0 = 0 .. 9 puts every situation on lanes 0, 63 and 64."""
    A = unique_arrays(L, P)
    kinds = np.zeros((L, P), np.int64)
    for l in range(L):
        for k in range(P):
            kind = kinds[l, k] = (k + 3 * l) % D2_KINDS
            b, c = k % NB, (k + 1 + k // NB % (NB - 1)) % NB
            sid = {0: 0xFFFF | ((k * 2654435761) & 0xFFFF0000), 1: b | 0xFF00, 2: 0xFF | (c << 8), 3: b | (c << 8), 4: b | (b << 8), 5: 6 | (c << 8), 6: b | (0x80 << 8),
                   7: 0xFEFE, 8: b | (c << 8) | 0xBEEF0000, 9: c | (c << 8) | 0x80010000}[int(kind)]
            A["slotid"][l, k] = sid
            if kind == 4:
                A["si"][l, 1, 1::2, k] = 0                       # b0 == b1: slot 1's zero integers leave slot 0's, its non-zero ones win
    return A, kinds


def body(tag):
    """13 sums unique to a tag (below 2^16): (9 integers, 4 float bit patterns)"""
    return [0x400000 + tag * 16 + f for f in range(NI)], [int(f32bits(np.float32(0x800000 + tag * 4 + f))) for f in range(NF)]


def d3_case(n_records, empty_slots=False, L=2, P=300, window=(37, 130)):
    """D3: records on the window's edges and on P - 1, unused ones with bodies, records outside the view (library == Lp, bucket 6,
    k == P, k inside the stride's padding, k == 2^31), filled up to n_records with used records of distinct (position, library,
    bucket).  empty_slots: no position names a bucket, every bucket comes from a record."""
    A = unique_arrays(L, P)
    k = np.arange(P)
    A["slotid"][:] = ((k % 3) | (3 << 8)).astype(np.uint32) if not empty_slots else 0xFFFF
    k0, n = window
    rec, t = [], 0

    def add(kk, l, b, pad=0):
        nonlocal t
        t += 1
        rec.append(record(kk, l, b, *body(t), pad=pad))
    for j, kk in enumerate((k0 - 1, k0, k0 + n - 1, k0 + n, P - 1)):
        add(kk, j % L, 4 + j % 2); add(kk, (j + 1) % L, j % 3)             # a bucket no slot names; one a slot names (the record wins)
    for _ in range(4):
        add(NONE32, 0, 1, pad=7)                                          # unused, with a body
    add(k0 + 1, L, 4); add(k0 + 2, 0, 6); add(P, 0, 4); add(P + 1, 1, 5); add(1 << 31, 0, 4); add(k0 + 3, 0x7FFFFF, 0xFF)
    taken = {(r[0], r[1]) for r in rec}
    cand = ((kk, l, b) for b in (5, 4, 2) for l in range(L) for kk in range(P))
    while len(rec) < n_records:
        kk, l, b = next(cand)
        if (kk, (l << 8) | b) not in taken:
            add(kk, l, b)
    assert len(rec) == n_records
    order = np.random.default_rng(n_records).permutation(n_records)
    return A, [rec[i] for i in order]


COUNTS = [1, 3, 7, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 24) + 3, 1 << 31, U32]
SUMS = [0, 1, U32]
FLOATS = [0x80000000, 0x00000001, 0x7F7FFFFF, 0x7F800000, 0x3FC00000, 0xC2F6E979]      # -0.0, a subnormal, FLT_MAX, +inf, 1.5, -123.456
QUIET_NAN = 0x7FC00000
TIE_FLOOR = 48


def rounding_ties(limit=TIE_FLOOR):
    """(sum, count) pairs of small integers whose exact quotient lies within one part in 2^26 of the midpoint of two neighbouring
    fp32 values (an eighth of an ulp or nearer: a division that is not correctly rounded, or rounds twice, lands on the other side):
    the `limit` nearest of the search, nearest first"""
    found = []
    for c in range(3, 160, 2):
        for s in range(1, 256):
            q = Fraction(s, c)
            if q.denominator == 1:
                continue
            x = np.float32(s / c)
            best = None
            for y in (np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))):
                m = (Fraction(float(x)) + Fraction(float(y))) / 2
                rel = abs(q - m) / m
                best = rel if best is None or rel < best else best
            if best <= Fraction(1, 1 << 26):
                found.append((best, s, c))
    found.sort()
    return [(s, c) for _, s, c in found[:limit]], len(found)


def d4_cells():
    """D4: one (9 integers, 4 float bit patterns) per cell; returns (cells, number of tie pairs found by the search, NaN cells placed)"""
    cells = []
    for j, c in enumerate(COUNTS):
        for s in SUMS + [COUNTS[(j + 1) % len(COUNTS)]]:
            i = [c, s, SUMS[(j + 1) % 3], COUNTS[(j + 3) % len(COUNTS)], s, COUNTS[(j + 2) % len(COUNTS)], U32 - j, j, s ^ 1]
            cells.append((i, [FLOATS[(j + f) % len(FLOATS)] for f in range(NF)]))
    ties, n_found = rounding_ties()
    for s, c in ties:
        fs = int(f32bits(np.float32(s)))
        cells.append(([c, s, s, 5, 6, c, s, s, s], [fs, fs, fs, fs]))
        cells.append(([c << 8, s << 8, s, 5, 6, c << 4, s, s, s << 3], [fs, fs, fs, fs]))          # the same quotients from larger operands
    cells.append(([0, 5, 6, 7, 8, 9, 10, 11, 12], [FLOATS[4], FLOATS[5], FLOATS[2], FLOATS[3]]))    # count 0, sums not: thirteen zeros
    cells.append(([9, 5, 6, 7, 8, 0, 10, 11, 12], [FLOATS[4], FLOATS[5], FLOATS[2], FLOATS[3]]))    # I_NQ2 == 0, F_SQ2 != 0
    cells.append(([3, 5, 6, 7, 8, 2, 10, 11, 12], [QUIET_NAN, FLOATS[4], FLOATS[5], FLOATS[4]]))    # the one NaN sum: its average is a NaN
    return cells, n_found, 1


def d4_case(via_records, L=1):
    """D4 as a view: cell j is position j; in slot 0 or 1 by turns (bucket j % 6), or — via_records — in a record over empty slots"""
    cells, n_found, n_nan = d4_cells()
    P = len(cells)
    A = unique_arrays(L, P)
    A["slotid"][:] = 0xFFFF
    rec = []
    for j, (i, f) in enumerate(cells):
        b, s = j % NB, j % 2
        if via_records:
            rec.append(record(j, 0, b, i, f))
        else:
            A["slotid"][0, j] = (b | 0xFF00) if s == 0 else (0xFF | (b << 8))
            A["si"][0, s, :, j] = np.array(i, np.uint64).astype(np.uint32); A["sf"][0, s, :, j] = np.array(f, np.uint64).astype(np.uint32)
    return A, rec, n_found, n_nan


def serialize_view(A, records, stride, pos0, tail):
    """the view as dense_check.cpp / panel_check.cpp read it; tail: the windows or the lists, already packed"""
    L, P = A["ncol"].shape
    PS = P if stride is None else stride
    rec = records_array(records)

    def planes(a, rows):
        out = np.full((rows, PS), POISON, np.uint32); out[:, :P] = np.asarray(a, np.uint32).reshape(rows, P)
        return out.tobytes()
    un = A.get("unavail")
    b = struct.pack("<iiqqQii", L, pos0, P, PS, len(rec), 1 if un is not None else 0, len(tail))
    b += planes(A["ncol"], L) + planes(A["depth"], L) + planes(A["slotid"], L) + planes(A["si"], L * 2 * NI) + planes(A["sf"], L * 2 * NF)
    if un is not None:
        b += planes(un, 1)
    return b + rec.tobytes() + b"".join(tail)


def read_checked(d, o, L, n, ds):
    """one call's destinations out of a *_check_asan result file (every buffer (planes - 1) * ds + n words) -> ({kind: [planes, ds]}, o)"""
    got = {}
    for k in KINDS:
        pl = planes_of(k, L)
        elems = (pl - 1) * ds + n if n else 0
        flat = np.full(pl * ds, SENT, np.uint32); flat[:elems] = d[o:o + elems]; o += elems
        got[k] = flat.reshape(pl, ds)
    return got, o


def run_checker(which, case_bytes, tmp_path, said):
    """make asan in tests/sim_<which>, run <which>_check_asan over the case; returns the result file's bytes"""
    open(tmp_path / "case.bin", "wb").write(case_bytes)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([side.sim_checker(side.SIDE[which]), str(tmp_path / "case.bin"), str(tmp_path / "res.bin")], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, env=env)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    assert p.stdout.decode().strip() == said
    return np.fromfile(tmp_path / "res.bin", np.uint8)


# ------------------------------------------------------------------------------------------------ the indel view

NIBBLE = {0: "=", 1: "A", 2: "C", 4: "G", 8: "T", 15: "N"}          # SAMv1's "=ACMGRSVTWYHKDBN": every other code spells N
CODE = {v: k for k, v in NIBBLE.items()}
DEST_PLANES = dict(pos=1, lib=1, len=1, rep_read=1, rep_qpos=1, istat=9, fstat=4, metrics=13)


def slot(pos, lib, ln, rep_read=0, rep_qpos=0, tag=0, i=None, f=None):
    """one 72-byte record as 18 words; the sums are unique to `tag` unless given"""
    bi, bf = body(tag)
    return [int(pos) & U32, int(lib) & U32, int(ln) & U32, int(rep_read) & U32, int(rep_qpos) & U32] + [int(x) & U32 for x in (i or bi)] + [int(x) & U32 for x in (f or bf)]


def make_reads(reads, lead=1):
    """reads: lists of 4-bit codes -> (seq4 bytes, seq_off, l_qseq); `lead` bytes in front, so that seq_off[0] is odd"""
    seq, off, lq = [0xEE] * lead, [], []
    for r in reads:
        off.append(len(seq)); lq.append(len(r))
        r = list(r) + [0x3] * (len(r) & 1)                                # (the unused low nibble of an odd read is not zero)
        seq += [(r[j] << 4) | r[j + 1] for j in range(0, len(r), 2)]
    return np.array(seq, np.uint8), np.array(off, np.uint64), np.array(lq, np.int32)


def indel_arrays(slots, reads=(), ref=None, ref_lo=0, ref_len=None, pos0=0, n_pos=1, n_lib=1, max_run=4):
    """the plain-data form of a brc_device_indels view; asserts the run bound (records of one position: rank_lane is quadratic)"""
    s = np.array(slots, np.uint32).reshape(len(slots), 18)
    live = s[s[:, 2] != 0]
    run = int(np.unique(live[:, 0], return_counts=True)[1].max()) if len(live) else 0
    assert run <= max_run, "a run of %d records at one position" % run
    seq4, seq_off, l_qseq = make_reads(reads)
    ref = None if ref is None else bytes(ref)
    return dict(slots=s, seq4=seq4, seq_off=seq_off, l_qseq=l_qseq, n_reads=len(reads), ref=ref, ref_lo=ref_lo,
                ref_hi=ref_lo + (len(ref) if ref is not None else 0), ref_len=(ref_lo + len(ref) if ref is not None else 0) if ref_len is None else ref_len,
                pos0=pos0, n_pos=n_pos, n_lib=n_lib, run=run)


def make_indels(route, I):
    """-> (capi.DeviceIndels, keep-alive buffers): every source array has exactly its own size, but the reference slice, which has
    one byte 'Z' behind it: a read at ref_hi spells it (the sanitizer programs get the slice alone)"""
    keep = {k: route.copy_bytes(I[k]) for k in ("slots", "seq4", "seq_off", "l_qseq")}
    if I["ref"] is not None:
        keep["ref"] = route.copy_bytes(np.frombuffer(I["ref"] + b"Z", np.uint8))
    S = len(I["slots"])
    v = capi.DeviceIndels(route.mem, 0, I["n_lib"], I["pos0"], I["n_pos"], route.ptr(keep["slots"]) if S else None, S, route.ptr(keep["seq4"]),
                          route.ptr(keep["seq_off"]), route.ptr(keep["l_qseq"]), I["n_reads"], route.ptr(keep["ref"]) if I["ref"] is not None else None,
                          I["ref_lo"], I["ref_hi"], I["ref_len"])
    return v, keep


def i32(x):
    x = int(x) & U32
    return x - (1 << 32) if x >> 31 else x


def allele_text(I, rec):
    """'+' / '-' and the characters of one record, by the rules of include/brc.h"""
    pos, ln, rr, rq = i32(rec[0]), i32(rec[2]), int(rec[3]), i32(rec[4])
    if ln > 0:
        out = bytearray(b"+")
        for j in range(ln):
            ch = "N"
            q = rq + 1 + j
            if rr < I["n_reads"] and 0 <= q < int(I["l_qseq"][rr]):
                byte = int(I["seq4"][int(I["seq_off"][rr]) + q // 2])
                ch = NIBBLE.get(byte >> 4 if q % 2 == 0 else byte & 15, "N")
            out.append(ord(ch))
        return bytes(out)
    p = pos + 1 + np.arange(-ln, dtype=np.int64)
    out = np.full(-ln, ord("N"), np.uint8)
    if I["ref"] is not None:
        ok = (p >= 0) & (p < I["ref_len"]) & (p >= I["ref_lo"]) & (p < I["ref_hi"])
        raw = np.frombuffer(I["ref"], np.uint8)[np.where(ok, p - I["ref_lo"], 0)] if len(I["ref"]) else np.zeros(-ln, np.uint8)
        out = np.where(ok & (raw != 0), raw, out).astype(np.uint8)
    return b"-" + out.tobytes()


def indel_table_reference(I, first, n):
    """{dest: u32 / u8 words} of the window [first, first + n) — the layout of test_indels.table_of — and the slot index of every row"""
    rows = []
    for s, rec in enumerate(I["slots"]):
        if i32(rec[2]) != 0 and first <= i32(rec[0]) < first + n:
            rows.append((i32(rec[0]), i32(rec[1]), allele_text(I, rec), s))
    rows = sorted(rows)
    order = np.array([r[3] for r in rows], np.int64)
    m = len(rows)
    s = I["slots"][order] if m else np.zeros((0, 18), np.uint32)
    t = {k: s[:, c].reshape(1, m).copy() for c, k in enumerate(("pos", "lib", "len", "rep_read", "rep_qpos"))}
    t["istat"] = s[:, 5:14].T.copy(); t["fstat"] = s[:, 14:18].T.copy()
    t["metrics"] = metrics_reference(t["istat"], t["fstat"])
    text = [r[2] for r in rows]
    t["allele_off"] = np.concatenate([[0], np.cumsum([len(x) for x in text])]).astype(np.uint32)
    t["alleles"] = np.frombuffer(b"".join(text), np.uint8)
    return t, order


def serialize_indels(I, calls):
    """the view as indels_check.cpp reads it; calls: (k0, n, cap, alleles_cap)"""
    b = struct.pack("<iiqQqQqqqii", I["n_lib"], I["pos0"], I["n_pos"], len(I["slots"]), I["n_reads"],
                    len(I["seq4"]), I["ref_lo"], I["ref_hi"], I["ref_len"], 1 if I["ref"] is not None else 0, len(calls))
    b += I["slots"].tobytes() + I["seq_off"].tobytes() + I["l_qseq"].tobytes() + I["seq4"].tobytes() + (I["ref"] if I["ref"] is not None else b"")
    for c in calls:
        b += struct.pack("<qqqq", *c)
    return b
