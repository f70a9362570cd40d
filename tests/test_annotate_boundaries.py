"""The annotators — K1 (k_annotate_groups: phase B's mismatch runs, phase C's quality-2 scan) and the wave forms (k_annotate_wave, with and
without EQX) — at every lane, group and pass boundary of their own layout, on reads constructed by hand (no make_batch, no random batch).

No test can see from outside which lane a base sat on, and no CPU build of these kernels exists that could carry a witness (the simulator
annotates through the serial annotate_read()).  But the layout is a pure function of the batch: `Model` below restates it (with the lines of
brc_engine.hip it restates), computes every base's mismatch flag, the runs, the five integers of every read by brute force, and the CELLS a
batch reaches.  Before any device route runs a batch three things are asserted on the CPU:
  a. the census: every cell the batch was built for is there (each family lists its own);
  b. the model's five integers are those of the reference's own fetch_func (bamrc_ref_annotate of oracle/_ref) for exactly these reads;
  c. oracle == [sim] (parity.compare_libs): the batch is a legal input.
Then the routes of tests/test_pileup_boundaries.py: the bounds-checked build, the product ([hip]), [sim]; every comparison is equality of
bits or bytes.  Left out of (b): reads that reach past the reference's end (fetch_func reads unowned memory there, bamreadcount.cpp:149),
and reads that are never pushed or have no bases (nothing of theirs is ever used).

The file runs after build(), like the rest of the suite: the ref_lib fixture it takes from tests/test_ref_compiled.py makes oracle/_ref, whose
Makefile links the bound binaries against tests/sim/libbrc_sim.so and csrc/libbrc_hip.so and has no rule to build either."""
import numpy as np
import pytest

import parity
from bam_readcount_amd import capi
from constructed import NT16, OTHER, Reads, chain, checked_lib, mismatches, ref_of  # noqa: F401  (checked_lib: fixture)
from test_ref_compiled import ref_annotate, ref_lib  # noqa: F401  (ref_lib: fixture)

FUNMAP, FREVERSE, FSECONDARY = 4, 16, 256
M, I, D, N_, S, P, EQ, X = 0, 1, 2, 3, 4, 6, 7, 8
QV = [0, 1, 2, 62, 63, 127, 128, 200, 255]                            # family E's byte values
LANES = [0, 1, 15, 16, 31, 32, 47, 48, 62, 63]                        # both sides of every DPP row boundary and of the pass boundary


# ------------------------------------------------------------------------------------------------ the layout model

def ops_of(arrs, i):
    o = int(arrs["cigar_off"][i]); n = int(arrs["n_cigar"][i])
    return [(int(c) & 15, int(c) >> 4) for c in arrs["cigar"][o:o + n]]


def bases_of(arrs, i):
    L = int(arrs["l_qseq"][i]); o = int(arrs["seq_off"][i])
    b = arrs["seq4"][o:o + (L + 1) // 2]
    return np.stack([b >> 4, b & 15], 1).reshape(-1)[:L]


class Rd:
    pass


class Model:
    """What brc_engine.hip does with a batch before a single value is computed: which annotator takes a read, and where every base of it sits.

    form (k_pick_wave :675-694, K1 phase A :248-263):
      dropped   not pushed (flag & BRC_PUSH_MASK), no operator, a lone operator that is not M / = / X          (:249-251)
      wave/eqx  wave_on (:2497: the region holds a read of five operators, or = / X and three), >= 3 operators, L > 0, regular (no P, no
                empty match operator), inside the reference; more than two M and no = / X: wave; = / X and more than two match
                operators: eqx                                                                                  (:675-694)
      serial    K1's fallback (:260): no reference, outside it, more than two M operators
      nobases   L == 0 (a record stored without its sequence)
      dense     everything else (:263 work_me)
    group form (:277-289, :305-316): wave w holds reads 64w .. 64w+63; its dense reads in order have G = ceil(L / 8) groups, S = exclusive
    prefix sum; global group X = S + g sits at pass X // 64, lane X % 64; base 8g + k is byte k.
    wave form (:890-891): base j is pass j // 64, lane j % 64."""

    def __init__(self, arrs, ref, wave_form=True):
        self.arrs = arrs
        code = NT16[ref]; self.n_ref = n_ref = len(ref); n = len(arrs["pos"])
        all_ops = [ops_of(arrs, i) for i in range(n)]
        nc_max = max(len(o) for o in all_ops)
        has_eqx = any(op in (EQ, X) for o in all_ops for op, _ in o)
        wave_eqx = has_eqx and nc_max >= 3                                      # :2496
        wave_on = wave_form and (nc_max >= 5 or wave_eqx)                       # :2497-2499
        self.reads = []
        for i in range(n):
            r = Rd(); r.i = i; r.ops = ops = all_ops[i]
            r.pos = int(arrs["pos"][i]); r.L = L = int(arrs["l_qseq"][i]); r.flag = int(arrs["flag"][i])
            r.seq = bases_of(arrs, i); r.qual = arrs["qual"][int(arrs["qual_off"][i]):int(arrs["qual_off"][i]) + L].astype(np.int64)
            n_m = sum(op == M for op, _ in ops); n_ml = sum(op in (M, EQ, X) for op, _ in ops); r.n_ml = n_ml
            rlen = sum(l for op, l in ops if op in (M, D, N_, EQ, X))
            eqx = any(op in (EQ, X) for op, _ in ops)
            irregular = any(op == P or op > X or (op in (M, EQ, X) and l == 0) for op, l in ops)
            inside = r.pos >= 0 and r.pos + rlen <= n_ref
            dropped = bool(r.flag & FUNMAP) or not ops or (len(ops) == 1 and ops[0][0] not in (M, EQ, X))
            r.inside = inside
            if wave_on and len(ops) >= 3 and L > 0 and not (r.flag & FUNMAP) and not irregular and inside and (n_ml > 2 if eqx else n_m > 2):
                r.form = "eqx" if eqx else "wave"
            elif dropped:
                r.form = "dropped"
            elif L == 0:
                r.form = "nobases"                                              # (:263: no group, no scan; nothing of it is ever counted)
            elif not inside or n_m > 2 or any(op == P for op, _ in ops):
                r.form = "serial"
            else:
                r.form = "dense"
            # the annotator's walk (bamreadcount.cpp:133-198): M compares and moves both cursors, D / N the reference's, I / S the
            # read's, = / X NEITHER; a reference position past the end ends everything (:151,175).  flag: the rule of :152.
            r.mm = np.zeros(L, bool); r.mops = []; rp = 0; x = r.pos; left = 0; clipped = L; right = L
            stop = False
            for k, (op, l) in enumerate(ops):
                if op == S:
                    clipped -= l
                    if k == 0: left += l
                    else: right -= l
                if stop:
                    continue
                if op == M:
                    r.mops.append((rp, rp + l))
                    m = l if L else 0
                    if x + m > n_ref:
                        m = max(0, n_ref - x); stop = True
                    cur = np.arange(rp, rp + m); rc = code[x:x + m]; b = r.seq[cur]
                    r.mm[cur] = (b != rc) & (rc != 15) & (b != 0)
                    if stop:
                        continue
                    rp += l; x += l
                elif op in (D, N_):
                    x += l
                elif op in (I, S):
                    rp += l
            d = np.diff(np.concatenate([[0], r.mm.astype(np.int8), [0]]))
            r.runs = list(zip(np.nonzero(d == 1)[0].tolist(), (np.nonzero(d == -1)[0] - 1).tolist()))    # maximal runs of read-adjacent mismatches
            zm = sum(int(r.qual[a:b + 1].max()) for a, b in r.runs)                                         # :152-172,199
            rev = bool(r.flag & FREVERSE)                                                                   # :201-238
            other = np.nonzero(r.qual != 2)[0]
            if rev:
                q2 = int(other[0]) - 1 if len(other) else -1
                tp = max(0, left, q2)
            else:
                q2 = int(other[-1]) - 1 if len(other) else -1
                tp = min(L - 1, right)
                if tp > q2 and q2 != -1: tp = q2
            r.ints = (zm, clipped, left, tp, q2); r.left, r.right, r.rev = left, right, rev
            r.stretch = (int(other[0]) if rev else L - 1 - int(other[-1])) if len(other) else L            # quality-2 bases at the 3' end
            self.reads.append(r)
        # group form: the lanes
        self.waves = []
        for w in range(0, n, 64):
            rs = [r for r in self.reads[w:w + 64] if r.form == "dense"]
            wv = Rd(); wv.first = w; wv.reads = self.reads[w:w + 64]; wv.dense = rs
            S_ = 0; read_of, g_of, fl = [], [], []
            for rank, r in enumerate(rs):
                r.G = (r.L + 7) // 8; r.S = S_; r.rank = rank; r.lane_as_read = r.i - w; r.wave = wv; S_ += r.G
                f8 = np.zeros(8 * r.G, bool); f8[:r.L] = r.mm
                read_of += [r.i] * r.G; g_of += range(r.G); fl.append(f8.reshape(r.G, 8))
            wv.T = S_
            wv.read_of = np.array(read_of, np.int64); wv.g_of = np.array(g_of, np.int64)
            wv.fl = np.concatenate(fl) if fl else np.zeros((0, 8), bool)
            wv.nbits = wv.fl.sum(1); wv.bit0 = wv.fl[:, 0].copy() if S_ else np.zeros(0, bool); wv.bit7 = wv.fl[:, 7].copy() if S_ else np.zeros(0, bool)
            same = np.zeros(S_, bool); same[1:] = wv.read_of[1:] == wv.read_of[:-1]
            prev7 = np.zeros(S_, bool); prev7[1:] = wv.bit7[:-1]
            wv.link = wv.bit0 & same & prev7                                     # :426 (lane 0: the carry of lane 63, :473-475 — the same rule)
            nlink = np.zeros(S_, bool); nlink[:-1] = wv.link[1:]
            lane = np.arange(S_) % 64
            wv.hard = (wv.nbits > 0) & ((wv.nbits > 1) | wv.link | (wv.bit7 & ((lane == 63) | nlink)))      # :435
            wv.pass_hard = np.array([wv.hard[p:p + 64].any() for p in range(0, S_, 64)], bool)
            self.waves.append(wv)

    def by_form(self, *forms):
        return [r for r in self.reads if r.form in forms]

    # -------------------------------------------------------------------------------------------- the cells
    def cells(self):
        c = set()
        forms = [r.form for r in self.reads]
        c.add(("n_reads", len(self.reads)))
        for wv in self.waves:
            T = wv.T; fl = wv.fl
            if not wv.dense:
                c.add("wave_without_dense")
            seen_drop = seen_fall = False
            for r in wv.reads:
                if r.form in ("dropped", "nobases"): seen_drop = True
                elif r.form in ("serial", "wave", "eqx"): seen_fall = True
                elif r.runs:
                    if r.rank != r.lane_as_read: c.add("rank_ne_lane")
                    if seen_drop: c.add("dropped_before_target")
                    if seen_fall: c.add("fallback_before_target")
            ser = [k for k, r in enumerate(wv.reads) if r.form == "serial" and not r.inside]
            for k in ser:
                if any(r.form == "dense" and r.runs for r in wv.reads[:k]) and any(r.form == "dense" and r.runs for r in wv.reads[k + 1:]):
                    c.add("serial_among_dense")
            for Xg in range(1, T):                                               # neighbouring lanes (and lane 63 | lane 0 of the next pass)
                l = (Xg - 1) % 64
                if wv.link[Xg]:
                    c.add(("link", l) if l < 63 else ("pb", "same_read_continues"))
                elif wv.read_of[Xg] != wv.read_of[Xg - 1] and wv.bit0[Xg]:
                    a = self.reads[wv.read_of[Xg - 1]]
                    if a.mm[a.L - 1]:
                        if a.L % 8:
                            c.add(("nolink_partial", a.L % 8))
                        else:
                            c.add(("nolink_other_read", l) if l < 63 else ("pb", "other_read_mismatching_first_base"))
                if l == 63 and wv.bit7[Xg - 1] and wv.read_of[Xg] == wv.read_of[Xg - 1] and not wv.bit0[Xg]:
                    c.add(("pb", "same_read_next_base_clean"))
            if T and T % 64 == 0 and wv.bit7[T - 1]:
                c.add(("pb", "no_next_pass"))                                   # :477
            for Xg in np.nonzero(wv.nbits)[0]:                                   # inside a group
                r = self.reads[wv.read_of[Xg]]; g = int(wv.g_of[Xg]); bits = np.nonzero(fl[Xg])[0]
                if len(bits) == 1 and not wv.pass_hard[Xg // 64]:
                    c.add(("lone_byte", int(bits[0])))                           # :436-442, the fast path
                    if 8 * g + bits[0] == r.L - 1 and r.L % 8:
                        c.add(("last_valid", r.L % 8))
                if len(bits) == 2 and not wv.link[Xg]:
                    c.add("pair_adjacent" if bits[1] - bits[0] == 1 else "pair_apart")
                if len(bits) == 8 and not wv.link[Xg] and not (Xg + 1 < T and wv.link[Xg + 1]) and 0 < g < r.G - 1:
                    c.add("full_isolated")
            for r in wv.dense:
                if r.runs and r.L <= 17: c.add(("L", r.L))
                self._run_cells(c, r)
                self._read_cells(c, r)
        for r in self.by_form("wave", "eqx"):
            self._wave_cells(c, r)
        if "serial" in forms: c.add("serial")
        return c

    def _run_cells(self, c, r):
        """family B (runs through whole lanes and passes) and family E (byte values) of a dense read"""
        Sg = r.S
        for a, b in r.runs:
            q = r.qual[a:b + 1]; n = b - a + 1
            pa, pb_ = (Sg + a // 8) // 64, (Sg + b // 8) // 64
            kind = "in_group" if a // 8 == b // 8 else "cross_lane" if pa == pb_ else "cross_pass"
            kinds = [kind]
            if kind == "cross_lane" and any((Sg + g) % 64 in (15, 31, 47) for g in range(a // 8, b // 8)):
                kinds.append("cross_row")                                        # the link crosses a 16-lane DPP row (wave_shr:1 / wave_shl:1)
            if n >= 2:
                m = int(q.argmax())
                for kd in kinds:
                    c.add(("q_max", int(q[m]), kd))
                    for j in range(n):
                        if j != m: c.add(("q_other", int(q[j]), kd))
            gf, gl = (a + 7) // 8, (b + 1) // 8 - 1                              # first / last group the run fills
            if gl < gf:
                continue
            k = gl - gf + 1
            c.add(("full_lanes", k)); c.add(("start_lane", (Sg + gf) % 64)); c.add(("passes_crossed", pb_ - pa))
            if (q == q.max()).sum() == 1:
                m = a + int(q.argmax()); gm = m // 8
                c.add(("max_at", "head" if gm < gf else "tail" if gm > gl else "first" if gm == gf else "last" if gm == gl else "middle"))
                if (Sg + gm) // 64 < pb_: c.add(("max_at", "earlier_pass"))
                if (Sg + gm) // 64 == pb_ - 1 and pb_ - pa == 2: c.add(("max_at", "middle_pass_of_three"))
            for p in range(pa + 1, pb_ + 1):                                     # lanes 0..63 of pass p full, the carry entering lane 0
                if Sg + gf < 64 * p and Sg + gl >= 64 * p + 63: c.add("all_of_a_pass")

    def _read_cells(self, c, r):
        """families D (two M operators) and G (the quality-2 scan) of a dense read"""
        ops = r.ops; strand = "rev" if r.rev else "fwd"
        c.add(("q2", strand, r.L, r.stretch))
        if r.stretch == r.L: c.add("all_q2")
        clip = r.left if r.rev else r.L - r.right
        if clip and r.stretch and clip > r.stretch: c.add("clip_beyond_q2")
        if clip and r.stretch > clip: c.add("q2_beyond_clip")
        inward = np.nonzero(r.qual == 2)[0]
        if len(inward) > r.stretch and r.stretch < r.L: c.add("second_q2_stretch")
        if ops[0][0] == S and r.mops and r.mm[r.mops[0][0]]: c.add(("clip_lead", ops[0][1]))
        if ops[-1][0] == S and r.mops and r.mm[r.mops[-1][1] - 1]: c.add("clip_trail")
        if r.pos == 0 and r.runs: c.add("at_ref_start")
        if r.pos == 0 and ops[0][0] == S and ops[0][1] > 8: c.add("r1off_below_window")        # :323 r1off < -8
        if r.mops and r.pos + sum(l for op, l in ops if op in (M, D, N_)) == self.n_ref and r.mm[r.mops[-1][1] - 1]: c.add("at_ref_end")
        if len(r.mops) == 2:
            (lo1, hi1), (lo2, hi2) = r.mops
            mid = [op for op, l in ops if op in (I, D)]
            if mid == [I]:
                c.add(("junction_mod8", hi1 % 8, "ins")); c.add(("ins_len", lo2 - hi1))
                if r.mm[hi1 - 1] and r.mm[lo2]: c.add("run_broken_by_insertion")
            if mid == [D]:
                c.add(("junction_mod8", hi1 % 8, "del")); c.add(("del_len", [l for op, l in ops if op == D][0]))
                if r.mm[hi1 - 1] and r.mm[lo2]: c.add("run_across_deletion")

    def _wave_cells(self, c, r):
        """family H: lane = base"""
        c.add(r.form); w = r.form
        c.add((w, "L%64", r.L % 64))
        c.add((w, "q2", "rev" if r.rev else "fwd", r.L, r.stretch))
        starts = np.array([lo for lo, hi in r.mops if hi > lo], np.int64)
        if r.form == "wave" and np.bincount(starts // 64).max() == 64: c.add("mops_in_pass==64")
        n_del = sum(op == D for op, _ in r.ops)
        own = lambda cell: cell if w == "wave" else (w, cell)
        for a, b in r.runs:
            q = r.qual[a:b + 1]; n = b - a + 1
            kind = "in_pass" if a // 64 == b // 64 else "cross_pass"
            if n >= 2:
                m = int(q.argmax()); c.add((w, "q_max", int(q[m]), kind))
                for j in range(n):
                    if j != m: c.add((w, "q_other", int(q[j]), kind))
            if n == 2 and b % 64 == 0: c.add((w, "link", b // 64, "max_left" if q[0] > q[1] else "max_right"))
            if b % 64 == 63 and b + 1 < r.L and not r.mm[b + 1] and n > 1: c.add((w, "ends_on_lane_63_next_clean"))
            if n >= 64:
                m = a + int(q.argmax())
                c.add((w, "run", n, a % 64, "max_before_last_boundary" if m // 64 < b // 64 else "no_boundary" if a // 64 == b // 64 else "max_in_last_pass"))
            if n_del > 64 and sum(1 for lo, hi in r.mops if a <= lo <= b) > 64: c.add(own("run_over_deletions"))
        if len(r.mops) > 64 and r.runs and all(a == b for a, b in r.runs) and len(r.runs) == len(r.mops): c.add(own("no_two_compared_bases_adjacent"))
        if r.form == "eqx" and r.n_ml > 64: c.add(("eqx", "match_operators>64"))          # (:899: the whole list is searched, several entries per offset)


# ------------------------------------------------------------------------------------------------ building a batch wave by wave

class Placer:
    """adds reads in non-decreasing position (Reads.arrays() then keeps the order written) and counts the groups of the wave being filled:
    at(lane) pads with clean fillers (8 bases, or 8a bases with amax > 1) until the next dense read's first group falls on `lane`;
    close() fills the wave to 64 reads"""

    def __init__(self, R, pos=64, amax=1):
        self.R, self.pos, self.amax, self.n, self.g, self.k = R, pos, amax, 0, 0, 0

    def _count(self, groups):
        self.n += 1; self.g += groups
        if self.n == 64:
            self.n = self.g = 0

    def filler(self, a=1):
        self.R.add(self.pos, [(M, 8 * a)], flag=(0, FREVERSE)[self.k & 1]); self.k += 1
        self.pos += max(3, 2 * a); self._count(a)

    def close(self):
        while self.n:
            self.filler()

    def at(self, lane):
        f = (lane - self.g) % 64
        if self.n + -(-f // self.amax) + 1 > 64:
            self.close(); f = lane
        while f:
            a = min(f, self.amax); self.filler(a); f -= a

    def add(self, ops, dense=True, advance=None, L=None, **kw):
        self.R.add(self.pos, ops, L=L, **kw)
        if L is None:
            L = sum(l for o, l in ops if o in (M, I, S, EQ, X))
        self._count((L + 7) // 8 if dense else 0)
        rlen = sum(l for o, l in ops if o in (M, D, N_, EQ, X))
        self.pos += (rlen // 4 + 8) if advance is None else advance


def quals(at, values):
    """qualities on query offsets (not through the aligned-base table: a base is a base)"""
    def edit(seq, qual, aq, ar, code):
        qual[np.asarray(at, np.int64)] = values
    return edit


def run_edit(a, b, q=30, qmax=None, at=None):
    """bases a..b of a one-operator read mismatch, quality q; the run's single maximum qmax on base `at`"""
    def edit(seq, qual, aq, ar, code):
        seq[a:b + 1] = OTHER[code[ar[a:b + 1]]]; qual[a:b + 1] = q
        if at is not None:
            qual[at] = qmax
    return edit


class Case:
    def __init__(self, name, ref, arrs, want, opts=None, names=(), env=None, wave_form=True):
        self.name, self.ref, self.arrs, self.want = name, ref, arrs, want
        self.opts, self.names, self.env, self.wave_form = opts or {}, names, env or {}, wave_form
        self.regions = [(0, len(ref))]


def finish(name, ref, R, want, variant="plain", long_pos=None):
    """variant: plain / per_lib (two libraries, -p: the one_stream == false instantiation) / sh12 (one 6 000-base read: pack_shift 12,
    the other instantiations of both kernels — family E holds a wave-form and an EQX read for them) / serial (BRC_WAVE_FORM=0: K1's
    serial lane)"""
    if variant == "sh12":
        R.add(long_pos, [(M, 6000)], edit=mismatches([7, 8, 4000]))
    arrs = R.arrays()
    opts, names, env, wave_form = {}, (), {}, True
    if variant == "per_lib":
        arrs["lib"] = (np.arange(len(arrs["pos"])) % 2).astype(arrs["lib"].dtype); opts = dict(per_lib=True); names = ["libA", "libB"]
    if variant == "serial":
        env = {"BRC_WAVE_FORM": "0"}; wave_form = False
    return Case(name, ref, arrs, want, opts, names, env, wave_form)


# ------------------------------------------------------------------------------------------------ A. links at every lane boundary

def case_a(variant):
    ref = ref_of(4_600 + (6_200 if variant == "sh12" else 0)); R = Reads(ref); pl = Placer(R)

    def pairs(seq, qual, aq, ar, code):
        for l in range(63):
            seq[8 * l + 7:8 * l + 9] = OTHER[code[ar[8 * l + 7:8 * l + 9]]]
            qual[8 * l + 7:8 * l + 9] = (41, 29) if l & 1 == 0 else (27, 43)
    for shift in [0] + [1, 15, 16, 31, 32, 47, 48, 62, 63]:                    # two-base runs 8l+7 | 8l+8 for every l, the read's first group on lane `shift`
        pl.at(shift); pl.add([(M, 512)], edit=pairs)
    pl.close()
    ends = chain(mismatches([0], q=33), mismatches([7], q=24))
    for _ in range(64):                                                        # 64 one-group reads, first and last base mismatching: T = 64, no next pass
        pl.add([(M, 8)], edit=ends)
    pl.add([(M, 16)], edit=chain(mismatches([0], q=33), mismatches([15], q=24)))   # groups 0..64: lane 63 | lane 0 in different reads
    for _ in range(63):
        pl.add([(M, 8)], edit=ends)
    for m in range(1, 8):                                                      # A's last group partial, its last valid base mismatching
        pl.at(8 * m); pl.add([(M, 8 + m)], edit=mismatches([8 + m - 1], q=35)); pl.add([(M, 8)], edit=mismatches([0], q=21))
    pl.at(63); pl.add([(M, 16)], edit=mismatches([7], q=37))                   # a run that ends on lane 63's last byte, the next base clean
    pl.close()
    want = {("link", l) for l in range(63)} | {("nolink_other_read", l) for l in range(63)} | {("nolink_partial", m) for m in range(1, 8)}
    want |= {("pb", v) for v in ("same_read_continues", "same_read_next_base_clean", "other_read_mismatching_first_base", "no_next_pass")}
    assert pl.pos < 4_500
    return finish("A-" + variant, ref, R, want, variant, 4_600)


# ------------------------------------------------------------------------------------------------ B. runs through whole lanes and passes

B_RUNS = [(1, 0, 0, 0), (2, 1, 1, 1), (3, 15, 7, 7), (15, 16, 0, 1), (16, 31, 1, 0), (17, 32, 7, 0), (63, 47, 0, 7), (64, 48, 1, 7), (65, 62, 7, 1),
          (128, 63, 1, 1), (130, 0, 0, 0)]                                    # (k full groups, lane of the first, head, tail)


def case_b(variant):
    ref = ref_of(10_400 + (6_200 if variant == "sh12" else 0)); R = Reads(ref); pl = Placer(R, amax=63)
    for k, s, h, t in B_RUNS:
        g0 = 1 if h else 0                                                     # the read's group 0 holds the head
        a = 8 * g0 - h; b = 8 * (g0 + k) + t - 1
        L = 8 * (g0 + k) + 8 + (8 if t else 0)                                 # a clean group behind the run
        first = (s - g0) % 64
        spots = {"first": 8 * g0 + 3, "last": 8 * (g0 + k - 1) + 4}
        if h: spots["head"] = a
        if t: spots["tail"] = b
        if 3 <= k < 63: spots["middle"] = 8 * (g0 + k // 2) + 5                # (the long runs have their middle in "middle_pass")
        p_end = (first + b // 8) // 64
        if p_end == 2: spots["middle_pass"] = 8 * (128 - first) - 3              # in pass 1, where the run ends in pass 2
        for at in spots.values():
            if h == 0 and s == 0:                                              # the run opens a pass; lane 63 before it: ANOTHER read's mismatching last base
                pl.at(63); pl.add([(M, 8)], edit=mismatches([7], q=45))
            pl.at(first); pl.add([(M, L)], edit=run_edit(a, b, 30, 50, at))
    pl.close()
    want = {("full_lanes", k) for k in (1, 2, 3, 15, 16, 17, 63, 64, 65, 128, 130)} | {("start_lane", s) for s in LANES}
    want |= {("passes_crossed", p) for p in (0, 1, 2)} | {("max_at", m) for m in ("head", "first", "middle", "last", "tail", "earlier_pass", "middle_pass_of_three")}
    want |= {"all_of_a_pass", ("pb", "other_read_mismatching_first_base")}
    assert pl.pos < 10_300
    return finish("B-" + variant, ref, R, want, variant, 10_400)


# ------------------------------------------------------------------------------------------------ C. inside a group

def case_c(variant):
    ref = ref_of(1_600); R = Reads(ref); pl = Placer(R)
    for k in range(8):                                                         # a wave without a hard lane: the fast path for every byte
        pl.at(2 + 3 * k); pl.add([(M, 24)], edit=mismatches([8 + k], q=22 + k))
    for m in range(1, 8):
        pl.at(30 + 4 * m); pl.add([(M, 8 + m)], edit=mismatches([8 + m - 1], q=31 + m))
    pl.close()
    pl.at(3); pl.add([(M, 24)], edit=chain(mismatches([10], q=25), mismatches([11], q=36)))
    pl.at(9); pl.add([(M, 24)], edit=chain(mismatches([9], q=25), mismatches([14], q=36)))
    pl.at(15); pl.add([(M, 24)], edit=run_edit(8, 15, 28, 44, 12))
    for L in range(1, 18):
        pl.at(20 + 2 * L if L < 17 else 61); pl.add([(M, L)], edit=chain(mismatches([0], q=26), mismatches([L - 1], q=39)))
    pl.close()
    want = {("lone_byte", k) for k in range(8)} | {("last_valid", m) for m in range(1, 8)} | {"pair_adjacent", "pair_apart", "full_isolated"}
    want |= {("L", L) for L in range(1, 18)}
    assert pl.pos < 1_500
    return finish("C-" + variant, ref, R, want, variant)


# ------------------------------------------------------------------------------------------------ D. two M operators

def case_d(variant):
    n_ref = 6_000
    ref = ref_of(n_ref); R = Reads(ref); pl = Placer(R, pos=0, amax=63)

    def junction(hi1, lo2):
        def edit(seq, qual, aq, ar, code):
            for o in (hi1 - 1, hi1):                                           # (aligned-base indices: the last base of the first M, the first of the second)
                seq[aq[o]] = OTHER[code[ar[o]]]
            qual[aq[hi1 - 1]] = 23 + hi1 % 8; qual[aq[hi1]] = 34
            seq[hi1:lo2] = 4; qual[hi1:lo2] = 45                               # inserted bases: anything
        return edit
    pl.add([(S, 9), (M, 31)], edit=mismatches([0, 1], q=30), advance=0)        # at position 0: r1off = -9 leaves the window (:323)
    pl.add([(M, 12), (D, 3), (M, 12)], edit=junction(12, 12), advance=0)
    pl.add([(M, 24)], edit=mismatches([0], q=30))
    for j in range(8):
        for il in (1, 7, 8, 9):
            pl.at((5 * j + il) % 64); pl.add([(M, 16 + j), (I, il), (M, 24)], edit=junction(16 + j, 16 + j + il))
        for dl in (1, 40):
            pl.at((7 * j + dl) % 64); pl.add([(M, 16 + j), (D, dl), (M, 24)], edit=junction(16 + j, 16 + j))
    for cl in (1, 7, 8, 9):
        pl.at(10 + cl); pl.add([(S, cl), (M, 40)], edit=mismatches([0, 1], q=30))
        pl.at(30 + cl); pl.add([(S, cl), (M, 20), (D, 3), (M, 20), (S, 3)], edit=mismatches([0, 19, 20, 39], q=32))
    pl.at(50); pl.add([(M, 40), (S, 5)], edit=mismatches([39], q=30))
    pl.close()
    assert pl.pos < n_ref - 100
    # the reference's last bases: reads that end exactly there (two M operators; a trailing clip whose groups lie past the slice: r1off > ref_n),
    # and one that overhangs — the serial lane among dense neighbours
    pl.pos = n_ref - 60
    for _ in range(3): pl.filler()
    pl.pos = n_ref - 29; pl.add([(M, 10), (D, 5), (M, 14)], edit=mismatches([9, 10, 23], q=30), advance=0)
    pl.pos = n_ref - 24; pl.add([(M, 24)], edit=mismatches([22, 23], q=30), advance=0)
    pl.pos = n_ref - 16; pl.add([(M, 16), (S, 20)], edit=mismatches([15], q=30), advance=0)
    pl.pos = n_ref - 10; pl.add([(M, 24)], dense=False, edit=lambda seq, qual, aq, ar, code: seq.__setitem__(slice(0, 3), 8), advance=0)
    pl.pos = n_ref - 8; pl.add([(M, 8)], edit=mismatches([0, 7], q=30), advance=0)
    want = {("junction_mod8", j, k) for j in range(8) for k in ("ins", "del")} | {("ins_len", l) for l in (1, 7, 8, 9)} | {("del_len", l) for l in (1, 40)}
    want |= {"run_across_deletion", "run_broken_by_insertion", "clip_trail", "at_ref_start", "r1off_below_window", "at_ref_end", "serial_among_dense", "serial"}
    want |= {("clip_lead", c) for c in (1, 7, 8, 9)}
    c = finish("D-" + variant, ref, R, want, variant)
    return c


# ------------------------------------------------------------------------------------------------ E. byte values

def value_runs(v, left):
    """two runs of four bases: v the maximum (second or third base: left / right of a boundary in their middle), and v beside a larger one"""
    lo, hi = v // 2, min(255, v + 55)
    return ([lo, v, lo, lo] if left else [lo, lo, v, lo]), ([v, v, hi, v] if left else [v, hi, v, v])


def case_e(variant):
    ref = ref_of(8_000 + (6_200 if variant == "sh12" else 0))
    ref[7_000 + 4] = ord("N"); ref[7_100 + 4] = ord("R"); ref[7_200 + 3:7_200 + 6] = np.frombuffer(ref[7_200 + 3:7_200 + 6].tobytes().lower(), np.uint8)
    R = Reads(ref, iupac=True); pl = Placer(R, amax=63)
    for n, v in enumerate(QV):
        r1, r2 = value_runs(v, n & 1)
        pl.at(5 + n); pl.add([(M, 24)], edit=chain(run_edit(1, 4), quals(range(1, 5), r1), run_edit(9, 12), quals(range(9, 13), r2)))           # inside a group
        pl.at(20 + n); pl.add([(M, 32)], edit=chain(run_edit(6, 9), quals(range(6, 10), r1), run_edit(22, 25), quals(range(22, 26), r2)))       # across a lane
        for r in (r1, r2):
            pl.at(63); pl.add([(M, 24)], edit=chain(run_edit(6, 9), quals(range(6, 10), r)))                                                     # across a pass
            if v >= 128:                                                                                                                         # bit 7 set, across a DPP row
                pl.at((15, 31, 47)[n % 3]); pl.add([(M, 24)], edit=chain(run_edit(6, 9), quals(range(6, 10), r)))
    # the wave form: one read, a run over every pass boundary 64p - 2 .. 64p + 1 and one inside every pass
    PRE = [(M, 2), (D, 1), (M, 2), (D, 1)]
    ed = []
    for n, v in enumerate(QV):
        for k, r in enumerate(value_runs(v, n & 1)):
            p = 64 * (2 * n + k + 1)
            ed += [wave_run(p - 2, p + 1), quals(range(p - 2, p + 2), r), wave_run(p + 20, p + 23), quals(range(p + 20, p + 24), r)]
    pl.add(PRE + [(M, 64 * 19 + 4)], dense=False, edit=chain(*ed))
    # ... and one read under = / X operators, a run across its first pass boundary: the EQX instantiations with -p and with SH = 12
    pl.add([(EQ, 2), (D, 1), (X, 2), (D, 1), (M, 200)], dense=False, edit=eqx_view(200, [wave_run(62, 65, 30, 50, 63)]), advance=240)
    pl.close()

    def at(p, what):
        def edit(seq, qual, aq, ar, code):
            seq[2:7] = OTHER[code[ar[2:7]]]; qual[2:7] = 30
            if what == "eq": seq[4] = 0
            if what == "n": seq[4] = 15
        return edit
    assert pl.pos < 7_000
    pl.pos = 7_000; pl.add([(M, 16)], edit=at(4, "ref"), advance=100)       # a reference N under the middle of five mismatching bases: two runs
    pl.add([(M, 16)], edit=at(4, "ref"), advance=100)                          # an IUPAC code: a mismatch like any other
    pl.add([(M, 16)], edit=at(4, "ref"), advance=100)                          # lower case: the same code
    pl.add([(M, 16)], edit=at(4, "eq"), advance=100)                           # '=' in the read: never a mismatch
    pl.add([(M, 16)], edit=at(4, "n"), advance=100)                            # N in the read: a mismatch
    pl.close()
    want = {(k, v, kind) for k in ("q_max", "q_other") for v in QV for kind in ("in_group", "cross_lane", "cross_pass")}
    want |= {(k, v, "cross_row") for k in ("q_max", "q_other") for v in (128, 200, 255)}
    want |= {("wave", k, v, kind) for k in ("q_max", "q_other") for v in QV for kind in ("in_pass", "cross_pass")}
    want |= {"ref_N_in_run", "ref_iupac", "ref_lower", "read_eq_in_run", "read_N_in_run", "eqx", ("eqx", "q_max", 50, "cross_pass")}
    assert pl.pos < 7_950
    return finish("E-" + variant, ref, R, want, variant, 8_000)


def e_cells(case, model):
    """the cells of family E that need the reference's characters"""
    c = set(); code = NT16[case.ref]
    for r in model.by_form("dense"):
        if len(r.ops) != 1 or r.L != 16:
            continue
        rc = code[r.pos:r.pos + r.L]
        for j in range(1, r.L - 1):
            around = r.mm[j - 1] and r.mm[j + 1]
            if around and rc[j] == 15 and not r.mm[j]: c.add("ref_N_in_run")
            if around and rc[j] not in (1, 2, 4, 8, 15) and r.mm[j]: c.add("ref_iupac")
            if around and case.ref[r.pos + j] >= 97 and r.mm[j]: c.add("ref_lower")
            if around and r.seq[j] == 0 and not r.mm[j]: c.add("read_eq_in_run")
            if around and r.seq[j] == 15 and r.mm[j] and rc[j] != 15: c.add("read_N_in_run")
    return c


# ------------------------------------------------------------------------------------------------ F. who is in the wave

F_COUNTS = [1, 63, 64, 65, 255, 256, 257]


def case_f_count(n):
    ref = ref_of(2_000); R = Reads(ref)
    for i in range(n):
        L = 8 + i % 10
        R.add(64 + 5 * i, [(M, L)], flag=(0, FREVERSE)[i & 1], edit=chain(mismatches([0], q=21 + i % 9), mismatches([L - 1], q=37)))
    return finish("F-n%d" % n, ref, R, {("n_reads", n)})


def case_f_rank():
    n_ref = 4_000
    ref = ref_of(n_ref); R = Reads(ref); pl = Placer(R)
    ends = chain(mismatches([0], q=33), mismatches([7], q=24))
    odd = [lambda: pl.add([(M, 8)], dense=False, flag=FUNMAP), lambda: pl.add([], dense=False, L=8), lambda: pl.add([(S, 8)], dense=False),
           lambda: pl.add([(M, 8)], dense=False, L=0, flag=FSECONDARY)]
    for k in range(16):                                                        # in front of, between and behind dense reads with runs on both sides
        odd[k % 4]()
        pl.add([(M, 8)], edit=ends); pl.add([(M, 16)], edit=mismatches([7, 8], q=40 + k))
    odd[0](); pl.close()
    for k in range(64):                                                        # a wave without a dense read
        odd[k % 4]()
    for k in range(8):
        pl.add([(M, 8)], edit=ends)
    pl.close()
    pl.pos = n_ref - 40                                                        # an overhanging read (K1's serial lane) among dense ones
    for k in range(3):
        pl.add([(M, 8)], edit=ends, advance=2)
    pl.add([(M, 8), (D, 30), (M, 8)], dense=False, advance=2, edit=mismatches([3, 4], q=30))
    for k in range(3):
        pl.add([(M, 8)], edit=ends, advance=2)
    want = {"rank_ne_lane", "wave_without_dense", "dropped_before_target", "fallback_before_target", "serial_among_dense"}
    return finish("F-rank", ref, R, want)


# ------------------------------------------------------------------------------------------------ G. the quality-2 scan

G_LENGTHS = [1, 7, 8, 9, 15, 16, 17, 100]
PRE = [(M, 2), (D, 1), (M, 2), (D, 1)]                                         # two tiny operators in front: three M operators, five operators


def q2_edit(L, rev, n, second=True):
    def edit(seq, qual, aq, ar, code):
        qual[:] = 30 + np.arange(L) % 7
        if rev: qual[:n] = 2
        elif n: qual[L - n:] = 2
        if second and L - n >= 5:                                              # a second stretch further in: it must not matter
            if rev: qual[n + 2:n + 4] = 2
            else: qual[L - n - 4:L - n - 2] = 2
    return edit


def g_stretches(L):
    return sorted({s for s in (0, 1, 7, 8, 9, 16, L - 1, L) if 0 <= s <= L})


def case_g():
    ref = ref_of(3_600); R = Reads(ref); pl = Placer(R)
    want = set()
    for L in G_LENGTHS:
        for rev in (False, True):
            for n in g_stretches(L):
                pl.add([(M, L)], flag=FREVERSE if rev else 0, edit=q2_edit(L, rev, n))
                want.add(("q2", "rev" if rev else "fwd", L, n))
                if L >= 7:
                    pl.add(PRE + [(M, L - 4)], dense=False, flag=FREVERSE if rev else 0, edit=q2_edit(L, rev, n))
                    want.add(("wave", "q2", "rev" if rev else "fwd", L, n))
    for rev in (False, True):                                                  # soft clips on the scanned end, shorter and longer than the stretch
        for clip, n in ((5, 9), (9, 5), (8, 8), (20, 3)):
            ops = [(S, clip), (M, 100 - clip)] if rev else [(M, 100 - clip), (S, clip)]
            pl.add(ops, flag=FREVERSE if rev else 0, edit=q2_edit(100, rev, n))
            ops = [(S, clip)] + PRE + [(M, 96 - clip)] if rev else PRE + [(M, 96 - clip), (S, clip)]
            pl.add(ops, dense=False, flag=FREVERSE if rev else 0, edit=q2_edit(100, rev, n))
    pl.close()
    want |= {"all_q2", "clip_beyond_q2", "q2_beyond_clip", "second_q2_stretch"}
    assert pl.pos < 3_450
    return finish("G", ref, R, want)


# ------------------------------------------------------------------------------------------------ H. wave form, lane = base

def wave_run(a, b, q=30, qmax=None, at=None):
    """query bases a..b mismatch the reference base they are compared with (a read whose long M operator starts at query offset 4 and
    reference offset 6: PRE)"""
    def edit(seq, qual, aq, ar, code):
        seq[a:b + 1] = OTHER[code[ar[a:b + 1]]]; qual[a:b + 1] = q
        if at is not None:
            qual[at] = qmax
    return edit


def eqx_view(n, edits):
    """a read [2= 1D 2X 1D nM]: the annotator's cursors do not move on = / X (bamreadcount.cpp:133-197), so it compares query bases 0 .. n-1
    with the reference from pos + 2 on.  The bases are written for THAT view — equal, then `edits` in query offsets — and the pileup sees
    what it sees."""
    def edit(seq, qual, aq, ar, code):
        lag_ar = ar[0] + 2 + np.arange(len(seq))
        seq[:n] = code[lag_ar[:n]]
        for e in edits:
            e(seq, qual, np.arange(len(seq)), lag_ar, code)
    return edit


def annotator_pairs(ops, pos):
    """(query offset, reference position) of every base the annotator compares (the walk of Model: = / X move neither cursor)"""
    cur, x = [], []; rp = 0; xx = pos
    for op, l in ops:
        if op == M:
            cur += range(rp, rp + l); x += range(xx, xx + l); rp += l; xx += l
        elif op in (D, N_):
            xx += l
        elif op in (I, S):
            rp += l
    return np.array(cur, np.int64), np.array(x, np.int64)


def every_compared_base(ops):
    """every base the annotator compares mismatches, quality 30, the fourth 50"""
    def edit(seq, qual, aq, ar, code):
        cur, x = annotator_pairs(ops, ar[0])
        seq[cur] = OTHER[code[x]]; qual[cur] = 30; qual[cur[3]] = 50
    return edit


def case_h(variant):
    ref = ref_of(7_000); R = Reads(ref); pl = Placer(R)
    want = set()

    def both(n, edits, eqx=True):
        """the read as [PRE nM] with the edits in query offsets, and the same under = / X operators"""
        pl.filler(); pl.add(PRE + [(M, n)], dense=False, edit=chain(*edits))
        if eqx:
            pl.filler(); pl.add([(EQ, 2), (D, 1), (X, 2), (D, 1), (M, n)], dense=False, edit=eqx_view(n, edits), advance=n + 40)
    # two-base runs on 64p - 1 | 64p, the larger quality on either side
    ed = []
    for p in range(1, 9):
        ed += [wave_run(64 * p - 1, 64 * p), quals([64 * p - 1, 64 * p], (41, 29) if p & 1 else (27, 43))]
    both(64 * 8 + 8, ed)
    for w in ("wave", "eqx"):
        want |= {(w, "link", p, "max_left" if p & 1 else "max_right") for p in range(1, 9)}
    # runs of exactly 64, 65, 128, 130 bases from lanes 0, 1, 63; the maximum on the last base before the last pass boundary the run crosses
    for n in (64, 65, 128, 130):
        for lane in (0, 1, 63):
            a = 64 + lane; b = a + n - 1
            at = 64 * (b // 64) - 1 if b // 64 > a // 64 else a + 5
            both(b + 1 - 4 + 9, [wave_run(a, b, 30, 50, at)])
            for w in ("wave", "eqx"):
                want.add((w, "run", n, lane, "no_boundary" if (n, lane) == (64, 0) else "max_before_last_boundary"))
    both(200, [wave_run(60, 63, 30, 50, 61)])                                  # a run ending on lane 63, the next base clean
    want |= {("wave", "ends_on_lane_63_next_clean"), ("eqx", "ends_on_lane_63_next_clean")}
    for L in (128, 129, 191):                                                  # L % 64 = 0, 1, 63: the last base mismatching
        both(L - 4, [wave_run(L - 2, L - 1, 30, 50, L - 1)])
        want |= {("wave", "L%64", L % 64), ("eqx", "L%64", L % 64)}
    # 130 one-base match operators with a deletion between them (one run across all deletions) and with an insertion between them (no two
    # compared bases adjacent); then the same with every fifth operator = or X: 104 M operators at the annotator's lagging offsets, the
    # = / X entries sharing a query offset with the M operator behind them
    for gap in (D, I):
        for mixed in (False, True):
            ops = []
            for k in range(130):
                ops += [((EQ if k % 10 == 4 else X if k % 10 == 9 else M) if mixed else M, 1)] + ([(gap, 1)] if k < 129 else [])
            pl.filler(); pl.add(ops, dense=False, edit=every_compared_base(ops), advance=300 if mixed else None)
    pl.close()
    want |= {"wave", "eqx", "mops_in_pass==64", "run_over_deletions", "no_two_compared_bases_adjacent"}
    want |= {("eqx", "match_operators>64"), ("eqx", "run_over_deletions"), ("eqx", "no_two_compared_bases_adjacent")}
    assert pl.pos < 6_700
    if variant == "serial":
        want = {"serial"}                                                      # (the same reads on K1's serial lane: no wave cell exists)
    return finish("H-" + variant, ref, R, want, variant)


# ------------------------------------------------------------------------------------------------ the cases and the routes

BUILDERS = {}
for _v in ("plain", "per_lib", "sh12"):
    for _f, _b in (("A", case_a), ("B", case_b), ("E", case_e)):
        BUILDERS["%s-%s" % (_f, _v)] = (lambda b, v: lambda: b(v))(_b, _v)
BUILDERS.update({"C-plain": lambda: case_c("plain"), "D-plain": lambda: case_d("plain"), "F-rank": case_f_rank, "G": case_g,
                 "H-plain": lambda: case_h("plain")})
BUILDERS.update({"F-n%d" % n: (lambda n: lambda: case_f_count(n))(n) for n in F_COUNTS})
KNOB_BUILDERS = {"H-serial": lambda: case_h("serial")}
PLAIN, KNOBS = sorted(BUILDERS), sorted(KNOB_BUILDERS)
_cases = {}


def prepared(name, monkeypatch=None):
    """the case, built once, its census asserted — before anything goes to a device route"""
    if name not in _cases:
        case = (BUILDERS.get(name) or KNOB_BUILDERS[name])()
        case.model = Model(case.arrs, case.ref, wave_form=case.wave_form)
        census(case)                                                            # (cached only once it holds: a batch whose census fails reaches no route)
        _cases[name] = case
    case = _cases[name]
    if monkeypatch:
        for k, v in case.env.items():
            monkeypatch.setenv(k, v)
    return case


def census(case):
    arrs, m = case.arrs, case.model
    assert (np.diff(arrs["pos"].astype(np.int64)) >= 0).all()                   # the order written is the order run
    (beg0, end), = case.regions                                                 # ... and the region's fetch keeps every read (capi.run_regions)
    assert len(capi.fetch_overlapping(arrs, capi.read_ends(arrs), beg0 - 1, end)) == len(arrs["pos"])
    got = m.cells()
    if case.name.startswith("E-"):
        got |= e_cells(case, m)
    missing = sorted(map(str, case.want - got))
    assert not missing, "%s: cells the batch was built for and does not reach: %s" % (case.name, missing)
    case.cells = got
    if case.wave_form:
        assert not [r.i for r in m.reads if r.form == "serial" and r.inside and r.L], "a read inside the reference on the serial lane"
    longest = max((b - a + 1 for r in m.reads for a, b in r.runs), default=0)
    print("census %-10s %4d cells wanted, %5d reads (%d dense, %d wave, %d eqx, %d serial, %d dropped), longest run %d" % (
        case.name, len(case.want), len(m.reads), *(len(m.by_form(f)) for f in ("dense", "wave", "eqx", "serial")), len(m.by_form("dropped", "nobases")), longest))


@pytest.mark.parametrize("name", PLAIN + KNOBS)
def test_census_every_cell_the_batch_was_built_for(name):
    case = prepared(name)
    assert case.want <= case.cells and len(case.want) > 0


@pytest.mark.parametrize("name", PLAIN)
def test_model_integers_equal_reference_fetch_func(ref_lib, name):
    """(b): the brute force of the model == bamrc_ref_annotate, read by read.  Left out: reads past the reference's end (fetch_func reads
    unowned memory there), reads never pushed / without operators / without bases (nothing of theirs is used)."""
    case = prepared(name)
    keep = [r.i for r in case.model.reads if r.inside and r.form != "dropped" and r.L > 0]
    assert len(keep) >= len(case.model.by_form("dense", "wave", "eqx"))
    zm = ref_annotate(ref_lib, capi.select_reads(case.arrs, keep), case.ref)
    want = np.array([case.model.reads[i].ints for i in keep], np.int64)
    bad = np.nonzero((zm != want).any(1))[0]
    assert not len(bad), "read %d (%s): model %r, fetch_func %r" % (keep[bad[0]], case.model.reads[keep[bad[0]]].ops[:6], tuple(want[bad[0]]), tuple(zm[bad[0]]))


def check(lib, oracle_lib, case, device_text=False):
    """parity.compare_libs against the oracle — planes, indel lists, warnings, text —, the oracle's side computed once per batch and kept
    (it is most of what a route costs, and every route of a batch compares with the same one)"""
    kw = dict(ref=case.ref, lib_names=case.names, **case.opts)
    if not hasattr(case, "oracle"):
        case.oracle = parity.run_engine(oracle_lib, case.arrs, case.regions, **kw)
    text, res = parity.run_engine(lib, case.arrs, case.regions, **kw)
    for i, (x, y) in enumerate(zip(res, case.oracle[1])):
        parity.assert_results_equal(x, y, "region %d %r" % (i, case.regions[i]))
        assert x.warn[:3] == y.warn[:3], "warn counts region %d: %r vs %r" % (i, x.warn, y.warn)
    assert len(res) == len(case.oracle[1]) and text == case.oracle[0], "text differs"
    assert text.count(b"\n") >= 8
    if device_text:
        got, _ = parity.run_engine(lib, case.arrs, case.regions, ref=case.ref, lib_names=case.names, device_text="chrS", **case.opts)
        assert got == text


# (the checked route stands first: in file order, and in the GPU job, the product runs a batch only after the bounds-checked build did)
@pytest.mark.gpu
@pytest.mark.parametrize("name", PLAIN + KNOBS)
def test_checked_build_reports_no_violation(checked_lib, oracle_lib, monkeypatch, name):
    check(checked_lib, oracle_lib, prepared(name, monkeypatch))


@pytest.mark.parametrize("name", PLAIN)
def test_constructed_reads_equal_oracle(dev_lib, oracle_lib, monkeypatch, name):
    check(dev_lib, oracle_lib, prepared(name, monkeypatch), device_text=True)


@pytest.mark.parametrize("name", KNOBS)
def test_constructed_reads_equal_oracle_under_knobs(knob_lib, oracle_lib, monkeypatch, name):
    check(knob_lib, oracle_lib, prepared(name, monkeypatch), device_text=True)
