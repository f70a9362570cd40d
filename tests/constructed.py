"""Batches written down by hand (no make_batch, no random batch), shared by the files that test the device pipeline at its own boundaries:
tests/test_pileup_boundaries.py (k_pileup2), tests/test_annotate_boundaries.py (k_annotate_groups, k_annotate_wave) and
tests/test_text_boundaries.py (the device's text; run_steps and queue_scenarios below, the latter also run against the reference's
compiled sources by tests/test_ref_compiled.py) and tests/test_side_paths.py (the third-allele lists, the fold, the indel reduce, the
counters)."""
import os

import numpy as np
import pytest

import synth
from bam_readcount_amd import capi
from conftest import ROOT

CHECKED = os.path.join(ROOT, "bam_readcount_amd", "csrc", "libbrc_hip_checked.so")

# htslib seq_nt16_table (brc_core.h: nt16_of_char): IUPAC character of either case -> 4-bit code; everything else 15
NT16 = np.full(256, 15, np.uint8)
for _i, _c in enumerate("=ACMGRSVTWYHKDBN"):
    NT16[ord(_c)] = _i; NT16[ord(_c.lower())] = _i
ACGT_CODE = np.zeros(256, np.uint8); ACGT_CODE[[65, 67, 71, 84]] = [1, 2, 4, 8]
OTHER = np.ones(16, np.uint8); OTHER[[1, 2, 4, 8]] = [2, 4, 8, 1]          # a base that is not the reference's ...
THIRD = np.full(16, 2, np.uint8); THIRD[[1, 2, 4, 8]] = [4, 8, 1, 2]       # ... and one that is neither


class Reads:
    """Reads written down one by one: add(pos, [(op, len)], ...) takes the bases from the reference, `edit(seq, qual, aq, ar)` then changes
    them in place (aq / ar: query offset and reference position of every aligned base).  arrays(): the batch, sorted by position (stable),
    arenas in read order.  iupac: the reference may hold any character (N, IUPAC codes, lower case); a read base over one that is not
    A C G T is A until an edit says otherwise."""

    def __init__(self, ref, iupac=False):
        if iupac:
            self.code = NT16[ref]
        else:
            self.code = ACGT_CODE[ref]; assert self.code.all()
        self.iupac = iupac
        self.ref = ref
        self.n_ref = len(ref)
        self.rows = []

    def add(self, pos, ops, flag=0, mapq=60, lib=0, nm=1, sm=30, tags=3, edit=None, L=None):
        """ops: M (0), = (7) and X (8) take the reference's bases; L: the read's length where the operators do not say it (a read without
        sequence)"""
        if L is None:
            L = sum(l for o, l in ops if o in (0, 1, 4, 7, 8))
        seq = np.ones(L, np.uint8); qual = (20 + (np.arange(L) * 7 + pos) % 21).astype(np.uint8)
        aq, ar = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]; q = 0; r = pos
        for o, l in ops:
            if o in (0, 7, 8):
                aq.append(np.arange(q, q + l)); ar.append(np.arange(r, r + l)); q += l; r += l
            elif o in (1, 4):
                q += l
            elif o in (2, 3):
                r += l
        aq = np.concatenate(aq); ar = np.concatenate(ar)
        if L:
            inside = (ar >= 0) & (ar < self.n_ref)                  # (a read may overhang the reference: those bases stay A)
            seq[aq[inside]] = self.code[ar[inside]]
            if self.iupac:
                seq[~np.isin(seq, (1, 2, 4, 8))] = 1
        if edit:
            edit(seq, qual, aq, ar, self.code)
        self.rows.append((pos, ops, flag, mapq, lib, nm, sm, tags, seq, qual))

    def arrays(self):
        rows = [self.rows[i] for i in np.argsort([r[0] for r in self.rows], kind="stable")]
        cols = list(zip(*rows))
        L = np.array([len(s) for s in cols[8]], np.int64); nc = np.array([len(o) for o in cols[1]], np.int64)
        seq4 = [np.zeros(0, np.uint8)]
        for s in cols[8]:
            s = np.append(s, 0) if len(s) & 1 else s
            seq4.append(((s[0::2] << 4) | s[1::2]).astype(np.uint8))
        a = dict(pos=cols[0], flag=cols[2], mapq=cols[3], lib=cols[4], l_qseq=L, n_cigar=nc, cigar_off=np.cumsum(nc) - nc,
                 seq_off=np.cumsum((L + 1) // 2) - (L + 1) // 2, qual_off=np.cumsum(L) - L, nm=cols[5], sm=cols[6], tags=cols[7],
                 cigar=[(l << 4) | o for ops in cols[1] for o, l in ops], seq4=np.concatenate(seq4), qual=np.concatenate(cols[9]))
        return {k: np.asarray(v).astype(dt) for k, dt in capi.BATCH_DTYPES.items() for v in [a[k]]}


def mismatches(offsets, lut=OTHER, q=None):
    def edit(seq, qual, aq, ar, code):
        o = np.asarray([x for x in offsets if x < len(aq)], np.int64)
        seq[aq[o]] = lut[code[ar[o]]]
        if q is not None:
            qual[aq[o]] = q
    return edit


def chain(*edits):
    def edit(*a):
        for e in edits:
            if e:
                e(*a)
    return edit


def ref_of(n):
    return synth.make_ref(np.random.default_rng(20), n)


def run_steps(lib, steps, ref=None, chrom="chrS", lib_names=(), clear_queue=False, observe=None, **opts):
    """Regions on ONE engine, each with a batch and a target of its own (tests/test_text_boundaries.py, tests/test_ref_compiled.py): a step is
    (arrs, (beg0, end)) or a dict(arrs=, region=, tid=0, continues=False, fetch=True).  fetch: only the reads that overlap [beg0 - 1, end)
    are pushed, as the command line fetches them; continues: BRC_OPT_CONTINUES_PREVIOUS (option 6) is set for the step.  Returns the texts
    and the results, one per step.  observe(eng): called behind every step's text, while the engine still holds the region (counters and
    other observables that no result carries: tests/test_side_paths.py)."""
    eng = capi.Engine(lib, lib_names=lib_names, **opts)
    texts, results = [], []
    try:
        for st in steps:
            if not isinstance(st, dict):
                st = dict(arrs=st[0], region=st[1])
            arrs = st["arrs"]; beg0, end = st["region"]
            if st.get("fetch", True):
                arrs = capi.select_reads(arrs, capi.fetch_overlapping(arrs, capi.read_ends(arrs), beg0 - 1, end))
            if hasattr(lib.lib, "brc_set_option"):
                eng._check(lib.lib.brc_set_option(eng.h, 6, 1 if st.get("continues") else 0))
            else:
                assert not st.get("continues")
            eng.begin_region(st.get("tid", 0), beg0, end, ref); eng.push_reads(arrs)
            results.append(eng.end_region()); texts.append(eng.format_region(chrom))
            if observe:
                observe(eng)
            if clear_queue:
                eng.clear_indel_queue()
        return texts, results
    finally:
        eng.close()


def queue_scenarios():
    """Regions that do NOT start from clean deletion queues (IndelQueue.cpp:3-15; the reference never clears them between command-line
    regions), written down by hand: name -> (ref, steps, kw).  A backbone of plain reads over [0, 1400); deletion reads whose last aligned
    base before the deletion lies at 399 (due at 400), 463 (due at 464: plane index 64 of a region that starts at 400), 319 and 700.
    Every scenario first runs a region that ends at the due position of a deletion, which therefore stays pending."""
    ref = ref_of(1500)

    def batch(n_libs, busy_lib=0, quiet_dels=True):
        R = Reads(ref)
        for s in range(0, 1300, 25):
            for l in range(n_libs):
                R.add(s, [(0, 100)], lib=l, flag=(0, 16)[(s // 25) & 1])
        for last, dl, n in ((399, 3, 2), (399, 7, 1), (463, 2, 1), (319, 4, 2), (700, 5, 1), (401, 2, 1)):
            for j in range(n):
                for l in range(n_libs):
                    if l == busy_lib or quiet_dels:
                        R.add(last - 30 - j, [(0, 31 + j), (2, dl), (0, 40)], lib=l, nm=dl, flag=(0, 16)[j & 1])
        return R.arrays()
    one = batch(1); two = batch(2); two_one_busy = batch(2, busy_lib=1, quiet_dels=False)
    plain = Reads(ref)
    for s in range(0, 1300, 25):
        plain.add(s, [(0, 100)])
    plain = plain.arrays()
    from400 = capi.select_reads(one, np.nonzero(one["pos"] >= 400)[0])
    first =(one, (100, 400))                                       # ends at 400: the deletions queued at 399 stay pending, due at 400
    sc = {
        "due-before_the_first_line": [first, (one, (450, 600)), (one, (390, 410))],
        "due-at_the_first_line": [first, (one, (400, 600)), (one, (390, 410))],
        "due-at_the_first_line-no_lead": [first, (plain, (400, 401)), (one, (400, 600))],
        "due-in_the_middle": [first, (one, (300, 500))],
        "due-at_the_last_line": [first, (one, (300, 401)), (one, (402, 500))],
        "due-behind-blocks_everything": [first, (one, (200, 350)), (one, (310, 330)), (one, (390, 410))],
        "blocked-on_a_bucket_edge": [(one, (100, 464)), (one, (336, 464)), (one, (400, 470))],      # due at 464: behind the second region; plane index 64 of the third
        "blocked-on_index_0": [first, (one, (300, 400)), dict(arrs=from400, region=(400, 500), fetch=False)],      # (no read before 400: the due position is plane index 0)
        "another_tid-dropped_at_the_first_position": [dict(arrs=one, region=(100, 400), tid=1), (one, (300, 500)), (one, (390, 410))],
        "after_a_busy_region_that_left_nothing": [first, (one, (395, 420)), (one, (300, 500)), (plain, (300, 500))],
    }
    out = {k: (ref, v, dict()) for k, v in sc.items()}
    names = ["libA", "libB"]
    out["two_libraries-both_busy"] = (ref, [(two, (100, 400)), (two, (300, 500))], dict(per_lib=True, lib_names=names))
    out["two_libraries-one_busy"] = (ref, [(two_one_busy, (100, 400)), (two_one_busy, (450, 600)), (two_one_busy, (300, 500))], dict(per_lib=True, lib_names=names))
    return out


def queue_expectations(name, want):
    """What queue_scenarios() was built to show, name by name (every scenario has an entry), read off the expected text — so that a
    scenario cannot quietly stop showing it"""
    known = []

    def at(scenario):
        known.append(scenario)
        return scenario == name

    def dels(text, pos):
        return [sum(t.startswith(b"-") for t in tok) for tok in (l.split(b"\t") for l in text.split(b"\n") if l) if int(tok[1]) == pos + 1]
    if at("due-before_the_first_line"):
        assert dels(want[1], 464) == [1] and dels(want[1], 450) == [0] and dels(want[2], 400) == [2]      # dropped at the first line: the region's own deletions print
    if at("due-at_the_first_line"):
        assert dels(want[1], 400) == [4]                                          # the pending pair and the pair the lead position queued behind it
    if at("due-in_the_middle"):
        assert dels(want[1], 320) == [0] and dels(want[1], 400) == [2]            # the pending pair; the region's own are stuck behind the entry queued at 319
    if at("due-at_the_first_line-no_lead"):
        assert dels(want[1], 400) == [2] and dels(want[2], 400) == [2]
    if at("due-at_the_last_line"):
        assert dels(want[1], 400) == [2] and dels(want[2], 402) == [1]
    if at("due-behind-blocks_everything"):
        assert dels(want[1], 320) == [0] and dels(want[2], 320) == [0] and dels(want[3], 400) == [2]
    if at("blocked-on_a_bucket_edge"):
        assert dels(want[1], 400) == [0] and dels(want[2], 464) == [1]
    if at("blocked-on_index_0"):
        assert dels(want[1], 320) == [0] and dels(want[2], 400) == [2] and want[2].startswith(b"chrS\t401\t")
    if at("another_tid-dropped_at_the_first_position"):
        assert dels(want[1], 320) == [1] and dels(want[1], 400) == [2]
    if at("after_a_busy_region_that_left_nothing"):
        assert dels(want[1], 400) == [4] and dels(want[2], 400) == [2] and b"\t-" not in want[3]
    if at("two_libraries-both_busy"):
        assert dels(want[1], 320) == [0] and dels(want[1], 400) == [4]            # the pending pair of either library; their own are stuck behind the entries queued at 319
        line = [l for l in want[1].split(b"\n") if l.startswith(b"chrS\t401\t")][0]
        assert line[:line.index(b"\tlibB\t")].count(b"\t-") == 2
    if at("two_libraries-one_busy"):
        assert all(b"\t-" not in l[:l.index(b"libB")] for l in want[2].split(b"\n") if l)
    assert name in known, "scenario %s has no expectation of its own" % name


@pytest.fixture(scope="module")
def checked_lib():
    """libbrc_hip_checked.so as build() left it (it is not built here: a missing library is an error)"""
    if not os.path.exists(CHECKED):
        raise RuntimeError("libbrc_hip_checked.so is not built (make -C bam_readcount_amd/csrc checked)")
    return capi.Library(CHECKED)
