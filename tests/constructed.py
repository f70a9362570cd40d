"""Batches written down by hand (no make_batch, no random batch), shared by the files that test the device pipeline at its own boundaries:
tests/test_pileup_boundaries.py (k_pileup2) and tests/test_annotate_boundaries.py (k_annotate_groups, k_annotate_wave)."""
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


@pytest.fixture(scope="module")
def checked_lib():
    """libbrc_hip_checked.so as build() left it (it is not built here: a missing library is an error)"""
    if not os.path.exists(CHECKED):
        raise RuntimeError("libbrc_hip_checked.so is not built (make -C bam_readcount_amd/csrc checked)")
    return capi.Library(CHECKED)
