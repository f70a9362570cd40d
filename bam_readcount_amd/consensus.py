"""The binding of the device-side consensus caller (include/brc_cons.h): libbrc_cons_hip.so, or the CPU build of the same per-lane
functions (tests/cpu_cons).  Cons.call() takes raw addresses; bam_readcount_amd.tensors.consensus() is the interface that allocates and
returns arrays.  Needs ctypes and numpy alone."""
import ctypes as C
import os

import numpy as np

from . import capi

CONS_LIB = os.path.join(capi.HERE, "csrc", "libbrc_cons_hip.so")
CONS_EXPORTS = [
    "brc_cons_create", "brc_cons_destroy", "brc_cons_kind", "brc_cons_last_error", "brc_cons_workspace", "brc_cons_call", "brc_cons_last_timing",
]
CONS_ALIGNED, CONS_FILL_REF, CONS_INS_CENTRIC = 1, 2, 4             # brc_cons_params.flags
CONS_MAX_LIB = 254
CONS_NCNT = 6
CONS_C_NAMES = ("a", "c", "g", "t", "del", "ins")                   # the planes of `cnt`
CONS_C_A, CONS_C_C, CONS_C_G, CONS_C_T, CONS_C_DEL, CONS_C_INS = range(6)
CONS_NO_INS = 0xFFFFFFFF
CONS_TABLE_NOT_ASCENDING, CONS_TABLE_OUT_OF_RANGE = 1, 2            # bits of the status word
CONS_IUPAC = "=ACMGRSVTWYHKDBN"                                     # the code of a set of bases: 1 A + 2 C + 4 G + 8 T
CONS_DESTS = ("counts", "call", "cnt", "ins_rec", "off", "seq")
CONS_UINTS = ("min_depth", "min_count", "num", "den", "ins_min_count", "ins_num", "ins_den", "fill", "gap")


class ConsParams(C.Structure):
    """brc_cons_params (include/brc_cons.h)"""
    _fields_ = [("lib_on", C.c_void_p), ("flags", C.c_uint32)] + [(k, C.c_uint32) for k in CONS_UINTS]


class ConsTable(C.Structure):
    """brc_cons_table (include/brc_cons.h): the sorted indel table, where it lies; count is row I_N of its istat"""
    _fields_ = [("m", C.c_int64), ("stride", C.c_int64), ("pos", C.c_void_p), ("lib", C.c_void_p), ("len", C.c_void_p), ("count", C.c_void_p),
                ("allele_off", C.c_void_p), ("alleles", C.c_void_p), ("alleles_len", C.c_int64)]


def cons_params(lib_on=None, flags=0, min_depth=0, min_count=1, frac=(1, 2), ins_min_count=1, ins_frac=(1, 2), fill="N", gap="-"):
    """(ConsParams, keepalive): lib_on is a sequence of 0 / 1 per library or None (every library counts); fill and gap are characters
    (a one-character str or bytes, or a number)"""
    def char(x):
        return x if isinstance(x, int) else ord(x)
    p = ConsParams(None, flags, min_depth, min_count, frac[0], frac[1], ins_min_count, ins_frac[0], ins_frac[1], char(fill), char(gap))
    keep = None
    if lib_on is not None:
        keep = np.ascontiguousarray(lib_on, np.uint8)
        p.lib_on = keep.ctypes.data
    return p, keep


class Cons(capi._Handle):
    """One handle of a library exporting include/brc_cons.h: the product's libbrc_cons_hip.so (default; raises when it is not built or
    there is no device — nothing falls back) or the CPU build of the same per-lane functions (tests/cpu_cons)."""

    PREFIX, EXPORTS, LIB, NAME = "brc_cons", CONS_EXPORTS, CONS_LIB, "cons"
    PROTOS = {"brc_cons_workspace": (C.c_int64, [C.POINTER(capi.DeviceView), C.c_int64, C.c_int64]),
              "brc_cons_call": (C.c_int, [C.c_void_p, C.POINTER(capi.DeviceView), C.POINTER(capi.DeviceIndels), C.POINTER(ConsParams), C.POINTER(ConsTable)] +
                                [C.c_int64] * 4 + [C.c_void_p] * 9)}

    def workspace(self, view, n, m):
        """bytes of scratch a call over n positions and a table of m records needs"""
        return int(self.lib.brc_cons_workspace(capi._ref(view), n, m))

    def call_raw(self, view, indels, params, table, k0, n, dst_stride, seq_cap=0, counts=None, call=None, cnt=None, ins_rec=None, off=None, seq=None,
                 status=None, workspace=None, stream=None):
        """brc_cons_call as it is: table arrays, scratch, destinations and the status word are addresses (or None) in memory of the
        views' kind; returns the code."""
        return self.lib.brc_cons_call(self.h, capi._ref(view), capi._ref(indels), capi._ref(params), capi._ref(table), k0, n, dst_stride, seq_cap, counts, call,
                                      cnt, ins_rec, off, seq, status, workspace, stream)

    def call(self, view, indels, params, table, k0, n, dst_stride, **kw):
        self._check("brc_cons_call", self.call_raw(view, indels, params, table, k0, n, dst_stride, **kw))

    def last_timing(self):
        """kernel seconds (waits for the launches of the last call), bytes asked for and written"""
        return super().last_timing()
