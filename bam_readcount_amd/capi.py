"""ctypes binding of the C-ABI declared in include/brc.h.

Plumbing only: the product is the shared library `bam_readcount_amd/csrc/libbrc_hip.so` (hand-written HIP
for gfx950 behind the C-ABI).  The same binding class can be pointed at any library exporting the ABI;
tests/ use that to drive the CPU oracle (oracle/libbrc_oracle.so) through identical calls.  This module
never falls back to another implementation: if the product library is missing, `load_product()` raises.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PRODUCT_LIB = os.path.join(HERE, "csrc", "libbrc_hip.so")

NBUCKET, NI, NF, NWARN, NKERNEL = 6, 9, 4, 4, 8
I_NAMES = ["n", "smq", "sse", "plus", "minus", "nq2", "smmq", "sclip", "sbq"]
F_NAMES = ["sev", "sq2", "snm", "s3p"]

EXPORTS = [
    "brc_strerror", "brc_last_error", "brc_kernel_name", "brc_engine_kind", "brc_create", "brc_destroy",
    "brc_begin_region", "brc_push_reads", "brc_upload", "brc_compute", "brc_fetch_result", "brc_end_region",
    "brc_clear_indel_queue", "brc_region_counts", "brc_format_region", "brc_format_window", "brc_region_windows",
    "brc_region_warnings", "brc_window_warnings", "brc_warnings_text", "brc_set_option", "brc_format_region_parts",
    "brc_set_chrom", "brc_fetch_window", "brc_compute_n", "brc_host_alloc", "brc_host_free", "brc_push_reads_pinned",
    "brc_region_piece_steps", "brc_region_passes", "brc_device_view_get", "brc_device_indels_get",
]


class Stat(C.Structure):
    _fields_ = [("i", C.c_uint32 * NI), ("f", C.c_float * NF)]


class Config(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("min_mapq", C.c_int32), ("min_bq", C.c_int32), ("max_cnt", C.c_int32),
                ("per_lib", C.c_int32), ("insertion_centric", C.c_int32), ("n_libs", C.c_int32),
                ("lib_names", C.POINTER(C.c_char_p)), ("device", C.c_int32), ("ref_len_check", C.c_int32)]


class ReadBatch(C.Structure):
    _fields_ = [("n_reads", C.c_int64), ("pos", C.c_void_p), ("flag", C.c_void_p), ("mapq", C.c_void_p), ("lib", C.c_void_p),
                ("l_qseq", C.c_void_p), ("n_cigar", C.c_void_p), ("cigar_off", C.c_void_p), ("seq_off", C.c_void_p),
                ("qual_off", C.c_void_p), ("nm", C.c_void_p), ("sm", C.c_void_p), ("tags", C.c_void_p), ("cigar", C.c_void_p),
                ("seq4", C.c_void_p), ("qual", C.c_void_p), ("n_cigar_total", C.c_uint64), ("seq_bytes", C.c_uint64),
                ("qual_bytes", C.c_uint64), ("qname", C.c_void_p)]


class Indel(C.Structure):
    _fields_ = [("pos", C.c_int32), ("lib", C.c_int32), ("len", C.c_int32), ("rep_read", C.c_uint32), ("rep_qpos", C.c_int32),
                ("allele_off", C.c_uint32), ("allele_len", C.c_uint32), ("stat", Stat)]


class Result(C.Structure):
    _fields_ = [("tid", C.c_int32), ("beg0", C.c_int32), ("end", C.c_int32), ("pos0", C.c_int32), ("n_pos", C.c_int64),
                ("stride", C.c_int64), ("n_lib", C.c_int32), ("ncol", C.POINTER(C.c_uint32)), ("depth", C.POINTER(C.c_uint32)),
                ("istat", C.POINTER(C.c_uint32)), ("fstat", C.POINTER(C.c_float)), ("unavail", C.POINTER(C.c_uint32)),
                ("refbase", C.POINTER(C.c_char)), ("n_indel", C.c_int64), ("indel", C.POINTER(Indel)),
                ("alleles", C.POINTER(C.c_char)), ("alleles_len", C.c_uint64), ("n_events", C.c_uint64),
                ("warn", C.c_uint64 * NWARN)]


class DeviceView(C.Structure):
    """brc_device_view (include/brc.h): the compact results of a computed region where they lie."""
    _fields_ = [("memory", C.c_int32), ("device", C.c_int32), ("n_lib", C.c_int32), ("pos0", C.c_int32), ("n_pos", C.c_int64),
                ("stride", C.c_int64), ("ncol", C.c_void_p), ("depth", C.c_void_p), ("slotid", C.c_void_p), ("si", C.c_void_p),
                ("unavail", C.c_void_p), ("sf", C.c_void_p), ("xagg", C.c_void_p), ("n_xagg", C.c_uint64)]


class DeviceIndels(C.Structure):
    """brc_device_indels (include/brc.h): the indel buckets of a computed region where they lie, and what spells their alleles."""
    _fields_ = [("memory", C.c_int32), ("device", C.c_int32), ("n_lib", C.c_int32), ("pos0", C.c_int32), ("n_pos", C.c_int64),
                ("slots", C.c_void_p), ("n_slots", C.c_uint64), ("seq4", C.c_void_p), ("seq_off", C.c_void_p), ("l_qseq", C.c_void_p),
                ("n_reads", C.c_int64), ("ref", C.c_void_p), ("ref_lo", C.c_int64), ("ref_hi", C.c_int64), ("ref_len", C.c_int64)]


MEM_DEVICE, MEM_HOST = 1, 2


class Timing(C.Structure):
    _fields_ = [("ms", C.c_float * NKERNEL), ("total_ms", C.c_float)]


BATCH_DTYPES = dict(pos=np.int32, flag=np.uint16, mapq=np.uint8, lib=np.int16, l_qseq=np.int32, n_cigar=np.uint32,
                    cigar_off=np.uint64, seq_off=np.uint64, qual_off=np.uint64, nm=np.int32, sm=np.int32, tags=np.uint8,
                    cigar=np.uint32, seq4=np.uint8, qual=np.uint8)


class BrcError(RuntimeError):
    pass


def _load(path):
    """CDLL(path), and for a HIP build (lib*_hip*.so) one HIP runtime for the whole process first.

    A PyTorch-ROCm wheel carries its own libamdhip64.so / libhsa-runtime64.so and asks for them by a name (libamdhip64.so) that an
    already loaded system runtime (soname libamdhip64.so.N) does not answer to: with an engine loaded BEFORE torch the process would hold
    two runtimes, the second finds no GPU ("No HIP GPUs are available"), and a tensor could never meet a brc_device_view.  The other
    order is fine — torch's copy carries the soname the HIP libraries here ask for — so that order is made the only one: where an
    installed torch has a runtime of its own it is loaded first (torch itself is not imported), and the libraries of this package
    bind to it, as they always did in a process that imported torch first (bench.py)."""
    if "_hip" in os.path.basename(path):
        _share_torch_hip_runtime()
    return C.CDLL(path)


_torch_hip_runtime = None


def _share_torch_hip_runtime():
    global _torch_hip_runtime
    import sys
    if _torch_hip_runtime is not None or "torch" in sys.modules:       # (an imported torch has loaded it already)
        return
    _torch_hip_runtime = False
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    for d in (spec.submodule_search_locations or []) if spec is not None else []:
        rt = os.path.join(d, "lib", "libamdhip64.so")
        if os.path.exists(rt):
            _torch_hip_runtime = C.CDLL(rt, mode=C.RTLD_GLOBAL)
            return


def _declare(lib, protos, optional=()):
    """protos {symbol: (restype, argtypes)} onto a loaded library; a missing symbol that is not in `optional` is an AttributeError"""
    for name, (restype, argtypes) in protos.items():
        if name in optional and not hasattr(lib, name):
            continue
        f = getattr(lib, name)
        f.restype = restype; f.argtypes = argtypes


_H, _I32, _I64 = C.c_void_p, C.c_int32, C.c_int64
_U64P, _TEXT = C.POINTER(C.c_uint64), [C.POINTER(C.c_char_p), C.POINTER(C.c_size_t)]


class Library:
    """One loaded shared library exporting the brc C-ABI."""

    # {symbol: (restype, argtypes)} of the calls of include/brc.h that this module makes; every call that returns a code is a C.c_int
    PROTOS = {
        "brc_strerror": (C.c_char_p, [C.c_int]), "brc_last_error": (C.c_char_p, [_H]), "brc_kernel_name": (C.c_char_p, [C.c_int]),
        "brc_engine_kind": (C.c_char_p, []),
        "brc_create": (C.c_int, [C.POINTER(Config), C.POINTER(_H)]), "brc_destroy": (None, [_H]),
        "brc_set_option": (C.c_int, [_H, C.c_int, _I64]), "brc_set_chrom": (C.c_int, [_H, C.c_char_p]),
        "brc_begin_region": (C.c_int, [_H, _I32, _I32, _I32, C.c_void_p, _I64]),
        "brc_push_reads": (C.c_int, [_H, C.POINTER(ReadBatch)]), "brc_push_reads_pinned": (C.c_int, [_H, C.POINTER(ReadBatch)]),
        "brc_host_alloc": (C.c_void_p, [C.c_size_t]), "brc_host_free": (None, [C.c_void_p]),
        "brc_region_piece_steps": (C.c_int, [_H, _U64P, _U64P]), "brc_region_passes": (C.c_int, [_H, _U64P, _U64P]),
        "brc_upload": (C.c_int, [_H]),
        "brc_compute": (C.c_int, [_H, C.POINTER(Timing)]), "brc_compute_n": (C.c_int, [_H, _I32, C.POINTER(Timing)]),
        "brc_fetch_result": (C.c_int, [_H, C.POINTER(Result)]), "brc_end_region": (C.c_int, [_H, C.POINTER(Result)]),
        "brc_fetch_window": (C.c_int, [_H, _I32, _I32, C.POINTER(Result)]),
        "brc_clear_indel_queue": (C.c_int, [_H]), "brc_region_counts": (C.c_int, [_H, _U64P, _U64P]),
        "brc_format_region": (C.c_int, [_H, C.POINTER(Result), C.c_char_p] + _TEXT),
        "brc_format_window": (C.c_int, [_H, C.POINTER(Result), C.c_char_p, _I32, _I32, _I32] + _TEXT),
        "brc_region_warnings": (C.c_int, [_H, C.c_char_p, _I64] + _TEXT),
        "brc_window_warnings": (C.c_int, [_H, _I32, _I32, _I64] + _TEXT),
        "brc_warnings_text": (C.c_int, [_H, C.c_char_p, C.c_size_t, _I64, C.POINTER(_I64)] + _TEXT),
        "brc_region_windows": (C.c_int, [_H, C.POINTER(_I32), C.POINTER(_I32), _I64]),
        "brc_device_view_get": (C.c_int, [_H, C.POINTER(DeviceView)]), "brc_device_indels_get": (C.c_int, [_H, C.POINTER(DeviceIndels)]),
    }
    # what the reference-compiled checker libraries lack: options, the zero-copy (pinned) feed, compute_n, fetch_window, warnings,
    # windows, device views, piece steps and passes.  Every other symbol of PROTOS must be there, or the load fails.
    OPTIONAL = {"brc_set_option", "brc_set_chrom", "brc_push_reads_pinned", "brc_host_alloc", "brc_host_free", "brc_region_piece_steps",
                "brc_region_passes", "brc_compute_n", "brc_fetch_window", "brc_region_warnings", "brc_warnings_text", "brc_window_warnings",
                "brc_region_windows", "brc_device_view_get", "brc_device_indels_get"}

    def __init__(self, path):
        if not os.path.exists(path):
            raise BrcError("brc library not found: %s (run `python __graft_entry__.py` / build() first)" % path)
        self.path = path
        self.lib = L = _load(path)
        _declare(L, self.PROTOS, self.OPTIONAL)

    def kind(self):
        return self.lib.brc_engine_kind().decode()

    def kernel_names(self):
        out = []
        for k in range(NKERNEL):
            s = self.lib.brc_kernel_name(k)
            out.append(s.decode() if s else None)
        return out


assert set(Library.PROTOS) <= set(EXPORTS) and Library.OPTIONAL <= set(Library.PROTOS)


def load_product():
    """The HIP engine.  Raises (never substitutes) when the library has not been built.
    BRC_HIP_LIB=<path of another build of libbrc_hip.so> is an A/B profiling knob (tools/gpu_ab.sh)."""
    alt = os.environ.get("BRC_HIP_LIB")
    if alt:
        if not os.path.basename(alt).startswith("libbrc_hip"):
            raise BrcError("BRC_HIP_LIB must name another build of libbrc_hip*.so, got %s" % alt)
        lib = Library(alt)
        if lib.kind() != Library(PRODUCT_LIB).kind():
            raise BrcError("BRC_HIP_LIB is not a HIP engine build: %s" % lib.kind())
        return lib
    return Library(PRODUCT_LIB)


def make_batch(arrs):
    """numpy arrays (names of brc_read_batch) -> (ReadBatch, keepalive list)."""
    keep = {}
    b = ReadBatch()
    n = len(arrs["pos"])
    b.n_reads = n
    for k, dt in BATCH_DTYPES.items():
        if k == "lib" and arrs.get("lib") is None:
            setattr(b, k, None)
            continue
        a = np.ascontiguousarray(arrs[k], dtype=dt)
        if a.size == 0:
            a = np.zeros(1, dt)
        keep[k] = a
        setattr(b, k, a.ctypes.data)
    b.n_cigar_total = int(np.asarray(arrs["cigar"]).size)
    b.seq_bytes = int(np.asarray(arrs["seq4"]).size)
    b.qual_bytes = int(np.asarray(arrs["qual"]).size)
    b.qname = None
    if arrs.get("qname") is not None:                       # read names (warning text only)
        names = [q if isinstance(q, bytes) else str(q).encode() for q in arrs["qname"]]
        arr = (C.c_char_p * max(1, len(names)))(*names)
        keep["qname"] = (names, arr)
        b.qname = C.cast(arr, C.c_void_p)
    return b, keep


def select_reads(arrs, idx):
    """Sub-batch with the reads `idx` (ascending), arenas compacted."""
    idx = np.asarray(idx, np.int64)
    out = {}
    for k in ("pos", "flag", "mapq", "lib", "l_qseq", "n_cigar", "nm", "sm", "tags"):
        if arrs.get(k) is not None:
            out[k] = np.asarray(arrs[k])[idx]
        else:
            out[k] = None
    if arrs.get("qname") is not None:
        out["qname"] = [arrs["qname"][int(i)] for i in idx]
    ncig = np.asarray(arrs["n_cigar"])[idx].astype(np.int64)
    lq = np.asarray(arrs["l_qseq"])[idx].astype(np.int64)
    sb = (lq + 1) // 2

    def gather(src, offs, lens):
        tot = int(lens.sum())
        if tot == 0:
            return np.zeros(0, src.dtype), np.zeros(len(lens), np.uint64)
        starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
        ii = np.repeat(offs.astype(np.int64) - starts, lens) + np.arange(tot)
        return src[ii], starts.astype(np.uint64)

    out["cigar"], out["cigar_off"] = gather(np.asarray(arrs["cigar"]), np.asarray(arrs["cigar_off"])[idx], ncig)
    out["seq4"], out["seq_off"] = gather(np.asarray(arrs["seq4"]), np.asarray(arrs["seq_off"])[idx], sb)
    out["qual"], out["qual_off"] = gather(np.asarray(arrs["qual"]), np.asarray(arrs["qual_off"])[idx], lq)
    return out


class RegionResult:
    """Host copy of a brc_result as numpy arrays."""

    def __init__(self, r):
        P, L = int(r.n_pos), int(r.n_lib)
        self.tid, self.beg0, self.end, self.pos0, self.n_pos, self.n_lib = r.tid, r.beg0, r.end, r.pos0, P, L

        S = int(r.stride)

        def arr(ptr, shape, dt):
            """planes are `stride` elements apart; keep the P valid ones"""
            if int(np.prod(shape)) == 0 or not ptr:
                return np.zeros(shape, dt)
            full = shape[:-1] + (S,)
            a = np.ctypeslib.as_array(ptr, shape=(int(np.prod(full)),)).view(dt).reshape(full)
            return a[..., :shape[-1]].copy()

        self.ncol = arr(r.ncol, (L, P), np.uint32)
        self.depth = arr(r.depth, (L, P), np.uint32)
        self.istat = arr(r.istat, (L, NBUCKET, NI, P), np.uint32)
        self.fstat = arr(r.fstat, (L, NBUCKET, NF, P), np.float32)
        self.unavail = arr(r.unavail, (P,), np.uint32) if r.unavail else None
        self.refbase = C.string_at(r.refbase, P) if P and r.refbase else b""
        alle = C.string_at(r.alleles, r.alleles_len) if r.alleles_len else b""
        self.indels = []
        for k in range(int(r.n_indel)):
            d = r.indel[k]
            self.indels.append(dict(pos=d.pos, lib=d.lib, len=d.len, rep_read=d.rep_read, rep_qpos=d.rep_qpos,
                                    allele=alle[d.allele_off:d.allele_off + d.allele_len].decode("latin1"),
                                    i=np.array(d.stat.i[:], np.uint32), f=np.array(d.stat.f[:], np.float32)))
        self.n_events = int(r.n_events)
        self.warn = [int(x) for x in r.warn]


class Engine:
    """Mirror of the reference's per-region pileup lifecycle (bam_plbuf_init .. destroy, bamreadcount.cpp:591-605)."""

    def __init__(self, lib, min_mapq=0, min_bq=0, max_cnt=0, per_lib=False, insertion_centric=False, lib_names=(),
                 device=0, ref_len_check=False, text_only=False, device_text=None):
        """text_only: BRC_OPT_TEXT_ONLY — results are consumed through format_region only (no dense planes; istat / fstat
        of fetch_result() come back as zeros)."""
        self.L = lib
        self._names = [s.encode() if isinstance(s, str) else bytes(s) for s in lib_names]
        self._name_arr = (C.c_char_p * max(1, len(self._names)))(*self._names) if self._names else None
        cfg = Config(1, min_mapq, min_bq, max_cnt, int(per_lib), int(insertion_centric), len(self._names),
                     self._name_arr if self._names else None, device, int(ref_len_check))
        self.h = C.c_void_p()
        self._check(lib.lib.brc_create(C.byref(cfg), C.byref(self.h)), create=True)
        if text_only or device_text:
            self._check(lib.lib.brc_set_option(self.h, 1, 1))
        if device_text:                                   # BRC_OPT_DEVICE_TEXT: device_text = the target name of column 1
            self._check(lib.lib.brc_set_option(self.h, 4, 1))
            self._check(lib.lib.brc_set_chrom(self.h, device_text.encode()))
        self._ref = None
        self._res = Result()
        self._pinned = []           # brc_host_alloc buffers of the current region (push_reads_pinned)

    def _check(self, rc, create=False):
        if rc != 0:
            msg = self.L.lib.brc_strerror(rc).decode()
            if not create and self.h:
                msg += ": " + self.L.lib.brc_last_error(self.h).decode()
            raise BrcError("brc error %d (%s)" % (rc, msg))

    def close(self):
        if self.h:
            self.L.lib.brc_destroy(self.h)
            self.h = C.c_void_p()
            self._free_pinned()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def begin_region(self, tid, beg0, end, ref):
        """ref: None or contiguous uint8 numpy array / bytes holding the whole contig."""
        self._free_pinned()                           # (the previous region's adopted arenas: the engine is done with them now)
        if ref is None:
            self._ref = None
            self._check(self.L.lib.brc_begin_region(self.h, tid, beg0, end, None, 0))
        else:
            self._ref = np.ascontiguousarray(np.frombuffer(ref, np.uint8) if isinstance(ref, (bytes, bytearray)) else ref, np.uint8)
            self._check(self.L.lib.brc_begin_region(self.h, tid, beg0, end, self._ref.ctypes.data, self._ref.size))

    def push_reads(self, arrs):
        b, keep = make_batch(arrs)
        self._check(self.L.lib.brc_push_reads(self.h, C.byref(b)))
        del keep

    def push_reads_pinned(self, arrs):
        """brc_push_reads_pinned: seq4 / qual are first copied into brc_host_alloc memory (what a decoder would have written there
        itself), which this object keeps alive until the next begin_region / close — the engine reads them in place."""
        lib = self.L.lib
        pinned = {}
        for k in ("seq4", "qual"):
            a = np.ascontiguousarray(arrs[k], np.uint8)
            p = lib.brc_host_alloc(max(a.size, 1))
            if not p:
                raise BrcError("brc_host_alloc failed")
            C.memmove(p, a.ctypes.data, a.size)
            buf = np.ctypeslib.as_array((C.c_uint8 * max(a.size, 1)).from_address(p))[:a.size]
            self._pinned.append(p); pinned[k] = buf
        b, keep = make_batch(dict(arrs, **pinned))
        self._check(lib.brc_push_reads_pinned(self.h, C.byref(b)))
        del keep

    def _free_pinned(self):
        for p in self._pinned:
            self.L.lib.brc_host_free(p)
        self._pinned = []

    def upload(self):
        self._check(self.L.lib.brc_upload(self.h))

    def compute(self):
        t = Timing()
        self._check(self.L.lib.brc_compute(self.h, C.byref(t)))
        return [float(x) for x in t.ms], float(t.total_ms)

    def compute_n(self, n):
        """n passes queued back to back, one wait (include/brc.h: brc_compute_n); per-kernel ms averaged over the passes"""
        t = Timing()
        self._check(self.L.lib.brc_compute_n(self.h, n, C.byref(t)))
        return [float(x) for x in t.ms], float(t.total_ms)

    def fetch_result(self):
        self._check(self.L.lib.brc_fetch_result(self.h, C.byref(self._res)))
        return RegionResult(self._res)

    def fetch_window(self, beg0, end):
        """The window [beg0, end) of the last computed region as a stand-alone result (include/brc.h: brc_fetch_window); it
        becomes the engine's current result: format_region() prints it."""
        self._check(self.L.lib.brc_fetch_window(self.h, beg0, end, C.byref(self._res)))
        return RegionResult(self._res)

    def end_region(self):
        self._check(self.L.lib.brc_end_region(self.h, C.byref(self._res)))
        return RegionResult(self._res)

    def counts(self):
        a, b = C.c_uint64(), C.c_uint64()
        self._check(self.L.lib.brc_region_counts(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def device_view(self):
        """brc_device_view_get: the compact results of the last compute where they lie (a DeviceView; valid until the next
        begin_region / upload / close of this engine)."""
        v = DeviceView()
        self._check(self.L.lib.brc_device_view_get(self.h, C.byref(v)))
        return v

    def device_indels(self):
        """brc_device_indels_get: the indel buckets of the last compute where they lie (a DeviceIndels; valid until the next
        begin_region / upload / close of this engine)."""
        v = DeviceIndels()
        self._check(self.L.lib.brc_device_indels_get(self.h, C.byref(v)))
        return v

    def piece_steps(self):
        """(ranged, walked) piece-steps of the last compute (brc_region_piece_steps); (0, 0) when the region was not compacted"""
        a, b = C.c_uint64(), C.c_uint64()
        self._check(self.L.lib.brc_region_piece_steps(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def passes(self):
        """(passes, xev_cap): how often the last compute ran the pipeline and the entries one third-allele sub-list holds now
        (brc_region_passes)"""
        a, b = C.c_uint64(), C.c_uint64()
        self._check(self.L.lib.brc_region_passes(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def clear_indel_queue(self):
        self._check(self.L.lib.brc_clear_indel_queue(self.h))

    def format_region(self, chrom):
        """Text of the last fetched region (bytes), exactly as the reference prints it."""
        p = C.c_char_p(); n = C.c_size_t()
        self._check(self.L.lib.brc_format_region(self.h, C.byref(self._res), chrom.encode(), C.byref(p), C.byref(n)))
        return C.string_at(p, n.value)

    def format_region_np(self, chrom):
        """Text of the last fetched region as a uint8 numpy view of the engine's buffer (no copy; texts above 2 GiB are fine).
        Valid until the next call on this engine."""
        p = C.c_void_p(); n = C.c_size_t()
        self._check(self.L.lib.brc_format_region(self.h, C.byref(self._res), chrom.encode(), C.cast(C.byref(p), C.POINTER(C.c_char_p)), C.byref(n)))
        if not n.value:
            return np.zeros(0, np.uint8)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_ubyte)), shape=(n.value,))

    def region_warnings(self, chrom, cap=-1):
        """Tagged warning events of the last computed region (include/brc.h: brc_region_warnings), bytes."""
        p = C.c_char_p(); n = C.c_size_t()
        self._check(self.L.lib.brc_region_warnings(self.h, chrom.encode(), cap, C.byref(p), C.byref(n)))
        return C.string_at(p, n.value)

    def warnings_text(self, events, max_per_type, counts):
        """ReadWarnings text of an event stream; `counts` (list of 4 ints) are the running per-type counters, updated in place."""
        c = (C.c_int64 * NWARN)(*counts)
        p = C.c_char_p(); n = C.c_size_t()
        self._check(self.L.lib.brc_warnings_text(self.h, events, len(events), max_per_type, c, C.byref(p), C.byref(n)))
        counts[:] = list(c)
        return C.string_at(p, n.value)

    def window_warnings(self, vbeg0, vend, cap=-1):
        """Events of a stand-alone run over [vbeg0,vend) inside the last computed region (site-list planner; no bounds lines)."""
        p = C.c_char_p(); n = C.c_size_t()
        self._check(self.L.lib.brc_window_warnings(self.h, vbeg0, vend, cap, C.byref(p), C.byref(n)))
        return C.string_at(p, n.value)

    def format_window(self, chrom, vbeg0, vend, delta):
        """Text of the sub-window [vbeg0,vend) of the last fetched region, coordinates shifted by -delta (site-list planner)."""
        p = C.c_char_p(); n = C.c_size_t()
        self._check(self.L.lib.brc_format_window(self.h, C.byref(self._res), chrom.encode(), vbeg0, vend, delta, C.byref(p), C.byref(n)))
        return C.string_at(p, n.value)

    def region_windows(self, vbeg0, vend):
        """Announce the only windows [vbeg0[i], vend[i]) of the open region that will be formatted (site-list planner): the engine
        piles up only the tiles they touch."""
        b = np.ascontiguousarray(vbeg0, np.int32); e = np.ascontiguousarray(vend, np.int32)
        assert b.shape == e.shape and b.ndim == 1
        self._check(self.L.lib.brc_region_windows(self.h, b.ctypes.data_as(C.POINTER(C.c_int32)), e.ctypes.data_as(C.POINTER(C.c_int32)), b.size))


def fetch_overlapping(arrs, ends, lo, hi):
    """Indices of reads overlapping [lo,hi) — what samfetch(in, idx, tid, lo, hi, ..) hands to fetch_func
    (bamreadcount.cpp:602; hts iterator: beg clamped at 0, overlap = pos < hi && end > lo)."""
    lo = max(lo, 0)
    pos = np.asarray(arrs["pos"]).astype(np.int64)
    return np.nonzero((pos < hi) & (np.asarray(ends) > lo))[0]


def read_ends(arrs):
    """bam_endpos per read: pos + reference length of the CIGAR (M,D,N,=,X); pos+1 for unmapped / no CIGAR."""
    cig = np.asarray(arrs["cigar"]).astype(np.int64)
    ncig = np.asarray(arrs["n_cigar"]).astype(np.int64)
    off = np.asarray(arrs["cigar_off"]).astype(np.int64)
    op = cig & 15
    ln = np.where((op == 0) | (op == 2) | (op == 3) | (op == 7) | (op == 8), cig >> 4, 0)
    cs = np.concatenate([[0], np.cumsum(ln)])
    rlen = cs[off + ncig] - cs[off]
    flag = np.asarray(arrs["flag"]).astype(np.int64)
    rlen = np.where(((flag & 4) != 0) | (ncig == 0) | (rlen == 0), 1, rlen)   # bam_endpos: rlen 0 counts as 1
    return np.asarray(arrs["pos"]).astype(np.int64) + rlen


def run_regions(engine, arrs, regions, tid, chrom, ref, clear_queue=True):
    """Drive the engine the way the reference's site-list loop does (bamreadcount.cpp:574-607):
    per region fetch [beg0-1, end), begin/push/end, format; returns (text, [RegionResult])."""
    ends = read_ends(arrs)
    text = b""
    results = []
    for (beg0, end) in regions:
        idx = fetch_overlapping(arrs, ends, beg0 - 1, end)
        engine.begin_region(tid, beg0, end, ref)
        engine.push_reads(select_reads(arrs, idx))
        results.append(engine.end_region())
        text += engine.format_region(chrom)
        if clear_queue:
            engine.clear_indel_queue()
    return text, results


def kernel_object_hash(path=None):
    """sha256 (first 16 hex digits) of the DEVICE code of a built library: its `.hip_fatbin` section — the gfx950 code object hipcc embeds,
    which changes when a kernel changes and only then (host-side edits leave it alone).  bench.py stamps the PMC passes under profiles/ with
    it: counters measured on other kernels than the loaded ones are not reported.  None: no such section (the oracle, the simulator)."""
    import hashlib
    import struct
    path = path or PRODUCT_LIB
    with open(path, "rb") as f:
        d = f.read()
    if d[:4] != b"\x7fELF" or d[4] != 2:
        return None
    shoff, = struct.unpack_from("<Q", d, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", d, 0x3A)
    def sh(i):
        name, typ, flags, addr, off, size = struct.unpack_from("<IIQQQQ", d, shoff + i * shentsize)
        return name, off, size
    _, stroff, strsize = sh(shstrndx)
    for i in range(shnum):
        name, off, size = sh(i)
        end = d.index(b"\0", stroff + name)
        if d[stroff + name:end] == b".hip_fatbin":
            return hashlib.sha256(d[off:off + size]).hexdigest()[:16]
    return None


class _Handle:
    """What the handle classes below share: one handle of one loaded library whose C-ABI names start with PREFIX.  The base checks the
    path and the exports, declares the prototypes, creates the handle (a refusal is a BrcError carrying the code as .rc) and owns
    kind(), close(), the (kernel_s, bytes_read, bytes_written) last_timing() and the rc -> BrcError(last_error) check.  A subclass sets
      PREFIX    "brc_dense": the handle's calls are brc_dense_create, _destroy, _kind, _last_error, _last_timing
      EXPORTS   every symbol the library must export
      LIB       the product's library, loaded when no path is given
      NAME      what the "not found" message calls the library
      PROTOS    {symbol: (restype, argtypes)} of the calls that are the library's own
      TIMING    the argtypes of _last_timing behind the handle, where they are not the three of the side libraries
    and holds its own methods only."""
    TIMING = [C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    PROTOS = {}

    def __init__(self, path=None, device=0):
        path = path or self.LIB
        if not os.path.exists(path):
            raise BrcError("%s library not found: %s (run `python __graft_entry__.py` / build() first)" % (self.NAME, path))
        self.path = path
        self.lib = L = _load(path)
        for s in self.EXPORTS:
            if not hasattr(L, s):
                raise BrcError("%s does not export %s" % (path, s))
        protos = {"_kind": (C.c_char_p, []), "_last_error": (C.c_char_p, [C.c_void_p]), "_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
                  "_destroy": (None, [C.c_void_p]), "_last_timing": (None, [C.c_void_p] + self.TIMING)}
        protos = {self.PREFIX + k: v for k, v in protos.items()}
        protos.update(self.PROTOS)
        _declare(L, protos)
        self.device = device
        h = C.c_void_p()
        rc = self._call("_create")(device, C.byref(h))
        if rc != 0:
            e = BrcError("%s_create failed: %d" % (self.PREFIX, rc))
            e.rc = rc
            raise e
        self.h = h

    def _call(self, suffix):
        return getattr(self.lib, self.PREFIX + suffix)

    def kind(self):
        return self._call("_kind")().decode()

    def close(self):
        if self.h:
            self._call("_destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, call, rc):
        if rc != 0:
            raise BrcError("%s: %d (%s)" % (call, rc, self._call("_last_error")(self.h).decode()))

    def last_timing(self):
        k = C.c_double(); r = C.c_uint64(); w = C.c_uint64()
        self._call("_last_timing")(self.h, C.byref(k), C.byref(r), C.byref(w))
        return dict(kernel_s=k.value, bytes_read=r.value, bytes_written=w.value)


def _ref(x):
    return C.byref(x) if x is not None else None


_TIMING5 = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]


class _Codec(_Handle):
    """What the two codec classes share on top of _Handle: the (kernel_s, call_s, bytes_in, bytes_out) last_timing() and the prototypes
    of the page-locked allocator, which carries the library's stem (PREFIX "brc_inflater": brc_inflate_host_alloc, _host_free)."""
    TIMING = _TIMING5

    def __init_subclass__(cls):
        stem = cls.PREFIX[:-1]
        cls.PROTOS = dict(cls.PROTOS, **{stem + "_host_alloc": (C.c_void_p, [C.c_size_t]), stem + "_host_free": (None, [C.c_void_p])})

    def last_timing(self):
        k = C.c_double(); c = C.c_double(); bi = C.c_uint64(); bo = C.c_uint64()
        self._call("_last_timing")(self.h, C.byref(k), C.byref(c), C.byref(bi), C.byref(bo))
        return dict(kernel_s=k.value, call_s=c.value, bytes_in=bi.value, bytes_out=bo.value)


# ---------------------------------------------------------------- the BGZF inflater (include/brc_inflate.h)
INFLATE_LIB = os.path.join(HERE, "csrc", "libbrc_inflate_hip.so")
INFLATE_EXPORTS = [
    "brc_inflater_create", "brc_inflater_destroy", "brc_inflater_kind", "brc_inflater_last_error", "brc_inflate_bgzf",
    "brc_inflate_host_alloc", "brc_inflate_host_free", "brc_inflater_last_timing",
]
INF_OK, INF_BAD_HEADER, INF_BAD_STREAM, INF_SIZE_MISMATCH, INF_CRC_MISMATCH, INF_TRUNCATED = range(6)
E_ARG, E_NODEVICE = -1, -2


class Inflater(_Codec):
    """One inflater handle of a library exporting include/brc_inflate.h: the product's libbrc_inflate_hip.so (default; raises when it
    is not built or there is no device — nothing falls back) or the CPU build of the same decoder (tests/sim_inflate)."""

    PREFIX, EXPORTS, LIB, NAME = "brc_inflater", INFLATE_EXPORTS, INFLATE_LIB, "inflater"
    PROTOS = {"brc_inflate_bgzf": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)])}

    def inflate_raw(self, src, dst_cap=None, capacity=None, whole=False):
        """brc_inflate_bgzf as it is: (rc, bytes of dst, dst_off[0..n], statuses[0..n)).  dst_cap / capacity None: sized by a first,
        size-only call.  dst is pre-filled with 0xA5 (what a failed member's slot must still hold afterwards); whole: all dst_cap
        bytes of it come back, not only the members' slots."""
        src = bytes(src)
        sbuf = np.frombuffer(src, np.uint8) if src else np.zeros(1, np.uint8)
        cap = len(src) // 26 + 1 if capacity is None else capacity
        off = np.zeros(cap + 1, np.uint64); st = np.zeros(max(cap, 1), np.uint8)
        n = C.c_size_t(cap)
        if dst_cap is None:
            self.lib.brc_inflate_bgzf(self.h, sbuf.ctypes.data, len(src), None, 0, off.ctypes.data, st.ctypes.data, C.byref(n))
            dst_cap = int(off[n.value]) if n.value <= cap else 0
            n = C.c_size_t(cap)
        dst = np.full(max(dst_cap, 1), 0xA5, np.uint8)
        rc = self.lib.brc_inflate_bgzf(self.h, sbuf.ctypes.data, len(src), dst.ctypes.data, dst_cap, off.ctypes.data, st.ctypes.data, C.byref(n))
        k = n.value
        if k > cap:
            return rc, b"", np.zeros(0, np.uint64), np.zeros(0, np.uint8), k
        return rc, dst[:dst_cap if whole else min(dst_cap, int(off[k]))].tobytes(), off[:k + 1].copy(), st[:k].copy(), k

    def inflate(self, src):
        """Raw BGZF bytes (whole members back to back) -> (inflated bytes, offsets (n + 1), statuses (n)).  Raises when src is not a
        chain of whole members; members that failed are reported by their status, their bytes are not meaningful."""
        rc, out, off, st, _ = self.inflate_raw(src)
        self._check("brc_inflate_bgzf", rc)
        return out, off, st


# ---------------------------------------------------------------- the BGZF deflater (include/brc_deflate.h)
DEFLATE_LIB = os.path.join(HERE, "csrc", "libbrc_deflate_hip.so")
DEFLATE_EXPORTS = [
    "brc_deflater_create", "brc_deflater_destroy", "brc_deflater_kind", "brc_deflater_last_error", "brc_deflate_bound",
    "brc_deflate_bgzf", "brc_deflate_eof_block", "brc_deflate_host_alloc", "brc_deflate_host_free", "brc_deflater_last_timing",
]
DEFLATE_MEMBER_INPUT = 0xff00


class Deflater(_Codec):
    """One deflater handle of a library exporting include/brc_deflate.h: the product's libbrc_deflate_hip.so (default; raises when it
    is not built or there is no device — nothing falls back) or the CPU build of the same compressor (tests/sim_deflate)."""

    PREFIX, EXPORTS, LIB, NAME = "brc_deflater", DEFLATE_EXPORTS, DEFLATE_LIB, "deflater"
    PROTOS = {"brc_deflate_bound": (C.c_size_t, [C.c_size_t]),
              "brc_deflate_bgzf": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
              "brc_deflate_eof_block": (C.c_void_p, [C.POINTER(C.c_size_t)])}

    def bound(self, n):
        return int(self.lib.brc_deflate_bound(n))

    def eof_block(self):
        n = C.c_size_t()
        p = self.lib.brc_deflate_eof_block(C.byref(n))
        return C.string_at(p, n.value)

    def deflate_raw(self, src, dst_cap=None, handle=True):
        """brc_deflate_bgzf as it is: (rc, bytes of dst, members).  dst_cap None: the bound.  dst is pre-filled with 0xA5 (what a
        refused call must leave untouched).  handle False: a NULL handle."""
        if isinstance(src, np.ndarray):
            sbuf = src if src.size else np.zeros(1, np.uint8); n_src = int(src.size)
        else:
            src = bytes(src); n_src = len(src)
            sbuf = np.frombuffer(src, np.uint8) if src else np.zeros(1, np.uint8)
        cap = self.bound(n_src) if dst_cap is None else dst_cap
        dst = np.full(max(cap, 1), 0xA5, np.uint8)
        got = C.c_size_t(0); nm = C.c_size_t(0)
        rc = self.lib.brc_deflate_bgzf(self.h if handle else None, sbuf.ctypes.data, n_src, dst.ctypes.data, cap, C.byref(got), C.byref(nm))
        if rc != 0:
            return rc, dst[:cap].tobytes(), 0
        return rc, dst[:got.value].tobytes(), nm.value

    def deflate(self, src):
        """Any bytes -> whole BGZF members back to back (no end-of-file member)."""
        rc, out, _ = self.deflate_raw(src)
        self._check("brc_deflate_bgzf", rc)
        return out


# ---------------------------------------------------------------- device-resident results (include/brc_dense.h)
DENSE_LIB = os.path.join(HERE, "csrc", "libbrc_dense_hip.so")
DENSE_EXPORTS = [
    "brc_dense_create", "brc_dense_destroy", "brc_dense_kind", "brc_dense_last_error", "brc_dense_expand", "brc_dense_last_timing",
]
NMETRIC = 13
M_NAMES = ["count", "avg_mapq", "avg_bq", "avg_se_mapq", "plus", "minus", "avg_pos", "avg_nm", "avg_mmq", "nq2", "avg_q2_dist",
           "avg_clipped", "avg_3p"]


class Dense(_Handle):
    """One handle of a library exporting include/brc_dense.h: the product's libbrc_dense_hip.so (default; raises when it is not built
    or there is no device — nothing falls back) or the CPU build of the same per-lane functions (tests/sim_dense).  expand() takes
    raw addresses; bam_readcount_amd.tensors.region() is the interface that allocates and returns arrays."""

    PREFIX, EXPORTS, LIB, NAME = "brc_dense", DENSE_EXPORTS, DENSE_LIB, "dense"
    PROTOS = {"brc_dense_expand": (C.c_int, [C.c_void_p, C.POINTER(DeviceView), C.c_int64, C.c_int64, C.c_int64] + [C.c_void_p] * 7)}

    def expand_raw(self, view, k0, n, dst_stride, ncol=None, depth=None, unavail=None, istat=None, fstat=None, metrics=None, stream=None):
        """brc_dense_expand as it is: destinations are addresses (or None) in memory of the view's kind; returns the code."""
        return self.lib.brc_dense_expand(self.h, _ref(view), k0, n, dst_stride, ncol, depth, unavail, istat, fstat, metrics, stream)

    def expand(self, view, k0, n, dst_stride, **kw):
        self._check("brc_dense_expand", self.expand_raw(view, k0, n, dst_stride, **kw))

    def last_timing(self):
        """kernel seconds (waits for the launches of the last expand), bytes read and written"""
        return super().last_timing()


# ---------------------------------------------------------------- the device-resident indel table (include/brc_indels.h)
INDELS_LIB = os.path.join(HERE, "csrc", "libbrc_indels_hip.so")
INDELS_EXPORTS = [
    "brc_indels_create", "brc_indels_destroy", "brc_indels_kind", "brc_indels_last_error", "brc_indels_workspace", "brc_indels_gather",
    "brc_indels_last_timing",
]
INDEL_DESTS = ("pos", "lib", "len", "rep_read", "rep_qpos", "istat", "fstat", "metrics", "allele_off", "alleles")


class Indels(_Handle):
    """One handle of a library exporting include/brc_indels.h: the product's libbrc_indels_hip.so (default; raises when it is not built
    or there is no device — nothing falls back) or the CPU build of the same per-lane functions (tests/sim_indels).  gather() takes
    raw addresses; bam_readcount_amd.tensors.indels() is the interface that allocates and returns arrays."""

    PREFIX, EXPORTS, LIB, NAME = "brc_indels", INDELS_EXPORTS, INDELS_LIB, "indels"
    PROTOS = {"brc_indels_workspace": (C.c_size_t, [C.POINTER(DeviceIndels), C.c_int64]),
              "brc_indels_gather": (C.c_int, [C.c_void_p, C.POINTER(DeviceIndels), C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int64, C.c_int64] +
                                    [C.c_void_p] * 11)}

    def workspace(self, view, n):
        """bytes of scratch a gather over n positions of the view needs"""
        return int(self.lib.brc_indels_workspace(_ref(view), n))

    def gather_raw(self, view, k0, n, workspace=None, workspace_bytes=0, counts=None, cap=0, alleles_cap=0, pos=None, lib=None, len=None,
                   rep_read=None, rep_qpos=None, istat=None, fstat=None, metrics=None, allele_off=None, alleles=None, stream=None):
        """brc_indels_gather as it is: scratch and destinations are addresses (or None) in memory of the view's kind; returns the code."""
        return self.lib.brc_indels_gather(self.h, _ref(view), k0, n, workspace, workspace_bytes, counts,
                                          cap, alleles_cap, pos, lib, len, rep_read, rep_qpos, istat, fstat, metrics, allele_off, alleles, stream)

    def gather(self, view, k0, n, **kw):
        self._check("brc_indels_gather", self.gather_raw(view, k0, n, **kw))

    def last_timing(self):
        """kernel seconds (waits for the launches of the last gather), bytes read and written"""
        return super().last_timing()


# ---------------------------------------------------------------- device-resident site panels (include/brc_panel.h)
PANEL_LIB = os.path.join(HERE, "csrc", "libbrc_panel_hip.so")
PANEL_EXPORTS = [
    "brc_panel_create", "brc_panel_destroy", "brc_panel_kind", "brc_panel_last_error", "brc_panel_gather", "brc_panel_last_timing",
]
PANEL_OUT_OF_RANGE, PANEL_NOT_ASCENDING = 1, 2
PANEL_DESTS = ("ncol", "depth", "unavail", "istat", "fstat", "metrics")


class Panel(_Handle):
    """One handle of a library exporting include/brc_panel.h: the product's libbrc_panel_hip.so (default; raises when it is not built
    or there is no device — nothing falls back) or the CPU build of the same per-lane functions (tests/sim_panel).  gather() takes
    raw addresses; bam_readcount_amd.tensors.sites() is the interface that allocates and returns arrays."""

    PREFIX, EXPORTS, LIB, NAME = "brc_panel", PANEL_EXPORTS, PANEL_LIB, "panel"
    PROTOS = {"brc_panel_gather": (C.c_int, [C.c_void_p, C.POINTER(DeviceView), C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 8)}

    def gather_raw(self, view, idx, n, dst_stride, ncol=None, depth=None, unavail=None, istat=None, fstat=None, metrics=None, status=None,
                   stream=None):
        """brc_panel_gather as it is: the list, the destinations and the status word are addresses (or None) in memory of the view's
        kind; returns the code."""
        return self.lib.brc_panel_gather(self.h, _ref(view), idx, n, dst_stride,
                                         ncol, depth, unavail, istat, fstat, metrics, status, stream)

    def gather(self, view, idx, n, dst_stride, **kw):
        self._check("brc_panel_gather", self.gather_raw(view, idx, n, dst_stride, **kw))

    def last_timing(self):
        """kernel seconds (waits for the launches of the last gather), bytes asked for and written"""
        return super().last_timing()


# ---------------------------------------------------------------- device-side site selection (include/brc_select.h)
SELECT_LIB = os.path.join(HERE, "csrc", "libbrc_select_hip.so")
SELECT_EXPORTS = [
    "brc_select_create", "brc_select_destroy", "brc_select_kind", "brc_select_last_error", "brc_select_workspace", "brc_select_sites",
    "brc_select_last_timing",
]
SELECT_SNV, SELECT_INDEL = 1, 2
ROLE_IGNORE, ROLE_CASE, ROLE_CONTROL = 0, 1, 2
SELECT_MAX_LIB = 254
WHY_A, WHY_C, WHY_G, WHY_T, WHY_INS, WHY_DEL = 1, 2, 4, 8, 16, 32


class SelectParams(C.Structure):
    """brc_select_params (include/brc_select.h)"""
    _fields_ = [("role", C.c_void_p), ("flags", C.c_uint32), ("min_depth", C.c_uint32), ("min_alt", C.c_uint32), ("frac_num", C.c_uint32),
                ("frac_den", C.c_uint32), ("ctl_min_depth", C.c_uint32), ("ctl_max_alt", C.c_uint32), ("ctl_frac_num", C.c_uint32),
                ("ctl_frac_den", C.c_uint32)]


def select_params(role=None, flags=SELECT_SNV | SELECT_INDEL, min_depth=0, min_alt=1, frac=(0, 1), ctl_min_depth=0, ctl_max_alt=2 ** 32 - 1,
                  ctl_frac=(1, 1)):
    """(SelectParams, keepalive): role is a sequence of ROLE_* per library, or None (every library a case library)"""
    p = SelectParams(None, flags, min_depth, min_alt, frac[0], frac[1], ctl_min_depth, ctl_max_alt, ctl_frac[0], ctl_frac[1])
    keep = None
    if role is not None:
        keep = np.ascontiguousarray(role, np.uint8)
        p.role = keep.ctypes.data
    return p, keep


class Select(_Handle):
    """One handle of a library exporting include/brc_select.h: the product's libbrc_select_hip.so (default; raises when it is not built
    or there is no device — nothing falls back) or the CPU build of the same per-lane functions (tests/sim_select).  sites() takes
    raw addresses; bam_readcount_amd.tensors.select() is the interface that allocates and returns arrays."""

    PREFIX, EXPORTS, LIB, NAME = "brc_select", SELECT_EXPORTS, SELECT_LIB, "select"
    PROTOS = {"brc_select_workspace": (C.c_int64, [C.POINTER(DeviceView), C.POINTER(DeviceIndels), C.c_int64]),
              "brc_select_sites": (C.c_int, [C.c_void_p, C.POINTER(DeviceView), C.POINTER(DeviceIndels), C.POINTER(SelectParams), C.c_int64, C.c_int64, C.c_int64] +
                                   [C.c_void_p] * 5)}

    def workspace(self, view, indels, n):
        """bytes of scratch a selection over n positions of the views needs"""
        return int(self.lib.brc_select_workspace(_ref(view), _ref(indels), n))

    def sites_raw(self, view, indels, params, k0, n, cap=0, idx=None, why=None, counts=None, workspace=None, stream=None):
        """brc_select_sites as it is: scratch and destinations are addresses (or None) in memory of the views' kind; returns the code."""
        return self.lib.brc_select_sites(self.h, _ref(view), _ref(indels), _ref(params), k0, n, cap, idx, why, counts, workspace, stream)

    def sites(self, view, indels, params, k0, n, **kw):
        self._check("brc_select_sites", self.sites_raw(view, indels, params, k0, n, **kw))

    def last_timing(self):
        """kernel seconds (waits for the launches of the last selection), bytes asked for and scratch bytes written"""
        return super().last_timing()


# ---------------------------------------------------------------- device-side window summaries (include/brc_bins.h)
BINS_LIB = os.path.join(HERE, "csrc", "libbrc_bins_hip.so")
BINS_EXPORTS = [
    "brc_bins_create", "brc_bins_destroy", "brc_bins_kind", "brc_bins_last_error", "brc_bins_reduce", "brc_bins_last_timing",
]
BINS_NSUM, BINS_MAX_THR, BINS_MAX_HIST, BINS_MAX_LIB = 12, 8, 4096, 65535
BINS_S_DEPTH, BINS_S_NCOL, BINS_S_BUCKET, BINS_S_NONREF, BINS_S_INS, BINS_S_DEL, BINS_S_MAXDEPTH = 0, 1, 2, 8, 9, 10, 11
BINS_DESCENDS, BINS_OUTSIDE = 1, 2


class BinsParams(C.Structure):
    """brc_bins_params (include/brc_bins.h)"""
    _fields_ = [("edges", C.c_void_p), ("width", C.c_int64), ("n_bins", C.c_int64), ("n_thr", C.c_int32), ("n_hist", C.c_int32),
                ("thr", C.c_uint32 * BINS_MAX_THR)]


def bins_params(width=0, edges=None, n_bins=0, thresholds=(), n_hist=0):
    """BinsParams: uniform bins of `width` positions, or an edge list — the ADDRESS of n_bins + 1 int32 plane indices in the views' kind
    of memory (the caller keeps them alive)"""
    p = BinsParams(edges, width, n_bins, len(thresholds), n_hist)
    for t, x in enumerate(thresholds[:BINS_MAX_THR]):
        p.thr[t] = x
    return p


class Bins(_Handle):
    """One handle of a library exporting include/brc_bins.h: the product's libbrc_bins_hip.so (default; raises when it is not built or
    there is no device — nothing falls back) or the CPU build of the same per-lane functions (tests/sim_bins).  reduce() takes raw
    addresses; bam_readcount_amd.tensors.bins() is the interface that allocates and returns arrays."""

    PREFIX, EXPORTS, LIB, NAME = "brc_bins", BINS_EXPORTS, BINS_LIB, "bins"
    PROTOS = {"brc_bins_reduce": (C.c_int, [C.c_void_p, C.POINTER(DeviceView), C.POINTER(DeviceIndels), C.POINTER(BinsParams), C.c_int64, C.c_int64] +
                                  [C.c_void_p] * 3 + [C.c_int64, C.c_void_p, C.c_void_p])}

    def reduce_raw(self, view, indels, params, k0, n, dst_stride, sums=None, covered=None, hist=None, status=None, stream=None):
        """brc_bins_reduce as it is: destinations and the status word are addresses (or None) in memory of the views' kind; returns the
        code."""
        return self.lib.brc_bins_reduce(self.h, _ref(view), _ref(indels), _ref(params), k0, n, sums, covered, hist, dst_stride, status, stream)

    def reduce(self, view, indels, params, k0, n, dst_stride, **kw):
        self._check("brc_bins_reduce", self.reduce_raw(view, indels, params, k0, n, dst_stride, **kw))

    def last_timing(self):
        """kernel seconds (waits for the launches of the last reduction), bytes asked for and destination bytes cleared"""
        return super().last_timing()


# ---------------------------------------------------------------- device-side depth-class intervals (include/brc_runs.h)
RUNS_LIB = os.path.join(HERE, "csrc", "libbrc_runs_hip.so")
RUNS_EXPORTS = [
    "brc_runs_create", "brc_runs_destroy", "brc_runs_kind", "brc_runs_last_error", "brc_runs_workspace", "brc_runs_find", "brc_runs_last_timing",
]
RUNS_MAX_LIB, RUNS_MAX_CUT = 254, 15
RUNS_MIN, RUNS_MAX, RUNS_SUM = 0, 1, 2
RUNS_REF_N = 1


class RunsParams(C.Structure):
    """brc_runs_params (include/brc_runs.h)"""
    _fields_ = [("role", C.c_void_p), ("combine", C.c_uint32), ("n_cut", C.c_uint32), ("cut", C.c_uint32 * RUNS_MAX_CUT), ("keep", C.c_uint32),
                ("flags", C.c_uint32)]


def runs_params(cuts, combine=RUNS_MIN, role=None, keep=None, flags=0):
    """(RunsParams, keepalive): cuts is a sequence of depths (strictly ascending, 1 .. RUNS_MAX_CUT of them), role a sequence of 0 (ignored)
    / 1 (counted) per library or None (every library counts), keep the bit mask of the classes whose runs are written (None: every class
    the call can produce)"""
    cuts = list(cuts)
    p = RunsParams(None, combine, len(cuts))
    for i, x in enumerate(cuts[:RUNS_MAX_CUT]):
        p.cut[i] = x
    p.keep = (1 << (len(cuts) + (2 if flags & RUNS_REF_N else 1))) - 1 if keep is None else keep
    p.flags = flags
    keepalive = None
    if role is not None:
        keepalive = np.ascontiguousarray(role, np.uint8)
        p.role = keepalive.ctypes.data
    return p, keepalive


class Runs(_Handle):
    """One handle of a library exporting include/brc_runs.h: the product's libbrc_runs_hip.so (default; raises when it is not built or
    there is no device — nothing falls back) or the CPU build of the same per-lane functions (tests/sim_runs).  find() takes raw
    addresses; bam_readcount_amd.tensors.runs() is the interface that allocates and returns arrays."""

    PREFIX, EXPORTS, LIB, NAME = "brc_runs", RUNS_EXPORTS, RUNS_LIB, "runs"
    PROTOS = {"brc_runs_workspace": (C.c_int64, [C.c_int64]),
              "brc_runs_find": (C.c_int, [C.c_void_p, C.POINTER(DeviceView), C.POINTER(DeviceIndels), C.POINTER(RunsParams), C.c_int64, C.c_int64, C.c_int64] +
                                [C.c_void_p] * 7)}

    def workspace(self, n):
        """bytes of scratch a call over n positions needs"""
        return int(self.lib.brc_runs_workspace(n))

    def find_raw(self, view, indels, params, k0, n, cap=0, start=None, end=None, cls=None, counts=None, per_class=None, workspace=None, stream=None):
        """brc_runs_find as it is: scratch and destinations are addresses (or None) in memory of the view's kind; returns the code."""
        return self.lib.brc_runs_find(self.h, _ref(view), _ref(indels), _ref(params), k0, n, cap, start, end, cls, counts, per_class, workspace, stream)

    def find(self, view, indels, params, k0, n, **kw):
        self._check("brc_runs_find", self.find_raw(view, indels, params, k0, n, **kw))

    def last_timing(self):
        """kernel seconds (waits for the launches of the last call), bytes asked for and scratch bytes written"""
        return super().last_timing()


# ---------------------------------------------------------------- device-side candidate filter (include/brc_vet.h)
VET_LIB = os.path.join(HERE, "csrc", "libbrc_vet_hip.so")
VET_EXPORTS = [
    "brc_vet_create", "brc_vet_destroy", "brc_vet_kind", "brc_vet_last_error", "brc_vet_workspace", "brc_vet_sites", "brc_vet_last_timing",
]
VET_MAX_LIB, VET_NVAL = 254, 20
VET_TESTS = ("DEPTH", "VAR_COUNT", "VAR_FREQ", "STRAND", "VAR_READPOS", "VAR_DIST3", "VAR_BQ", "VAR_MAPQ", "VAR_MMQS", "VAR_RL", "REF_READPOS",
             "REF_DIST3", "REF_BQ", "REF_MAPQ", "REF_RL", "MMQS_DIFF", "MAPQ_DIFF", "RL_DIFF")          # bit i of a failure word is VET_TESTS[i]
VET_BIT = {name: 1 << i for i, name in enumerate(VET_TESTS)}
VET_ALL_TESTS = (1 << len(VET_TESTS)) - 1
VET_NOT_ASKED, VET_NO_SITE = 1 << 30, 1 << 31
VET_OUT_OF_RANGE, VET_NOT_ASCENDING = 1, 2
VET_V_NAMES = ("cv", "cr", "d", "freq", "strand", "mmqs_diff", "mapq_diff", "rl_diff", "var_readpos", "var_dist3", "var_bq", "var_mapq", "var_mmqs",
               "var_rl", "ref_readpos", "ref_dist3", "ref_bq", "ref_mapq", "ref_mmqs", "ref_rl")         # the columns of vals
VET_UINTS = ("min_depth", "min_var_count", "freq_num", "freq_den", "min_strand_reads", "strand_num", "strand_den", "min_ref_reads")
VET_FLOATS = ("min_var_readpos", "min_var_dist3", "min_var_bq", "min_var_mapq", "max_var_mmqs", "min_var_rl", "min_ref_readpos", "min_ref_dist3",
              "min_ref_bq", "min_ref_mapq", "min_ref_rl", "max_mmqs_diff", "max_mapq_diff", "max_rl_diff")
VET_DEFAULTS = dict(min_depth=8, min_var_count=4, freq_num=1, freq_den=20, min_strand_reads=5, strand_num=1, strand_den=100, min_ref_reads=2,
                    min_var_readpos=0.1, min_var_dist3=0.1, min_var_bq=15.0, min_var_mapq=15.0, max_var_mmqs=100.0, min_var_rl=90.0,
                    min_ref_readpos=0.1, min_ref_dist3=0.1, min_ref_bq=15.0, min_ref_mapq=15.0, min_ref_rl=90.0, max_mmqs_diff=50.0,
                    max_mapq_diff=50.0, max_rl_diff=0.25)


class VetParams(C.Structure):
    """brc_vet_params (include/brc_vet.h)"""
    _fields_ = [("lib_on", C.c_void_p), ("tests", C.c_uint32)] + [(k, C.c_uint32) for k in VET_UINTS] + [(k, C.c_float) for k in VET_FLOATS]


def vet_params(lib_on=None, tests=VET_ALL_TESTS, **thresholds):
    """(VetParams, keepalive): lib_on is a sequence of 0 / 1 per library or None (every library is judged), tests a mask of VET_BIT values;
    thresholds are the members of brc_vet_params by name, VET_DEFAULTS where not given"""
    unknown = set(thresholds) - set(VET_DEFAULTS)
    if unknown:
        raise TypeError("unknown thresholds %r" % sorted(unknown))
    t = dict(VET_DEFAULTS, **thresholds)
    p = VetParams(None, tests, *[t[k] for k in VET_UINTS + VET_FLOATS])
    keepalive = None
    if lib_on is not None:
        keepalive = np.ascontiguousarray(lib_on, np.uint8)
        p.lib_on = keepalive.ctypes.data
    return p, keepalive


class Vet(_Handle):
    """One handle of a library exporting include/brc_vet.h: the product's libbrc_vet_hip.so (default; raises when it is not built or
    there is no device — nothing falls back) or the CPU build of the same per-lane functions (tests/sim_vet).  sites() takes raw
    addresses; bam_readcount_amd.tensors.vet() is the interface that allocates and returns arrays."""

    PREFIX, EXPORTS, LIB, NAME = "brc_vet", VET_EXPORTS, VET_LIB, "vet"
    PROTOS = {"brc_vet_workspace": (C.c_int64, [C.POINTER(DeviceView), C.c_int64]),
              "brc_vet_sites": (C.c_int, [C.c_void_p, C.POINTER(DeviceView), C.POINTER(DeviceIndels), C.POINTER(VetParams), C.c_void_p, C.c_void_p,
                                          C.c_int64, C.c_int64] + [C.c_void_p] * 6)}

    def workspace(self, view, n):
        """bytes of scratch a call over a list of n elements of the view needs"""
        return int(self.lib.brc_vet_workspace(_ref(view), n))

    def sites_raw(self, view, indels, params, idx, alt, n, dst_stride, fail=None, keep=None, vals=None, status=None, workspace=None, stream=None):
        """brc_vet_sites as it is: lists, scratch, destinations and the status word are addresses (or None) in memory of the views'
        kind; returns the code."""
        return self.lib.brc_vet_sites(self.h, _ref(view), _ref(indels), _ref(params), idx, alt, n, dst_stride, fail, keep, vals, status, workspace, stream)

    def sites(self, view, indels, params, idx, alt, n, dst_stride, **kw):
        self._check("brc_vet_sites", self.sites_raw(view, indels, params, idx, alt, n, dst_stride, **kw))

    def last_timing(self):
        """kernel seconds (waits for the launches of the last call), bytes asked for and written"""
        return super().last_timing()


# ---------------------------------------------------------------- device-side indel candidate filter (include/brc_ivet.h)
IVET_LIB = os.path.join(HERE, "csrc", "libbrc_ivet_hip.so")
IVET_EXPORTS = [
    "brc_ivet_create", "brc_ivet_destroy", "brc_ivet_kind", "brc_ivet_last_error", "brc_ivet_workspace", "brc_ivet_records", "brc_ivet_last_timing",
]
IVET_MAX_LIB, IVET_NVAL = 254, 20
IVET_TESTS = tuple(t for t in VET_TESTS if t != "VAR_BQ") + ("CTL_DEPTH", "CTL_ALLELE")
IVET_BIT = dict({t: VET_BIT[t] for t in VET_TESTS if t != "VAR_BQ"}, CTL_DEPTH=1 << 18, CTL_ALLELE=1 << 19)      # the shared tests keep brc_vet.h's bits
IVET_ALL_TESTS = sum(IVET_BIT.values())
IVET_NOT_ASKED, IVET_NO_SITE = VET_NOT_ASKED, VET_NO_SITE
IVET_LIST_OUT_OF_RANGE, IVET_LIST_NOT_ASCENDING, IVET_TABLE_OUT_OF_RANGE, IVET_TABLE_NOT_ASCENDING = 1, 2, 4, 8
IVET_UINTS = VET_UINTS + ("ctl_min_depth", "ctl_max_count", "ctl_frac_num", "ctl_frac_den")
IVET_FLOATS = tuple(k for k in VET_FLOATS if k != "min_var_bq")
IVET_DEFAULTS = dict({k: x for k, x in VET_DEFAULTS.items() if k != "min_var_bq"}, ctl_min_depth=0, ctl_max_count=0, ctl_frac_num=1, ctl_frac_den=1)


class IVetParams(C.Structure):
    """brc_ivet_params (include/brc_ivet.h)"""
    _fields_ = [("role", C.c_void_p), ("tests", C.c_uint32), ("kinds", C.c_uint32)] + [(k, C.c_uint32) for k in IVET_UINTS] + [(k, C.c_float) for k in IVET_FLOATS]


class IVetTable(C.Structure):
    """brc_ivet_table (include/brc_ivet.h): the table brc_indels_gather writes, where it lies"""
    _fields_ = [("m", C.c_int64), ("stride", C.c_int64), ("pos", C.c_void_p), ("lib", C.c_void_p), ("len", C.c_void_p), ("istat", C.c_void_p),
                ("fstat", C.c_void_p), ("allele_off", C.c_void_p), ("alleles", C.c_void_p), ("alleles_len", C.c_int64)]


def ivet_params(role=None, tests=IVET_ALL_TESTS, kinds=WHY_INS | WHY_DEL, **thresholds):
    """(IVetParams, keepalive): role is a sequence of ROLE_* per library or None (every library a case library), tests a mask of IVET_BIT
    values, kinds a mask of WHY_INS | WHY_DEL; thresholds are the members of brc_ivet_params by name, IVET_DEFAULTS where not given"""
    unknown = set(thresholds) - set(IVET_DEFAULTS)
    if unknown:
        raise TypeError("unknown thresholds %r" % sorted(unknown))
    t = dict(IVET_DEFAULTS, **thresholds)
    p = IVetParams(None, tests, kinds, *[t[k] for k in IVET_UINTS + IVET_FLOATS])
    keepalive = None
    if role is not None:
        keepalive = np.ascontiguousarray(role, np.uint8)
        p.role = keepalive.ctypes.data
    return p, keepalive


class IVet(_Handle):
    """One handle of a library exporting include/brc_ivet.h: the product's libbrc_ivet_hip.so (default; raises when it is not built or
    there is no device — nothing falls back) or the CPU build of the same per-lane functions (tests/sim_ivet).  records() takes raw
    addresses; bam_readcount_amd.tensors.vet_indels() is the interface that allocates and returns arrays."""

    PREFIX, EXPORTS, LIB, NAME = "brc_ivet", IVET_EXPORTS, IVET_LIB, "ivet"
    PROTOS = {"brc_ivet_workspace": (C.c_int64, [C.POINTER(DeviceView), C.c_int64]),
              "brc_ivet_records": (C.c_int, [C.c_void_p, C.POINTER(DeviceView), C.POINTER(DeviceIndels), C.POINTER(IVetParams), C.POINTER(IVetTable),
                                             C.c_void_p, C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 7)}

    def workspace(self, view, m):
        """bytes of scratch a call over a table of m records needs"""
        return int(self.lib.brc_ivet_workspace(_ref(view), m))

    def records_raw(self, view, indels, params, table, idx, why, n, dst_stride, fail=None, vals=None, ctl_count=None, keep=None, status=None,
                    workspace=None, stream=None):
        """brc_ivet_records as it is: table arrays, lists, scratch, destinations and the status word are addresses (or None) in memory of
        the views' kind; returns the code."""
        return self.lib.brc_ivet_records(self.h, _ref(view), _ref(indels), _ref(params), _ref(table), idx, why, n, dst_stride, fail, vals, ctl_count, keep,
                                         status, workspace, stream)

    def records(self, view, indels, params, table, idx, why, n, dst_stride, **kw):
        self._check("brc_ivet_records", self.records_raw(view, indels, params, table, idx, why, n, dst_stride, **kw))

    def last_timing(self):
        """kernel seconds (waits for the launches of the last call), bytes asked for and written"""
        return super().last_timing()


# ---------------------------------------------------------------- device-side indel normalisation (include/brc_inorm.h)
INORM_LIB = os.path.join(HERE, "csrc", "libbrc_inorm_hip.so")
INORM_EXPORTS = [
    "brc_inorm_create", "brc_inorm_destroy", "brc_inorm_kind", "brc_inorm_last_error", "brc_inorm_workspace", "brc_inorm_table", "brc_inorm_last_timing",
]
INORM_MAX_SHIFT = 1 << 20
INORM_NOT_JUDGED, INORM_LIMIT, INORM_EDGE = 1, 2, 4                 # bits of a record's flags
INORM_TABLE_BAD, INORM_ANY_LIMIT, INORM_ANY_EDGE = 1, 2, 4          # bits of the status word
INORM_SRC_DESTS = ("npos", "shift", "flags", "group")
INORM_DESTS = ("pos", "lib", "len", "rep_read", "rep_qpos", "members", "istat", "fstat", "metrics", "allele_off", "alleles")


class INormParams(C.Structure):
    """brc_inorm_params (include/brc_inorm.h)"""
    _fields_ = [("max_shift", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class INormSource(C.Structure):
    """brc_inorm_source (include/brc_inorm.h): the input table, where it lies"""
    _fields_ = [("m", C.c_int64), ("stride", C.c_int64), ("pos", C.c_void_p), ("lib", C.c_void_p), ("len", C.c_void_p), ("rep_read", C.c_void_p),
                ("rep_qpos", C.c_void_p), ("istat", C.c_void_p), ("fstat", C.c_void_p), ("allele_off", C.c_void_p), ("alleles", C.c_void_p),
                ("alleles_len", C.c_int64)]


class INorm(_Handle):
    """One handle of a library exporting include/brc_inorm.h: the product's libbrc_inorm_hip.so (default; raises when it is not built or
    there is no device — nothing falls back) or the CPU build of the same per-lane functions (tests/sim_inorm).  table() takes raw
    addresses; bam_readcount_amd.tensors.normalize_indels() is the interface that allocates and returns arrays."""

    PREFIX, EXPORTS, LIB, NAME = "brc_inorm", INORM_EXPORTS, INORM_LIB, "inorm"
    PROTOS = {"brc_inorm_workspace": (C.c_size_t, [C.c_int64, C.c_int64]),
              "brc_inorm_table": (C.c_int, [C.c_void_p, C.POINTER(DeviceIndels), C.POINTER(INormParams), C.POINTER(INormSource), C.c_int64, C.c_int64,
                                            C.c_void_p, C.c_size_t] + [C.c_void_p] * 5 + [C.c_int64, C.c_int64] + [C.c_void_p] * 13)}

    def workspace(self, n, m):
        """bytes of scratch a call over a window of n positions and a table of m records needs"""
        return int(self.lib.brc_inorm_workspace(n, m))

    def table_raw(self, indels, params, source, k0, n, workspace=None, workspace_bytes=0, counts=None, npos=None, shift=None, flags=None, group=None,
                  cap=0, alleles_cap=0, pos=None, lib=None, len=None, rep_read=None, rep_qpos=None, members=None, istat=None, fstat=None, metrics=None,
                  allele_off=None, alleles=None, status=None, stream=None):
        """brc_inorm_table as it is: table arrays, scratch, destinations and the status word are addresses (or None) in memory of the
        view's kind; returns the code."""
        return self.lib.brc_inorm_table(self.h, _ref(indels), _ref(params), _ref(source), k0, n, workspace, workspace_bytes, counts, npos, shift, flags,
                                        group, cap, alleles_cap, pos, lib, len, rep_read, rep_qpos, members, istat, fstat, metrics, allele_off, alleles,
                                        status, stream)

    def table(self, indels, params, source, k0, n, **kw):
        self._check("brc_inorm_table", self.table_raw(indels, params, source, k0, n, **kw))

    def last_timing(self):
        """kernel seconds (waits for the launches of the last call), bytes asked for and written"""
        return super().last_timing()


# ---------------------------------------------------------------- device-side join of computed regions (include/brc_join.h)
JOIN_LIB = os.path.join(HERE, "csrc", "libbrc_join_hip.so")
JOIN_EXPORTS = [
    "brc_join_create", "brc_join_destroy", "brc_join_kind", "brc_join_last_error", "brc_join_workspace", "brc_join_sizes_of", "brc_join_views",
    "brc_join_last_timing",
]
JOIN_MAX_SOURCES, JOIN_MAX_LIB = 16, 254
JOIN_REF_DIFFERS = 1                                                # bit of the status word
JOIN_DESTS = ("ncol", "depth", "slotid", "si", "sf", "xagg", "slots", "seq_off", "l_qseq", "seq4", "ref")


class JoinSource(C.Structure):
    """brc_join_source (include/brc_join.h): the two views of one engine"""
    _fields_ = [("view", C.POINTER(DeviceView)), ("indels", C.POINTER(DeviceIndels))]


class JoinDest(C.Structure):
    """brc_join_dest (include/brc_join.h): the caller's destination buffers"""
    _fields_ = [(k, C.c_void_p) for k in JOIN_DESTS]


class JoinSizes(C.Structure):
    """brc_join_sizes (include/brc_join.h): what the host knows of a join before it runs"""
    _fields_ = [("n_lib", C.c_int32), ("has_ref", C.c_int32), ("n_xagg", C.c_uint64), ("n_slots", C.c_uint64), ("ref_lo", C.c_int64), ("ref_hi", C.c_int64),
                ("ref_len", C.c_int64)] + [(k + "_bytes", C.c_uint64) for k in JOIN_DESTS if k != "seq4"] + [("workspace_bytes", C.c_uint64)]


def join_sources(pairs):
    """[(DeviceView, DeviceIndels | None)] -> a JoinSource array (it holds on to the structs it points to)"""
    arr = (JoinSource * len(pairs))()
    for s, (v, d) in enumerate(pairs):
        arr[s].view = C.pointer(v)
        if d is not None:
            arr[s].indels = C.pointer(d)
    arr._keep = list(pairs)
    return arr


class Join(_Handle):
    """One handle of a library exporting include/brc_join.h: the product's libbrc_join_hip.so (default; raises when it is not built or
    there is no device — nothing falls back) or the CPU build of the same per-lane functions (tests/sim_join).  views() takes raw
    addresses; bam_readcount_amd.tensors.join() is the interface that allocates and returns an engine-like object."""

    PREFIX, EXPORTS, LIB, NAME = "brc_join", JOIN_EXPORTS, JOIN_LIB, "join"
    PROTOS = {"brc_join_workspace": (C.c_size_t, [C.c_uint64]),
              "brc_join_sizes_of": (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.POINTER(JoinSizes)]),
              "brc_join_views": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.POINTER(JoinDest), C.POINTER(DeviceView),
                                           C.POINTER(DeviceIndels), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p])}

    def workspace(self, n_slots):
        """bytes of scratch a join with n_slots joined indel records needs"""
        return int(self.lib.brc_join_workspace(n_slots))

    def sizes_raw(self, sources, pos0, n_pos, stride):
        """brc_join_sizes_of as it is -> (the code, JoinSizes); sources: a JoinSource array (join_sources) or None"""
        z = JoinSizes()
        return self.lib.brc_join_sizes_of(len(sources) if sources is not None else 0, sources, pos0, n_pos, stride, C.byref(z)), z

    def sizes(self, sources, pos0, n_pos, stride):
        rc, z = self.sizes_raw(sources, pos0, n_pos, stride)
        if rc != 0:
            raise BrcError("brc_join_sizes_of: %d" % rc)
        return z

    def views_raw(self, sources, pos0, n_pos, stride, dest=None, out_view=None, out_indels=None, counts=None, seq_cap=0, status=None, workspace=None,
                  workspace_bytes=0, stream=None, K=None):
        """brc_join_views as it is: dest a JoinDest of addresses (or None: the counts alone), out_view / out_indels the host structs it
        fills in (or None), counts, status and workspace addresses in memory of the views' kind; returns the code."""
        K = (len(sources) if sources is not None else 0) if K is None else K
        return self.lib.brc_join_views(self.h, K, sources, pos0, n_pos, stride, _ref(dest), _ref(out_view), _ref(out_indels), counts, seq_cap, status,
                                       workspace, workspace_bytes, stream)

    def views(self, sources, pos0, n_pos, stride, **kw):
        self._check("brc_join_views", self.views_raw(sources, pos0, n_pos, stride, **kw))

    def last_timing(self):
        """kernel seconds (waits for the launches of the last call), bytes read and written"""
        return super().last_timing()
