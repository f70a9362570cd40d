"""Results of a computed region as arrays in the memory where the engine left them.

    from bam_readcount_amd import capi, tensors
    eng = capi.Engine(capi.load_product(), ...); dense = capi.Dense()
    eng.begin_region(...); eng.push_reads(...); eng.upload(); eng.compute()
    r = tensors.region(eng, dense)            # torch tensors on the engine's GPU; nothing crossed PCIe
    af = r["istat"][:, 1:5, 0] / r["depth"][:, None].clamp(min=1)      # allele fractions of A C G T, on the device

With the HIP libraries the arrays are `torch` tensors on the engine's device, filled by the gfx950 kernels of libbrc_dense_hip.so on
torch's current stream: torch work queued on that stream afterwards sees them, no host synchronisation in between.  With the CPU
builds of the tests (libbrc_sim.so + libbrc_dense_sim.so) the same call returns numpy arrays.  torch is imported only when a
device view is expanded: importing the package, and the CPU route, need numpy alone.  It may be imported before or after the
engine is created: the binding keeps the process at one HIP runtime, torch's (capi._load).

Lifetime: region() reads the engine's buffers of the LAST compute.  With the HIP libraries it returns as soon as the kernels are
queued, so the next begin_region / upload / close of that engine must not start before they have run — synchronise the stream
(or use the results on the host, which does) first.  The returned arrays are the caller's and stay valid.

Indel buckets are not part of these arrays; engine.fetch_result() returns them (on a text_only engine without any planes).
"""
import numpy as np

from . import capi

KINDS = ("istat", "fstat", "metrics", "depth", "ncol", "unavail")
DEFAULT_WANT = ("istat", "fstat", "metrics", "depth", "ncol")


def shapes(n_lib, n):
    """kind -> (shape, numpy dtype) of a window of n positions: no padding, the last axis is the position"""
    return {"ncol": ((n_lib, n), np.uint32), "depth": ((n_lib, n), np.uint32), "unavail": ((n,), np.uint32),
            "istat": ((n_lib, capi.NBUCKET, capi.NI, n), np.uint32), "fstat": ((n_lib, capi.NBUCKET, capi.NF, n), np.float32),
            "metrics": ((n_lib, capi.NBUCKET, capi.NMETRIC, n), np.float32)}


def region(engine, dense, beg0=None, end=None, want=DEFAULT_WANT, out=None):
    """The reference positions [beg0, end) of the engine's last computed region, clipped to its planes (None: from the first /
    to the last plane position; the planes start at the region's lead position beg0 - 1, see include/brc.h: brc_result).

    Returns a dict: every kind in `want` (KINDS) -> an array shaped as in shapes(), uint32 / float32 as in brc_result (torch.uint32
    tensors: convert with .to(torch.int64), or reinterpret with .view(torch.int32), for operators torch lacks on unsigned types),
    plus the ints "pos0" (the region's first plane position), "first" (the reference position of element 0 of every array), "n"
    and "n_lib".
    out: a dict of arrays to fill instead of allocating (same shapes, dtypes, device; contiguous).
    """
    want = tuple(want)
    for k in want:
        if k not in KINDS:
            raise ValueError("unknown kind %r (one of %r)" % (k, KINDS))
    v = engine.device_view()
    P, pos0, L = int(v.n_pos), int(v.pos0), int(v.n_lib)
    lo = pos0 if beg0 is None else max(int(beg0), pos0)
    hi = pos0 + P if end is None else min(int(end), pos0 + P)
    lo = min(lo, pos0 + P)
    n = max(hi - lo, 0)
    k0 = lo - pos0 if n else 0
    res = {"pos0": pos0, "first": pos0 + k0, "n": n, "n_lib": L}
    shp = shapes(L, n)
    if v.memory == capi.MEM_HOST:
        arrays, ptr, stream = _host_arrays(shp, want, out), (lambda a: a.ctypes.data), None
    elif v.memory == capi.MEM_DEVICE:
        arrays, ptr, stream = _torch_arrays(shp, want, out, int(v.device))
    else:
        raise capi.BrcError("brc_device_view of unknown memory kind %d" % v.memory)
    if n and want:
        dense.expand(v, k0, n, n, stream=stream, **{k: ptr(arrays[k]) for k in want})
    res.update(arrays)
    return res


def _check_out(a, shape, what):
    if tuple(a.shape) != tuple(shape):
        raise ValueError("out[%r] has shape %r, wanted %r" % (what, tuple(a.shape), tuple(shape)))


def _host_arrays(shp, want, out):
    arrays = {}
    for k in want:
        shape, dt = shp[k]
        if out is not None and k in out:
            a = out[k]
            _check_out(a, shape, k)
            if not isinstance(a, np.ndarray) or a.dtype != dt or not a.flags["C_CONTIGUOUS"] or not a.flags["WRITEABLE"]:
                raise ValueError("out[%r] must be a writable C-contiguous numpy array of %s" % (k, np.dtype(dt).name))
        else:
            a = np.empty(shape, dt)
        arrays[k] = a
    return arrays


def _torch_arrays(shp, want, out, device):
    import torch          # (lazily: the package and its CPU route work without torch)
    dev = torch.device("cuda", device)
    tdt = {np.uint32: torch.uint32, np.float32: torch.float32}
    arrays = {}
    for k in want:
        shape, dt = shp[k]
        if out is not None and k in out:
            a = out[k]
            _check_out(a, shape, k)
            if not isinstance(a, torch.Tensor) or a.dtype != tdt[dt] or a.device != dev or not a.is_contiguous():
                raise ValueError("out[%r] must be a contiguous %s tensor on %s" % (k, tdt[dt], dev))
        else:
            a = torch.empty(shape, dtype=tdt[dt], device=dev)
        arrays[k] = a
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
    return arrays, (lambda a: a.data_ptr()), stream
