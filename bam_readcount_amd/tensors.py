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

Indel buckets are not part of region()'s arrays: indels() below returns them as a sorted table, in the same memory.

A site list — positions scattered over planes that are otherwise EMPTY (Engine.region_windows) — is served by sites(): the listed
positions alone, gathered by libbrc_panel_hip.so (capi.Panel) in one call, in the same memory.

The positions worth listing can be picked on the device too: select() returns those with non-reference evidence (a base, an insertion,
a deletion) in "case" libraries and none in "control" libraries, found by libbrc_select_hip.so (capi.Select) over the compact planes:
    sel = tensors.select(eng, select, case=["tumor"], control=["normal"], min_depth=10, min_alt=3, min_frac=(1, 20), ctl_max_alt=0)
    panel = tensors.sites(eng, capi.Panel(), positions=sel["pos"])

Per-window questions — depth, coverage at thresholds, allele and indel load per bin and library, a depth histogram — are answered by
bins(): exact integer sums over uniform bins or an edge list, reduced by libbrc_bins_hip.so (capi.Bins) without a synchronisation:
    cov = tensors.bins(eng, capi.Bins(), width=1000, thresholds=(10, 20, 30), hist=256)

Where the stretches are — the maximal intervals over which coverage stays in one class: callable in every library, below 10x in the
normal, no coverage, reference is N — is answered by runs(): an ascending list of intervals with a class each, found by
libbrc_runs_hip.so (capi.Runs) over the depth planes; its starts and ends are edges for bins() and masks for select()'s list:
    ok = tensors.runs(eng, capi.Runs(), cuts=(10,), combine="min", keep=(1,), ref_n=True)       # >= 10x in every library, reference known

Between "candidate" and "call" sit the per-allele read-metric tests that false-positive filters run on the thirteen columns — variant
bucket against reference bucket of the same site.  vet() runs them on a list where it lies, by libbrc_vet_hip.so (capi.Vet), with no
synchronisation: select -> vet -> sites is a chain of device lists:
    r = tensors.vet(eng, capi.Vet(), idx=sel["idx"], alt=sel["why"], min_var_count=4, min_var_mapq=20.0)
    panel = tensors.sites(eng, capi.Panel(), positions=sel["pos"][r["keep"].nonzero()[:, 0]])

Indel candidates are judged on the records of the indel table: vet_indels() runs the same tests on every record — its own sums against
the reference base's bucket at its position — and an allele-aware control veto (a control library's record of the same position,
length and text), by libbrc_ivet_hip.so (capi.IVet), with no synchronisation.  select()'s own control veto does not compare allele
text, so it runs with the control libraries ignored:
    sel = tensors.select(eng, select, role=[1, 0], snv=False, min_depth=8, min_alt=3)
    r = tensors.vet_indels(eng, capi.IVet(), tensors.indels(eng, capi.Indels()), idx=sel["idx"], why=sel["why"], role=[1, 2])
An aligner may place one indel anywhere inside a repeat: normalize_indels() left-aligns the table and merges what became equal first:
    norm = tensors.normalize_indels(eng, capi.INorm(), tensors.indels(eng, lib)); r = tensors.vet_indels(eng, ivet, norm, role=[1, 2])

A tumour and its normal are usually two files, hence two engines: join() copies the computed regions of several engines into ONE
engine-like object — the libraries of the second behind those of the first — that every function above takes in an engine's place,
by libbrc_join_hip.so (capi.Join):
    both = tensors.join([tumour_eng, normal_eng], capi.Join(), names=["tumour", "normal"])
    sel = tensors.select(both, select, case=["tumour"], control=["normal"], min_depth=10, min_alt=3)

A region becomes a SEQUENCE with consensus(): one call per position from the pooled counts of A C G T and of the reads that carry a
deletion across it (which only the indel table knows), accepted insertions behind their anchors, and the offset of every reference
position in the sequence, by libbrc_cons_hip.so (consensus.Cons):
    c = tensors.consensus(eng, consensus.Cons(), table=tensors.normalize_indels(eng, inorm, tensors.indels(eng, lib)), min_depth=4)
"""
from functools import lru_cache, partial

import numpy as np

from . import capi
from . import consensus as cons_api


# ------------------------------------------------------------------------------------------------ the memory the results lie in

def _is_torch(x):
    return type(x).__module__.split(".")[0] == "torch"


class _Host:
    """Results in host memory (the CPU builds): numpy arrays, no stream, no torch."""
    torch = stream = None

    def empty(self, shape, dt):
        return np.empty(shape, dt)

    def zeros(self, shape, dt):
        return np.zeros(shape, dt)

    def arange(self, n, dt):
        return np.arange(n, dtype=dt)

    def ptr(self, a, null_if_empty=False):
        return None if null_if_empty and not a.size else a.ctypes.data

    def upload(self, a):
        return a

    def read(self, a):
        return a.tolist()

    def offset(self, a, k):
        return a + a.dtype.type(k)            # (the sum keeps the array's dtype)

    def holds(self, x, kind):
        if _is_torch(x):
            raise ValueError("a torch tensor of %s needs an engine whose results lie on a GPU" % kind)
        return False

    def check_out(self, a, k, dt):
        if not isinstance(a, np.ndarray) or a.dtype != dt or not a.flags["C_CONTIGUOUS"] or not a.flags["WRITEABLE"]:
            raise ValueError("out[%r] must be a writable C-contiguous numpy array of %s" % (k, np.dtype(dt).name))


@lru_cache(None)
def _torch_dtypes(torch):
    """THE dtype table: (numpy dtype -> torch dtype, unsigned numpy dtype -> the signed twin it is made as)"""
    return ({np.int32: torch.int32, np.uint32: torch.uint32, np.int64: torch.int64, np.uint64: torch.uint64, np.float32: torch.float32,
             np.uint8: torch.uint8}, {np.uint32: torch.int32, np.uint64: torch.int64})


class _Device:
    """Results on cuda:<device> (the HIP libraries): torch tensors, work on torch's current stream of that device.  The one place
    that imports torch, when a device view is met, and the one place that can make the host wait: read()."""

    def __init__(self, device):
        import torch          # (lazily: the package and its CPU route work without torch)
        self.torch = torch
        self.dtype, self.signed = _torch_dtypes(torch)
        self.dev = torch.device("cuda", device)
        self.stream = torch.cuda.current_stream(self.dev).cuda_stream

    def _new(self, make, shape, dt):          # (unsigned 32- and 64-bit tensors: made as their signed twins and viewed, which every torch accepts)
        if dt in self.signed:
            return make(shape, dtype=self.signed[dt], device=self.dev).view(self.dtype[dt])
        return make(shape, dtype=self.dtype[dt], device=self.dev)

    def empty(self, shape, dt):
        return self._new(self.torch.empty, shape, dt)

    def zeros(self, shape, dt):
        return self._new(self.torch.zeros, shape, dt)

    def arange(self, n, dt):
        return self.torch.arange(n, dtype=self.dtype[dt], device=self.dev)

    def ptr(self, a, null_if_empty=False):
        return None if null_if_empty and not a.numel() else a.data_ptr()

    def upload(self, a):
        """a host array -> a tensor on the device: one copy from pageable memory, which may wait for the stream"""
        return self.torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(self.dev)

    def read(self, a):
        """THE WAIT: the host reads device memory — count-then-fill (_sized_by_data) calls this once, nothing else does"""
        return [a.item()] if a.numel() == 1 else a.cpu().tolist()

    def offset(self, a, k):
        return a + k

    def holds(self, x, kind):
        return _is_torch(x)

    def check_list(self, a, what, words, dtypes=(np.int32,), n=None):
        if a.dtype not in [self.dtype[d] for d in dtypes] or a.device != self.dev or a.dim() != 1 or not a.is_contiguous() or n not in (None, int(a.numel())):
            raise ValueError("%s must be a contiguous one-dimensional %s on %s" % (what, words, self.dev))

    def check_out(self, a, k, dt):
        if not isinstance(a, self.torch.Tensor) or a.dtype != self.dtype[dt] or a.device != self.dev or not a.is_contiguous():
            raise ValueError("out[%r] must be a contiguous %s tensor on %s" % (k, self.dtype[dt], self.dev))


def _memory(view, what="brc_device_view"):
    """the flavour of the memory a view's results lie in"""
    if view.memory == capi.MEM_HOST:
        return _Host()
    if view.memory == capi.MEM_DEVICE:
        return _Device(int(view.device))
    raise capi.BrcError("%s of unknown memory kind %d" % (what, view.memory))


def _window(view, beg0, end):
    """[beg0, end) clipped to the view's positions (None: from the first / to the last) -> (k0, n): n positions from plane index k0 on"""
    P, pos0 = int(view.n_pos), int(view.pos0)
    lo = pos0 if beg0 is None else max(int(beg0), pos0)
    hi = pos0 + P if end is None else min(int(end), pos0 + P)
    lo = min(lo, pos0 + P)
    n = max(hi - lo, 0)
    return (lo - pos0 if n else 0), n


def _check_want(want, kinds):
    want = tuple(want)
    for k in want:
        if k not in kinds:
            raise ValueError("unknown kind %r (one of %r)" % (k, kinds))
    return want


def _arrays(mem, shp, want, out=None):
    """kind -> the array of shp[kind] = (shape, numpy dtype) for every kind in want: the caller's out[kind], validated, or a new one"""
    arrays = {}
    for k in want:
        shape, dt = shp[k]
        if out is not None and k in out:
            a = out[k]
            if tuple(a.shape) != tuple(shape):
                raise ValueError("out[%r] has shape %r, wanted %r" % (k, tuple(a.shape), tuple(shape)))
            mem.check_out(a, k, dt)
        else:
            a = mem.empty(shape, dt)
        arrays[k] = a
    return arrays


def _ptrs(mem, arrays, **kw):
    return {k: mem.ptr(a, **kw) for k, a in arrays.items()}


def _scratch(mem, n_bytes):
    return mem.empty(max(n_bytes // 4, 1), np.int32)


def _listed(mem, x, kind, noun, place, lo, hi, closed=False, parse=None):
    """A caller's ascending list (kind: "positions", "indices", "edges"), where it lies.  A torch tensor stays where it is -> (True,
    the tensor, its numel): its contents are NOT read, nothing waits; the caller type-checks it (mem.check_list) after its own
    earlier checks.  Anything else is a host list, checked here — not descending, inside [lo, hi) (closed: [lo, hi]), ValueError
    otherwise — -> (False, the list as an int64 numpy array, its size), for the caller to upload once, after its last check.
    noun, place: what the messages call the elements and the bounds."""
    if mem.holds(x, kind):
        return True, x, int(x.numel())
    a = parse(x) if parse else np.asarray(x, np.int64).ravel()
    if a.size and (a[1:] < a[:-1]).any():
        raise ValueError("the %s must not descend" % noun)
    if a.size and (a[0] < lo or (a[-1] > hi if closed else a[-1] >= hi)):
        raise ValueError("%s outside %s [%d, %d%s" % (noun, place, lo, hi, "]" if closed else ")"))
    return False, a, int(a.size)


def _sized_by_data(mem, call, n_counts, shapes, want, caps, fill_empty=False, **first):
    """Count-then-fill, for results whose sizes are data — SYNCHRONISES ONCE: call(counts=, **first) asks for the n_counts sizes alone,
    the host reads them (mem.read: the one wait, as torch.nonzero has one), the arrays `want` of shapes(*sizes) = {destination: (shape,
    dtype)} are allocated exactly, and call(<caps> = the sizes, <destination> = ...) fills them without another wait — skipped when
    there is no destination, or (but with fill_empty) no first size.  -> (the sizes, {destination: array})"""
    counts = mem.zeros(n_counts, np.int32)
    call(counts=mem.ptr(counts), **first)
    sizes = [x & 0xFFFFFFFF for x in mem.read(counts)]
    shp = shapes(*sizes)
    arrays = {k: mem.empty(*shp[k]) for k in want}
    if want and (sizes[0] or fill_empty):
        call(**dict(zip(caps, sizes)), **_ptrs(mem, arrays))
    return sizes, arrays


def _mark_libraries(r, given, value, names, numbers=False):
    """r[l] = value for every library in `given` — one or a sequence of the engine's library names, with `numbers` library numbers
    too —, none of them twice.  names: a function that gives the engine's library names, called when the first name is met."""
    known = None
    for x in ([given] if isinstance(given, (str, bytes)) else list(given)):
        if numbers and not isinstance(x, (str, bytes)):
            if isinstance(x, bool) or int(x) != x or not 0 <= int(x) < r.size:
                raise ValueError("libs: library names or numbers in [0, %d)" % r.size)
            l = int(x)
        else:
            if known is None:
                known = names()
            x = x.decode() if isinstance(x, bytes) else x
            if x not in known:
                raise ValueError("%r is not a library of the engine (%r)" % (x, known))
            l = known.index(x)
        if r[l]:
            raise ValueError("library %r is named twice" % (x,))
        r[l] = value


def _library_names(engine, n_lib, who):
    """the engine's library names, one per library; who: the subject of the message ("libs names")"""
    names = [b.decode() for b in engine._names]
    if len(names) != n_lib:
        raise ValueError("%s libraries: the engine reports one set of counts for all of them" % who)
    return names


# ------------------------------------------------------------------------------------------------ the entry points

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
    want = _check_want(want, KINDS)
    v = engine.device_view()
    pos0, L = int(v.pos0), int(v.n_lib)
    k0, n = _window(v, beg0, end)
    mem = _memory(v)
    arrays = _arrays(mem, shapes(L, n), want, out)
    if n and want:                                                # NOTHING SYNCHRONISES: every size is known on the host
        dense.expand(v, k0, n, n, stream=mem.stream, **_ptrs(mem, arrays))
    return dict({"pos0": pos0, "first": pos0 + k0, "n": n, "n_lib": L}, **arrays)


INDEL_KINDS = capi.INDEL_DESTS
INDEL_DEFAULT_WANT = INDEL_KINDS


def indel_shapes(m, allele_bytes):
    """kind -> (shape, numpy dtype) of a table of m records: record r is element r of the last axis"""
    return {"pos": ((m,), np.int32), "lib": ((m,), np.int32), "len": ((m,), np.int32), "rep_read": ((m,), np.uint32), "rep_qpos": ((m,), np.int32),
            "istat": ((capi.NI, m), np.uint32), "fstat": ((capi.NF, m), np.float32), "metrics": ((capi.NMETRIC, m), np.float32),
            "allele_off": ((m + 1,), np.uint32), "alleles": ((allele_bytes,), np.uint8)}


def indels(engine, indels, beg0=None, end=None, want=INDEL_DEFAULT_WANT):
    """The indel buckets of the engine's last computed region whose position lies in [beg0, end) (clipped to the region's positions as
    region() clips), in brc_result.indel's order: ascending (position, library, allele text) — include/brc_indels.h.

    Returns a dict: every kind in `want` (INDEL_KINDS) -> an array shaped as in indel_shapes(): pos, lib, len, rep_read, rep_qpos [m],
    istat [9, m], fstat [4, m], metrics [13, m], allele_off [m + 1], alleles (uint8: the text of record r is
    alleles[allele_off[r]:allele_off[r + 1]], sign first), plus the ints "m" (records), "first" and "n" (the window).
    With the HIP libraries the arrays are torch tensors on the engine's device, filled on torch's current stream, the scratch comes
    from torch.empty; with the CPU builds they are numpy arrays.

    SYNCHRONISES ONCE: the table's sizes are data.  A first gather asks for the two counts alone, the host reads them (as
    torch.nonzero does), then the arrays are allocated exactly and a second gather fills them without another wait.
    """
    want = _check_want(want, INDEL_KINDS)
    v = engine.device_indels()
    k0, n = _window(v, beg0, end)
    wsb = indels.workspace(v, n)
    mem = _memory(v, "brc_device_indels")
    ws = _scratch(mem, wsb)
    # ONE WAIT: the two sizes are data
    (m, nbytes), arrays = _sized_by_data(mem, partial(indels.gather, v, k0, n, workspace=mem.ptr(ws), workspace_bytes=wsb, stream=mem.stream), 2,
                                         indel_shapes, want, ("cap", "alleles_cap"), fill_empty=True)
    return dict({"m": m, "first": int(v.pos0) + k0, "n": n}, **arrays)


def _window_positions(windows):
    """(vbeg0, vend) -> (positions of [vbeg0[i], vend[i]) of every window in order, the window number of each), int64"""
    if len(windows) != 2:
        raise ValueError("windows is a pair of arrays (vbeg0, vend)")
    b = np.asarray(windows[0], np.int64).ravel(); e = np.asarray(windows[1], np.int64).ravel()
    if b.shape != e.shape or (e < b).any():
        raise ValueError("windows: vbeg0 and vend must have one length, and no window may end before it begins")
    cnt = e - b
    n = int(cnt.sum())
    site = np.repeat(np.arange(b.size, dtype=np.int64), cnt)
    pos = np.repeat(b, cnt) + (np.arange(n, dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    return pos, site


def sites(engine, panel, positions=None, windows=None, want=DEFAULT_WANT, out=None, indels=None):
    """The LISTED positions of the engine's last computed region, and nothing else (include/brc_panel.h): for a region whose windows
    were announced with Engine.region_windows, where every other position is empty and a whole-axis region() would expand them all.

    Exactly one of
      positions: reference (axis) positions — a sequence, a numpy array, or (HIP libraries) an int32 torch tensor already on the
                 engine's device;
      windows:   a pair of arrays (vbeg0, vend), the arrays Engine.region_windows takes: the positions [vbeg0[i], vend[i]) of every
                 window, in order.
    A list given on the host is checked on the host — non-decreasing (equal neighbours are fine: site lists repeat lines) and inside
    the planes, ValueError otherwise, before anything is queued — and uploaded once.  A device tensor is used where it lies and NOT
    checked; nothing synchronises: "status" tells afterwards (capi.PANEL_OUT_OF_RANGE: such elements are empty positions;
    capi.PANEL_NOT_ASCENDING: buckets with a third-allele record are unspecified).

    Returns region()'s dict — every kind in `want` -> an array shaped shapes(n_lib, N), element j is listed position j — plus "pos"
    [N] int32 (the positions), "site" [N] int32 (the window number of each element; arange(N) for `positions`), "status" (one uint32
    element in the arrays' memory, written by the kernels, not read by this call) and the ints "n", "n_lib", "pos0".
    out: as for region().
    indels: a capi.Indels of the engine's kind -> also "indels": indels() over [min, max] of the list (SYNCHRONISES, see there; for a
    device list also to learn min and max), reduced to the records whose position is listed, each with "j": the index of the first
    listed element of its position.
    """
    if (positions is None) == (windows is None):
        raise ValueError("give exactly one of positions and windows")
    want = _check_want(want, KINDS)
    v = engine.device_view()
    P, pos0, L = int(v.n_pos), int(v.pos0), int(v.n_lib)
    mem = _memory(v)
    site = None
    if windows is not None:
        positions, site = _window_positions(windows)
    # NOTHING SYNCHRONISES for a device tensor (used where it lies, unread); a host list is checked here and uploaded once below
    here, pos, n = _listed(mem, positions, "positions", "listed positions", "the region's planes", pos0, pos0 + P)
    arrays = _arrays(mem, shapes(L, n), want, out)
    if here:
        mem.check_list(pos, "positions", "int32 tensor")
        idx, lpos, lsite = mem.offset(pos, -pos0), pos, mem.arange(n, np.int32)
    else:
        idx, lpos, lsite = mem.upload(np.stack([pos - pos0, pos, np.arange(n) if site is None else site]).astype(np.int32))       # one upload
    status = mem.zeros(1, np.uint32)
    if n:
        panel.gather(v, mem.ptr(idx), n, n, status=mem.ptr(status), stream=mem.stream, **_ptrs(mem, arrays))
    res = dict({"pos0": pos0, "n": n, "n_lib": L, "pos": lpos, "site": lsite, "status": status}, **arrays)
    if indels is not None:
        res["indels"] = _listed_indels(mem, engine, indels, lpos, n, pos0)
    return res


def _listed_indels(mem, engine, indels_lib, listed, n, pos0):
    """indels() over [min, max] of the listed positions, reduced to the records whose position is listed, plus "j": searchsorted and
    index arithmetic in numpy / torch, no kernel of its own."""
    if n == 0:
        t = indels(engine, indels_lib, beg0=pos0, end=pos0)          # (an empty window: no record)
    else:
        t = indels(engine, indels_lib, beg0=int(listed.min()), end=int(listed.max()) + 1)
    torch = mem.torch
    if torch is None:
        def take(a, sel):
            return a[..., sel]
        rep, cat = np.repeat, np.concatenate
        off = t["allele_off"].astype(np.int64)
        as_u32, as_i32 = (lambda a: a.astype(np.uint32)), (lambda a: a.astype(np.int32))
        arange, zero1 = np.arange, np.zeros(1, np.int64)
        jj = np.searchsorted(listed, t["pos"], side="left") if n else np.zeros(0, np.int64)
        sel = np.nonzero((jj < n) & (listed[np.minimum(jj, n - 1)] == t["pos"]))[0] if n else jj
    else:
        dev = mem.dev

        def take(a, sel):             # (torch indexes no unsigned 32-bit tensors: through their int32 view)
            if a.dtype == torch.uint32:
                return a.view(torch.int32).index_select(a.dim() - 1, sel).view(torch.uint32)
            return a.index_select(a.dim() - 1, sel)
        rep, cat = torch.repeat_interleave, torch.cat
        off = t["allele_off"].view(torch.int32).to(torch.int64)
        as_u32, as_i32 = (lambda a: a.to(torch.int32).view(torch.uint32)), (lambda a: a.to(torch.int32))

        def arange(k):
            return torch.arange(k, dtype=torch.int64, device=dev)
        zero1 = arange(1)
        jj = torch.searchsorted(listed, t["pos"]) if n else torch.zeros(0, dtype=torch.int64, device=dev)
        sel = ((jj < n) & (listed[jj.clamp(max=n - 1)] == t["pos"])).nonzero().reshape(-1) if n else jj
    # the kept records' allele text, packed: byte i of the new text comes from the old offset of its record + its place inside it
    lens = (off[1:] - off[:-1])[sel]
    new_off = cat([zero1, lens.cumsum(0)])
    src = rep(off[:-1][sel] - new_off[:-1], lens) + arange(int(new_off[-1]))
    res = {"first": t["first"], "n": t["n"], "m": int(sel.shape[0]), "j": as_i32(take(jj, sel))}
    for k in INDEL_KINDS:
        res[k] = as_u32(new_off) if k == "allele_off" else take(t[k], src if k == "alleles" else sel)
    return res


def _roles(engine, n_lib, role, case, control):
    """role (a sequence of capi.ROLE_* per library) or case= / control= (library names of the engine) -> uint8 [n_lib], or None"""
    if role is not None and (case is not None or control is not None):
        raise ValueError("give role, or case / control, not both")
    if role is None and case is None and control is None:
        return None
    if role is not None:
        r = np.asarray(role).ravel()
        if r.size != n_lib or (r.astype(np.int64) != r).any() or ((r < 0) | (r > capi.ROLE_CONTROL)).any():
            raise ValueError("role: one of 0 (ignore), 1 (case), 2 (control) per library, %d of them" % n_lib)
        r = r.astype(np.uint8)
    else:
        names = _library_names(engine, n_lib, "case / control name")
        r = np.zeros(n_lib, np.uint8)
        _mark_libraries(r, [] if case is None else case, capi.ROLE_CASE, lambda: names)
        _mark_libraries(r, [] if control is None else control, capi.ROLE_CONTROL, lambda: names)
    if not (r == capi.ROLE_CASE).any():
        raise ValueError("no case library")
    return r


def _u32(x, what):
    if isinstance(x, bool) or int(x) != x or not 0 <= int(x) < 2 ** 32:
        raise ValueError("%s must be an integer in [0, 2^32)" % what)
    return int(x)


def select(engine, select, *, role=None, case=None, control=None, snv=True, indel=True, min_depth, min_alt, min_frac=(0, 1), ctl_min_depth=0,
           ctl_max_alt=2 ** 32 - 1, ctl_max_frac=(1, 1), beg0=None, end=None):
    """The positions of [beg0, end) of the engine's last computed region (clipped as region() clips) that carry non-reference evidence
    in a case library and none in the control libraries — include/brc_select.h has the exact integer predicate:
      a base b other than the reference's (snv) or an insertion / a deletion (indel) with, in SOME case library, depth >= min_depth,
      count >= min_alt and count / depth >= min_frac (num, den), and in EVERY control library depth >= ctl_min_depth, count <=
      ctl_max_alt and count / depth <= ctl_max_frac.  Allele text is not compared: a control insertion of any spelling counts against an
      insertion candidate.
    role: one of capi.ROLE_IGNORE / ROLE_CASE / ROLE_CONTROL per library; or case= / control= lists of the engine's library names (the
    others are ignored); none of them: every library is a case library.

    Returns {"idx": int32 [n] plane indices, ascending, "pos": int32 [n] = pos0 + idx, "why": int32 [n] the reason bits (capi.WHY_*),
    "n": int, "first": int, "pos0": int}.  With the HIP libraries the arrays are torch tensors on the engine's device, filled on
    torch's current stream, the scratch comes from torch.empty; with the CPU builds they are numpy arrays.  "pos" is what
    sites(positions=...) takes.

    SYNCHRONISES ONCE: the list's length is data.  A first call asks for the count alone, the host reads it (as torch.nonzero does),
    then the list is allocated exactly and a second call fills it without another wait.
    ValueError for parameters the library would refuse, before anything is queued."""
    flags = (capi.SELECT_SNV if snv else 0) | (capi.SELECT_INDEL if indel else 0)
    if not flags:
        raise ValueError("nothing to look for: snv and indel are both off")
    for pair, what in ((min_frac, "min_frac"), (ctl_max_frac, "ctl_max_frac")):
        if len(pair) != 2:
            raise ValueError("%s is a pair (numerator, denominator)" % what)
    frac = (_u32(min_frac[0], "min_frac"), _u32(min_frac[1], "min_frac"))
    cfrac = (_u32(ctl_max_frac[0], "ctl_max_frac"), _u32(ctl_max_frac[1], "ctl_max_frac"))
    if frac[1] == 0 or cfrac[1] == 0:
        raise ValueError("a fraction's denominator must not be 0")
    if _u32(min_alt, "min_alt") == 0:
        raise ValueError("min_alt must be at least 1")
    v, d = engine.device_view(), engine.device_indels()
    pos0, L = int(v.pos0), int(v.n_lib)
    if L > capi.SELECT_MAX_LIB:
        raise ValueError("the selector takes at most %d libraries" % capi.SELECT_MAX_LIB)
    roles = _roles(engine, L, role, case, control)
    params, keep = capi.select_params(roles, flags, _u32(min_depth, "min_depth"), int(min_alt), frac, _u32(ctl_min_depth, "ctl_min_depth"),
                                      _u32(ctl_max_alt, "ctl_max_alt"), cfrac)
    k0, n = _window(v, beg0, end)
    wsb = select.workspace(v, d, n)
    mem = _memory(v)
    ws = _scratch(mem, wsb)
    # ONE WAIT: the list's length is data
    (m,), got = _sized_by_data(mem, partial(select.sites, v, d, params, k0, n, workspace=mem.ptr(ws), stream=mem.stream), 1,
                               lambda m: {"idx": ((m,), np.int32), "why": ((m,), np.int32)}, ("idx", "why"), ("cap",))
    del keep
    return {"idx": got["idx"], "pos": mem.offset(got["idx"], pos0), "why": got["why"], "n": m, "first": pos0 + k0, "pos0": pos0}


BIN_KINDS = ("sums", "covered", "hist")


def bins(engine, bins, *, width=None, edges=None, thresholds=(), hist=0, beg0=None, end=None, want=BIN_KINDS):
    """Per-bin summaries of the reference positions [beg0, end) of the engine's last computed region (clipped as region() clips),
    reduced where the region lies by libbrc_bins_hip.so (capi.Bins) — include/brc_bins.h has the exact definitions.

    Exactly one of
      width: uniform bins of `width` positions from the window's first position on (the last one may be shorter);
      edges: n_bins + 1 reference (axis) positions; bin b is [edges[b], edges[b + 1]), positions outside [edges[0], edges[-1]) lie in no
             bin, equal neighbours make an empty bin.  A sequence or numpy array is checked on the host — non-descending and inside the
             window [first, first + n], ValueError otherwise, before anything is queued — and uploaded once.  A one-dimensional int32
             torch tensor on the engine's device (HIP libraries) is used where it lies and NOT checked; nothing synchronises: "status"
             tells afterwards (capi.BINS_DESCENDS: the bins are what a binary search finds; capi.BINS_OUTSIDE: such edges count as
             the window's ends).
    thresholds: up to capi.BINS_MAX_THR depths for "covered"; hist: the bars of the depth histogram (0: none; depths of hist - 1 and
    above share the last bar).

    Returns a dict: every kind in `want` (BIN_KINDS) ->
      "sums"    uint64 [n_lib, capi.BINS_NSUM, n_bins]: per library and bin the sums of depth, ncol, the reads of the six buckets
                "=ACGTN", the non-reference reads, the insertion reads, the deletion reads, and the largest depth (capi.BINS_S_*)
      "covered" uint64 [n_lib, len(thresholds), n_bins]: positions with depth >= thresholds[t]
      "hist"    uint64 [n_lib, hist]: positions that lie in some bin, by min(depth, hist - 1)
    plus "status" (one uint32 element in the arrays' memory, written by the kernels, not read by this call), for uniform bins "start"
    (int64 [n_bins]: the reference position each bin starts at) and the ints "n_bins", "first", "n", "n_lib", "pos0".  Integer sums
    only: a mean is sums / (edges' differences or width), the caller's division (torch: .view(torch.int64) first — torch has few
    operators on unsigned types).
    With the HIP libraries the arrays are torch tensors on the engine's device, filled on torch's current stream; every size is
    known on the host, so NOTHING SYNCHRONISES.  With the CPU builds they are numpy arrays."""
    want = _check_want(want, BIN_KINDS)
    if (width is None) == (edges is None):
        raise ValueError("give exactly one of width and edges")
    thr = [_u32(t, "a threshold") for t in thresholds]
    if len(thr) > capi.BINS_MAX_THR:
        raise ValueError("at most %d thresholds" % capi.BINS_MAX_THR)
    if isinstance(hist, bool) or int(hist) != hist or not 0 <= int(hist) <= capi.BINS_MAX_HIST:
        raise ValueError("hist: 0 .. %d bars" % capi.BINS_MAX_HIST)
    n_hist = int(hist)
    if width is not None and (isinstance(width, bool) or int(width) != width or int(width) < 1):
        raise ValueError("width must be a positive integer")
    v, d = engine.device_view(), engine.device_indels()
    pos0, L = int(v.pos0), int(v.n_lib)
    mem = _memory(v)
    k0, n = _window(v, beg0, end)
    first = pos0 + k0
    if width is not None:
        n_bins = (n + int(width) - 1) // int(width)
    else:
        # NOTHING SYNCHRONISES for a device tensor (used where it lies, unread); a host list is checked here and uploaded once below
        here, e, n_edges = _listed(mem, edges, "edges", "edges", "the window", first, first + n, closed=True, parse=_edge_list)
        n_bins = n_edges - 1
        if n_bins < 0:
            raise ValueError("edges: at least one position")
    arrays = _arrays(mem, {"sums": ((L, capi.BINS_NSUM, n_bins), np.uint64), "covered": ((L, len(thr), n_bins), np.uint64),
                           "hist": ((L, n_hist), np.uint64)}, want)
    status = mem.zeros(1, np.uint32)
    if width is None and here:
        mem.check_list(e, "edges", "int32 tensor")
    res = {"n_bins": n_bins, "first": first, "n": n, "n_lib": L, "pos0": pos0, "status": status}
    if width is not None:
        res["start"] = first + mem.arange(n_bins, np.int64) * int(width)
        params = capi.bins_params(int(width), None, 0, thr, n_hist)
    else:
        idx = mem.offset(e, -pos0) if here else mem.upload((e - pos0).astype(np.int32))
        params = capi.bins_params(0, mem.ptr(idx, null_if_empty=True), n_bins, thr, n_hist)
        if params.edges is None:
            raise ValueError("edges: at least one position")
    bins.reduce(v, d, params, k0, n, n_bins, status=mem.ptr(status), stream=mem.stream, **_ptrs(mem, arrays, null_if_empty=True))
    res.update(arrays)
    return res


def _edge_list(edges):
    e = np.asarray(edges)
    if e.ndim != 1 or e.size < 1 or (e.size and (e.astype(np.int64) != e).any()):
        raise ValueError("edges: a one-dimensional list of at least one integer position")
    return e.astype(np.int64)


RUNS_COMBINE = {"min": capi.RUNS_MIN, "max": capi.RUNS_MAX, "sum": capi.RUNS_SUM}


def _counted(engine, n_lib, libs):
    """libs (library names of the engine, or library numbers) -> uint8 [n_lib] of 0 / 1, or None: every library counts"""
    if libs is None:
        return None
    given = [libs] if isinstance(libs, (str, bytes)) else list(libs)
    if not given:
        raise ValueError("no library is counted")
    r = np.zeros(n_lib, np.uint8)
    _mark_libraries(r, given, 1, partial(_library_names, engine, n_lib, "libs names"), numbers=True)
    return r


def runs(engine, runs, *, cuts, combine="min", libs=None, keep=None, ref_n=False, beg0=None, end=None):
    """The maximal intervals of [beg0, end) of the engine's last computed region (clipped as region() clips) over which the depth class
    is constant — include/brc_runs.h has the exact definition:
      V = the minimum ("min"), maximum ("max") or sum ("sum", in 64 bits) of the depth over the counted libraries; class = the number
      of cuts <= V, 0 .. len(cuts); with ref_n a position whose reference character is none of ACGTacgt has class len(cuts) + 1.
    cuts: 1 .. capi.RUNS_MAX_CUT depths, strictly ascending.  libs: the counted libraries, by the engine's library names or by number
    (None: all of them).  keep: the classes whose intervals are returned (None: all).

    Returns {"n": the number of intervals, "k0", "k1": int32 [n] plane indices [k0[j], k1[j]), ascending and disjoint, "start", "end":
    int32 [n] the same as reference positions pos0 + k, "cls": int32 [n] the class of each, "per_class": uint64 [n_class] the number of
    positions of each class in the window whatever keep is, "n_class": len(cuts) + 2}.  With the HIP libraries the arrays are torch
    tensors on the engine's device, filled on torch's current stream, the scratch comes from torch.empty; with the CPU builds they are
    numpy arrays.  "start" / "end" interleaved are what bins(edges=...) takes.

    SYNCHRONISES ONCE: the list's length is data.  A first call asks for the count and per_class alone, the host reads the count (as
    torch.nonzero does), then the list is allocated exactly and a second call fills it without another wait.
    ValueError for parameters the library would refuse, before anything is queued."""
    if combine not in RUNS_COMBINE:
        raise ValueError("combine: one of %r" % (sorted(RUNS_COMBINE),))
    try:
        cut = [_u32(c, "a cut") for c in cuts]
    except TypeError:
        raise ValueError("cuts: a sequence of integers")
    if not 1 <= len(cut) <= capi.RUNS_MAX_CUT:
        raise ValueError("cuts: 1 .. %d depths" % capi.RUNS_MAX_CUT)
    if any(b <= a for a, b in zip(cut, cut[1:])):
        raise ValueError("the cuts must ascend strictly")
    n_class = len(cut) + 2
    if keep is None:
        mask = (1 << (n_class if ref_n else n_class - 1)) - 1
    else:
        mask = 0
        for c in ([keep] if isinstance(keep, int) and not isinstance(keep, bool) else list(keep)):
            if isinstance(c, bool) or int(c) != c or not 0 <= int(c) < n_class:
                raise ValueError("keep: classes in [0, %d)" % n_class)
            mask |= 1 << int(c)
        if not mask:
            raise ValueError("keep is empty: no class would be returned")
    v = engine.device_view()
    pos0, L = int(v.pos0), int(v.n_lib)
    if L > capi.RUNS_MAX_LIB:
        raise ValueError("runs takes at most %d libraries" % capi.RUNS_MAX_LIB)
    d = None
    if ref_n:
        try:
            d = engine.device_indels()
        except capi.BrcError as e:
            raise ValueError("ref_n needs the engine's indels view, which carries the reference: %s" % e)
    params, keepalive = capi.runs_params(cut, RUNS_COMBINE[combine], _counted(engine, L, libs), mask, capi.RUNS_REF_N if ref_n else 0)
    k0, n = _window(v, beg0, end)
    wsb = runs.workspace(n)
    mem = _memory(v)
    ws, per = _scratch(mem, wsb), mem.zeros(n_class, np.uint64)
    # ONE WAIT: the list's length is data
    (m,), got = _sized_by_data(mem, partial(runs.find, v, d, params, k0, n, workspace=mem.ptr(ws), stream=mem.stream), 1,
                               lambda m: dict.fromkeys(("start", "end", "cls"), ((m,), np.int32)), ("start", "end", "cls"), ("cap",),
                               per_class=mem.ptr(per))
    del keepalive
    a, b = got["start"], got["end"]
    return {"n": m, "k0": a, "k1": b, "start": mem.offset(a, pos0), "end": mem.offset(b, pos0), "cls": got["cls"], "per_class": per, "n_class": n_class}


VET_KINDS = ("fail", "keep", "vals")


def vet_shapes(n_lib, n):
    """kind -> (shape, numpy dtype) of vet()'s arrays for a list of n elements: the last axis is the list element"""
    return {"fail": ((n_lib, 4, n), np.uint32), "keep": ((n,), np.int32), "vals": ((n_lib, 4, capi.VET_NVAL, n), np.float32)}


def _vet_tests(tests):
    if tests is None:
        return capi.VET_ALL_TESTS
    if isinstance(tests, (int, np.integer)) and not isinstance(tests, bool):
        if not 0 <= int(tests) <= capi.VET_ALL_TESTS:
            raise ValueError("tests: a mask of capi.VET_BIT values")
        return int(tests)
    mask = 0
    for t in ([tests] if isinstance(tests, str) else list(tests)):
        if t not in capi.VET_BIT:
            raise ValueError("unknown test %r (one of %r)" % (t, capi.VET_TESTS))
        mask |= capi.VET_BIT[t]
    return mask


def vet(engine, vet, *, idx, alt=None, libs=None, tests=None, want=VET_KINDS, **thresholds):
    """The per-allele read-metric tests of include/brc_vet.h on LISTED plane positions of the engine's last computed region: for
    element j, library l and every base v asked about, the variant bucket's count, strand counts and averages (position in read,
    distance to the 3' end, base quality, mapping quality, mismatch-quality sum, clipped length) against thresholds and against the
    reference base's bucket of the same site — exact integer tests, and fp32 tests stated operation by operation.

    idx: plane indices (select()'s "idx"), non-decreasing — a sequence or numpy array, or (HIP libraries) an int32 torch tensor on the
         engine's device, used where it lies.
    alt: per element a mask of capi.WHY_A | WHY_C | WHY_G | WHY_T, the bases asked about (select()'s "why"; insertion and deletion bits
         are ignored), of idx's kind; None: all four.
    libs: the judged libraries, by the engine's library names or by number (None: all).
    tests: the tests to run — names of capi.VET_TESTS, or a mask of capi.VET_BIT values (None: all eighteen).
    thresholds: members of brc_vet_params by name; capi.VET_DEFAULTS where not given: min_depth 8, min_var_count 4, freq 1 / 20,
         min_strand_reads 5, strand 1 / 100, min_ref_reads 2, min_var_readpos / min_var_dist3 / min_ref_readpos / min_ref_dist3 0.1,
         min_var_bq / min_var_mapq / min_ref_bq / min_ref_mapq 15, max_var_mmqs 100, min_var_rl / min_ref_rl 90, max_mmqs_diff /
         max_mapq_diff 50, max_rl_diff 0.25.

    Returns every kind in `want` — "fail": uint32 [n_lib, 4, n] failure words (bit i: capi.VET_TESTS[i]; capi.VET_NOT_ASKED,
    capi.VET_NO_SITE: nothing judged), "keep": int32 [n] the mask of asked bases that pass every test in SOME judged library, "vals":
    float32 [n_lib, 4, capi.VET_NVAL, n] the numbers compared (capi.VET_V_NAMES) — plus "status" (one uint32 element in the arrays'
    memory: capi.VET_OUT_OF_RANGE / VET_NOT_ASCENDING, written by the kernels, not read by this call) and the ints "n", "n_lib", "pos0".
    With the HIP libraries the arrays are torch tensors on the engine's device, filled on torch's current stream, the scratch comes from
    torch.empty; with the CPU builds they are numpy arrays.  NOTHING SYNCHRONISES: every size follows from n.  So
        sel = select(...); r = vet(engine, v, idx=sel["idx"], alt=sel["why"]); k = r["keep"].nonzero()[:, 0]
        panel = sites(engine, capi.Panel(), positions=sel["pos"][k])
    runs with device lists throughout.  A list given on the host is checked on the host (non-decreasing, inside the planes); a device
    tensor is not: "status" tells afterwards.  ValueError for what the library would refuse, before anything is queued."""
    want = _check_want(want, VET_KINDS)
    mask = _vet_tests(tests)
    unknown = set(thresholds) - set(capi.VET_DEFAULTS)
    if unknown:
        raise ValueError("unknown thresholds %r (capi.VET_DEFAULTS has the names)" % sorted(unknown))
    t = dict(capi.VET_DEFAULTS, **thresholds)
    for k in capi.VET_UINTS:
        t[k] = _u32(t[k], k)
    if t["freq_den"] == 0 or t["strand_den"] == 0:
        raise ValueError("a fraction's denominator must not be 0")
    for k in capi.VET_FLOATS:
        x = np.float32(t[k])
        if isinstance(t[k], bool) or not np.isfinite(x):
            raise ValueError("%s must be a finite number (in fp32)" % k)
        t[k] = float(x)
    v, d = engine.device_view(), engine.device_indels()
    P, pos0, L = int(v.n_pos), int(v.pos0), int(v.n_lib)
    if L > capi.VET_MAX_LIB:
        raise ValueError("the filter takes at most %d libraries" % capi.VET_MAX_LIB)
    mem = _memory(v)
    params, keepalive = capi.vet_params(_counted(engine, L, libs), mask, **t)
    if alt is not None and _is_torch(alt) != _is_torch(idx):
        raise ValueError("idx and alt must be of one kind: both torch tensors or both host arrays")
    words = "32-bit integer tensor of idx's length"
    # NOTHING SYNCHRONISES for device tensors (used where they lie, unread); host lists are checked here and uploaded once each below
    here, lidx, n = _listed(mem, idx, "indices", "listed indices", "the region's planes", 0, P)
    wsb = vet.workspace(v, n)
    if here:
        mem.check_list(lidx, "idx", words)
        if alt is not None:
            mem.check_list(alt, "alt", words, dtypes=(np.int32, np.uint32), n=n)
    elif alt is not None:
        alt = np.asarray(alt, np.int64).ravel()
        if alt.size != n or ((alt < 0) | (alt >= 2 ** 32)).any():
            raise ValueError("alt: one mask of capi.WHY_* per listed element")
    arrays = _arrays(mem, vet_shapes(L, n), want)
    ws, status = _scratch(mem, wsb), mem.zeros(1, np.uint32)
    if not here:                                                  # host lists: one upload each
        lidx = mem.upload(lidx.astype(np.int32))
        alt = None if alt is None else mem.upload(alt.astype(np.uint32))
    if n:
        vet.sites(v, d, params, mem.ptr(lidx), None if alt is None else mem.ptr(alt), n, n, status=mem.ptr(status), workspace=mem.ptr(ws), stream=mem.stream,
                  **_ptrs(mem, arrays))
    del keepalive
    return dict({"pos0": pos0, "n": n, "n_lib": L, "status": status}, **arrays)


IVET_KINDS = ("fail", "keep", "vals", "ctl_count")
_IVET_KIND_BITS = {"ins": capi.WHY_INS, "del": capi.WHY_DEL}


def ivet_shapes(m, n):
    """kind -> (shape, numpy dtype) of vet_indels()'s arrays for a table of m records and a list of n elements"""
    return {"fail": ((m,), np.uint32), "keep": ((n,), np.int32), "vals": ((capi.IVET_NVAL, m), np.float32), "ctl_count": ((m,), np.uint32)}


def _ivet_tests(tests):
    if tests is None:
        return capi.IVET_ALL_TESTS
    if isinstance(tests, (int, np.integer)) and not isinstance(tests, bool):
        if int(tests) < 0 or int(tests) & ~capi.IVET_ALL_TESTS:
            raise ValueError("tests: a mask of capi.IVET_BIT values (VAR_BQ is not a test of indel records)")
        return int(tests)
    mask = 0
    for t in ([tests] if isinstance(tests, str) else list(tests)):
        if t not in capi.IVET_BIT:
            raise ValueError("unknown test %r (one of %r)" % (t, capi.IVET_TESTS))
        mask |= capi.IVET_BIT[t]
    return mask


def vet_indels(engine, ivet, table, *, idx=None, why=None, role=None, case=None, control=None, kinds=("ins", "del"), tests=None, want=IVET_KINDS,
               **thresholds):
    """The read-metric tests of include/brc_ivet.h on every record of a sorted indel TABLE of the engine's last computed region — the
    record's own sums against the reference base's bucket at the record's pileup position, the seventeen tests of vet() other than
    VAR_BQ — and an ALLELE-AWARE control veto: CTL_ALLELE is set when a control library has a record of the same position, length and
    text whose count fails count <= ctl_max_count and count / depth <= ctl_frac_num / ctl_frac_den; CTL_DEPTH when a control library
    is shallower than ctl_min_depth there.

    table: the dict indels(...) returns, or sites(..., indels=...)["indels"]: pos, lib, len, istat, fstat, allele_off, alleles and "m",
         used where they lie (an array that is not contiguous is packed first: a copy on the stream, no wait).
    idx, why: optionally select()'s list ("idx", "why"), non-decreasing plane indices — a sequence or numpy array, or (HIP libraries)
         int32 torch tensors on the engine's device, used where they lie.  why None: insertions and deletions both count.
    role / case / control: as in select(); none of them: every library is a case library (no control test can fail).
    kinds: the kinds of record judged, of "ins" and "del".
    tests: names of capi.IVET_TESTS, or a mask of capi.IVET_BIT values (None: all nineteen).
    thresholds: members of brc_ivet_params by name; capi.IVET_DEFAULTS where not given: vet()'s defaults, ctl_min_depth 0,
         ctl_max_count 0 and ctl_frac 1 / 1 — any read of the same allele in a control library vetoes.

    Returns every kind in `want` — "fail": uint32 [m] failure words (capi.IVET_BIT; capi.IVET_NOT_ASKED, capi.IVET_NO_SITE: nothing
    judged), "vals": float32 [capi.IVET_NVAL, m] the numbers compared (capi.VET_V_NAMES), "ctl_count": uint32 [m] the largest count of
    a control record of the same allele, "keep": int32 [n] per list element the OR of capi.WHY_INS / WHY_DEL over its records that
    pass every test (restricted to the kinds in why) — plus "status" (one uint32 element in the arrays' memory: capi.IVET_LIST_* /
    IVET_TABLE_* bits, written by the kernels, not read by this call) and the ints "m", "n", "n_lib", "pos0".
    With the HIP libraries the arrays are torch tensors on the engine's device, filled on torch's current stream; with the CPU builds
    they are numpy arrays.  NOTHING SYNCHRONISES: every size follows from table["m"] and n.

    An allele-aware veto end to end: select()'s own control veto does not compare allele text, so run it with the control libraries
    IGNORED, and give them to vet_indels as control:
        sel = select(eng, s, role=[1, 0], snv=False, min_depth=8, min_alt=3)           # library 1 (the normal) ignored
        t = indels(eng, capi.Indels())
        r = vet_indels(eng, capi.IVet(), t, idx=sel["idx"], why=sel["why"], role=[1, 2], ctl_max_count=1)
        panel = sites(eng, capi.Panel(), positions=sel["pos"][r["keep"].nonzero()[:, 0]])
    Records of one event placed apart inside a repeat meet only in a normalised table: vet_indels(eng, ivet, normalize_indels(eng, inorm,
    indels(eng, lib)), role=[1, 2]); the verdicts go back to the raw records as r["fail"][norm["src"]["group"]] (group -1: not judged).
    ValueError for what the library would refuse, before anything is queued."""
    want = _check_want(want, IVET_KINDS)
    mask = _ivet_tests(tests)
    kmask = 0
    for x in ([kinds] if isinstance(kinds, str) else list(kinds)):
        if x not in _IVET_KIND_BITS:
            raise ValueError("kinds: of 'ins' and 'del'")
        kmask |= _IVET_KIND_BITS[x]
    if not kmask:
        raise ValueError("kinds: at least one of 'ins' and 'del'")
    unknown = set(thresholds) - set(capi.IVET_DEFAULTS)
    if unknown:
        raise ValueError("unknown thresholds %r (capi.IVET_DEFAULTS has the names)" % sorted(unknown))
    t = dict(capi.IVET_DEFAULTS, **thresholds)
    for k in capi.IVET_UINTS:
        t[k] = _u32(t[k], k)
    if t["freq_den"] == 0 or t["strand_den"] == 0 or t["ctl_frac_den"] == 0:
        raise ValueError("a fraction's denominator must not be 0")
    for k in capi.IVET_FLOATS:
        with np.errstate(over="ignore"):
            x = np.float32(t[k])
        if isinstance(t[k], bool) or not np.isfinite(x):
            raise ValueError("%s must be a finite number (in fp32)" % k)
        t[k] = float(x)
    v, d = engine.device_view(), engine.device_indels()
    P, pos0, L = int(v.n_pos), int(v.pos0), int(v.n_lib)
    if L > capi.IVET_MAX_LIB:
        raise ValueError("the filter takes at most %d libraries" % capi.IVET_MAX_LIB)
    mem = _memory(v)
    params, keepalive = capi.ivet_params(_roles(engine, L, role, case, control), mask, kmask, **t)
    # the table, where it lies
    need = ("pos", "lib", "len", "istat", "fstat") + (("allele_off", "alleles") if mask & capi.IVET_BIT["CTL_ALLELE"] else ())
    if not isinstance(table, dict) or "m" not in table or any(k not in table for k in need):
        raise ValueError("table: the dict indels() returns, with %r" % (need,))
    m = int(table["m"])
    tab = capi.IVetTable(m, m)
    held, shp = [], indel_shapes(m, 0)
    for k in ("pos", "lib", "len", "istat", "fstat", "allele_off", "alleles"):
        a = table.get(k)
        if a is None:
            continue
        shape, dt = shp[k]
        if _is_torch(a) != (mem.torch is not None) or tuple(a.shape) != (shape if k != "alleles" else tuple(a.shape)[:1]):
            raise ValueError("table[%r] is not an array of shape %r of a table of %d records in the engine's memory" % (k, shape, m))
        dts = (dt, np.int32) if dt == np.uint32 else (dt,)            # (torch code often carries unsigned words as int32)
        if (a.dtype not in dts) if mem.torch is None else (a.dtype not in [mem.dtype[x] for x in dts]):
            raise ValueError("table[%r] must hold %s" % (k, np.dtype(dt).name))
        if mem.torch is not None and a.device != mem.dev:
            raise ValueError("table[%r] must be a tensor on %s" % (k, mem.dev))
        a = np.ascontiguousarray(a) if mem.torch is None else a.contiguous()      # (used where it lies; a strided selection is packed first)
        held.append(a)
        setattr(tab, k, mem.ptr(a))
    if table.get("alleles") is not None:
        tab.alleles_len = int(table["alleles"].shape[0])
    if why is not None and idx is None:
        raise ValueError("why needs idx")
    n, lidx, here = 0, None, False
    if idx is not None:
        if why is not None and _is_torch(why) != _is_torch(idx):
            raise ValueError("idx and why must be of one kind: both torch tensors or both host arrays")
        words = "32-bit integer tensor of idx's length"
        # NOTHING SYNCHRONISES for device tensors (used where they lie, unread); host lists are checked here and uploaded once each below
        here, lidx, n = _listed(mem, idx, "indices", "listed indices", "the region's planes", 0, P)
        if here:
            mem.check_list(lidx, "idx", words)
            if why is not None:
                mem.check_list(why, "why", words, dtypes=(np.int32, np.uint32), n=n)
        elif why is not None:
            why = np.asarray(why, np.int64).ravel()
            if why.size != n or ((why < 0) | (why >= 2 ** 32)).any():
                raise ValueError("why: one mask of capi.WHY_* per listed element")
    wsb = ivet.workspace(v, m)
    arrays = _arrays(mem, ivet_shapes(m, n), want)
    ws, status = _scratch(mem, wsb), mem.zeros(1, np.uint32)
    if idx is not None and not here:                              # host lists: one upload each
        lidx = mem.upload(lidx.astype(np.int32))
        why = None if why is None else mem.upload(why.astype(np.uint32))
    if m or n:
        ivet.records(v, d, params, tab, mem.ptr(lidx) if n else None, mem.ptr(why) if (n and why is not None) else None, n, m, status=mem.ptr(status),
                     workspace=mem.ptr(ws), stream=mem.stream, **_ptrs(mem, arrays))
    del keepalive, held
    return dict({"pos0": pos0, "m": m, "n": n, "n_lib": L, "status": status}, **arrays)


INORM_KINDS = INDEL_KINDS + ("members",)
_INORM_NEED = ("pos", "lib", "len", "istat", "fstat", "allele_off", "alleles")


def _table_arrays(mem, table, need, optional):
    """The arrays of an indel table dict, where they lie, validated as vet_indels() validates its table -> (m, {name: contiguous array});
    a strided selection is packed first: a copy on the stream, no wait."""
    if not isinstance(table, dict) or any(k not in table for k in ("m", "first", "n") + need):
        raise ValueError("table: the dict indels() returns, with %r and its window 'm', 'first', 'n'" % (need,))
    m = int(table["m"])
    held, shp = {}, indel_shapes(m, 0)
    for k in need + optional:
        a = table.get(k)
        if a is None:
            continue
        shape, dt = shp[k]
        if _is_torch(a) != (mem.torch is not None) or tuple(a.shape) != (shape if k != "alleles" else tuple(a.shape)[:1]):
            raise ValueError("table[%r] is not an array of shape %r of a table of %d records in the engine's memory" % (k, shape, m))
        dts = (dt, np.int32) if dt == np.uint32 else (dt,)            # (torch code often carries unsigned words as int32)
        if (a.dtype not in dts) if mem.torch is None else (a.dtype not in [mem.dtype[x] for x in dts]):
            raise ValueError("table[%r] must hold %s" % (k, np.dtype(dt).name))
        if mem.torch is not None and a.device != mem.dev:
            raise ValueError("table[%r] must be a tensor on %s" % (k, mem.dev))
        held[k] = np.ascontiguousarray(a) if mem.torch is None else a.contiguous()
    return m, held


def normalize_indels(engine, inorm, table, *, max_shift=1024, want=INORM_KINDS):
    """A sorted indel TABLE of the engine's last computed region LEFT-ALIGNED against the uploaded reference and MERGED — include/
    brc_inorm.h has the exact rule: every record steps left while the reference character at its position matches the last character
    of its text (an insertion's text rotates, a deletion's becomes the reference's raw characters of the stretch it now deletes), at
    most max_shift steps and not past the table's window or the reference slice; records that became equal in (position, library,
    length, text) become one, with integer sums, fp32 sums in ascending input order and the thirteen columns of the sums.

    table: the dict indels(...) returns, or sites(..., indels=...)["indels"]: pos, lib, len, istat, fstat, allele_off, alleles (rep_read
         and rep_qpos where it has them) and "m", "first", "n" — the window is the table's own; used where they lie (an array that is
         not contiguous is packed first: a copy on the stream, no wait).
    max_shift: 0 .. capi.INORM_MAX_SHIFT; 0 merges without shifting.

    Returns a dict of indels()'s shape — every kind in `want` (INORM_KINDS: INDEL_KINDS and "members": uint32 [m'], the records merged
    into each) for the m' merged records, in indels()'s order, plus the ints "m" (= m'), "first", "n" — that vet_indels() takes as it
    is, plus "src": {"npos": int32, "shift": uint32, "flags": uint32 (capi.INORM_NOT_JUDGED / INORM_LIMIT / INORM_EDGE), "group": int32}
    [table["m"]] over the INPUT records — group is the merged record each went into, -1 for a record that is not judged — and
    "status" (one uint32 element in the arrays' memory: capi.INORM_TABLE_BAD / INORM_ANY_LIMIT / INORM_ANY_EDGE, written by the
    kernels, not read by this call).  rep_read and rep_qpos are those of a class's first member: provenance only.
    With the HIP libraries the arrays are torch tensors on the engine's device, filled on torch's current stream, the scratch comes
    from torch.empty; with the CPU builds they are numpy arrays.

    SYNCHRONISES ONCE: the merged table's sizes are data.  A first call asks for the two counts alone, the host reads them (as
    torch.nonzero does), then the arrays are allocated exactly and a second call fills them without another wait.
    ValueError for what the library would refuse, before anything is queued."""
    want = _check_want(want, INORM_KINDS)
    if isinstance(max_shift, bool) or int(max_shift) != max_shift or not 0 <= int(max_shift) <= capi.INORM_MAX_SHIFT:
        raise ValueError("max_shift: an integer in [0, %d]" % capi.INORM_MAX_SHIFT)
    d = engine.device_indels()
    pos0, P = int(d.pos0), int(d.n_pos)
    mem = _memory(d, "brc_device_indels")
    m, held = _table_arrays(mem, table, _INORM_NEED, ("rep_read", "rep_qpos"))
    first, n = int(table["first"]), int(table["n"])
    k0 = first - pos0 if n else 0
    if n < 0 or k0 < 0 or k0 + n > P:
        raise ValueError("table: its window [%d, %d) lies outside the region's positions [%d, %d)" % (first, first + n, pos0, pos0 + P))
    src = capi.INormSource(m, m, alleles_len=int(held["alleles"].shape[0]))
    for k, a in held.items():
        setattr(src, k, mem.ptr(a))
    params = capi.INormParams(int(max_shift))
    wsb = inorm.workspace(n, m)
    ws, status = _scratch(mem, wsb), mem.zeros(1, np.uint32)
    if m and not n:                                               # (a window of no positions: the library judges nothing and writes nothing)
        per = {"npos": held["pos"] + 0, "shift": mem.zeros((m,), np.uint32), "flags": mem.zeros((m,), np.uint32), "group": mem.zeros((m,), np.int32) - 1}
    else:
        per = {"npos": mem.empty((m,), np.int32), "shift": mem.empty((m,), np.uint32), "flags": mem.empty((m,), np.uint32), "group": mem.empty((m,), np.int32)}

    def shapes_of(mm, nbytes):
        return dict(indel_shapes(mm, nbytes), members=((mm,), np.uint32))

    def call(**kw):                                               # (the per-record arrays and the status word ride on the filling call)
        if "counts" not in kw:
            kw = dict(kw, status=mem.ptr(status), **_ptrs(mem, per))
        inorm.table(d, params, src, k0, n, workspace=mem.ptr(ws), workspace_bytes=wsb, stream=mem.stream, **kw)
    # ONE WAIT: the two sizes are data
    (mm, nbytes), arrays = _sized_by_data(mem, call, 2, shapes_of, want, ("cap", "alleles_cap"), fill_empty=True)
    if not want:                                                  # (nothing of the merged table wanted: the per-record arrays alone)
        call(cap=0, alleles_cap=0)
    del held
    return dict({"m": mm, "first": first, "n": n, "src": per, "status": status}, **arrays)


class Joined:
    """What join() returns: the joined region as every function of this module asks an engine for it — device_view(),
    device_indels(), _names — over arrays this object holds (`arrays`: capi.JOIN_DESTS -> array; `status`: one uint32 element,
    capi.JOIN_REF_DIFFERS; `counts`: kept indel records, bytes of seq4).  close() lets the arrays go."""

    def __init__(self, view, indels, names, arrays, status, counts):
        self._view, self._indels, self._names, self.arrays, self.status, self.counts = view, indels, names, arrays, status, counts

    def _copy(self, v):
        if self.arrays is None:
            raise capi.BrcError("the joined region was closed")
        c = type(v)()
        capi.C.memmove(capi.C.byref(c), capi.C.byref(v), capi.C.sizeof(v))
        return c

    def device_view(self):
        return self._copy(self._view)

    def device_indels(self):
        return self._copy(self._indels)

    def close(self):
        self.arrays = self.status = None


def join(engines, join, names=None, beg0=None, end=None):
    """The last computed regions of several engines — two BAM files, a tumour and its normal — COPIED into one region: the libraries of
    engines[s] become the libraries behind those of engines[:s], over the window [beg0, end) (None: from the first / to the last
    position any engine has; the window is NOT clipped: where an engine has no planes its libraries are empty positions).  include/
    brc_join.h has the exact rule: 116 bytes per position and library copied once by libbrc_join_hip.so (capi.Join), third-allele and
    indel records relabelled, one synthetic read per indel record that spells what the source's read spelled, the reference slices
    merged.

    names: one label per engine (default "0", "1", ...): the libraries of a joined engine are called `label` (an engine that counts
    all libraries as one) or `label/<library name>`.

    Returns a Joined: device_view(), device_indels() and _names as an engine has them, so region(), indels(), sites(), select(),
    bins(), runs(), vet(), normalize_indels() and vet_indels() take it in an engine's place.  It holds its arrays — torch tensors on
    the engines' device, filled on torch's current stream, with the HIP libraries; numpy arrays with the CPU builds — and is a COPY:
    once the stream has run the join (the caller synchronises, as for region()) the engines may begin another region or be closed.
    Its unavail is absent (0xFFFFFFFF everywhere), rep_read / rep_qpos of its indel records are the join's own.

    SYNCHRONISES ONCE when the engines hold indel records: the bytes of the synthetic reads are data (a first call asks for the
    counts alone).  ValueError, before anything is queued: no engine or more than capi.JOIN_MAX_SOURCES, engines on different devices, a
    mix of host and device engines, more than capi.JOIN_MAX_LIB libraries, duplicate labels, an empty window."""
    engines = list(engines)
    if not 1 <= len(engines) <= capi.JOIN_MAX_SOURCES:
        raise ValueError("join: 1 .. %d engines" % capi.JOIN_MAX_SOURCES)
    labels = [str(s) for s in range(len(engines))] if names is None else [x.decode() if isinstance(x, bytes) else str(x) for x in names]
    if len(labels) != len(engines) or len(set(labels)) != len(labels):
        raise ValueError("names: one label per engine, none of them twice")
    pairs = [(e.device_view(), e.device_indels()) for e in engines]
    kinds = {(int(v.memory), int(v.device)) for v, _ in pairs}
    if len({m for m, _ in kinds}) != 1:
        raise ValueError("join: a mix of engines with results in host and in device memory")
    if len(kinds) != 1:
        raise ValueError("join: engines on different devices")
    lib_names = []
    for e, (v, _), label in zip(engines, pairs, labels):
        own = [b.decode() for b in e._names]
        lib_names += [label] if int(v.n_lib) == 1 and len(own) != 1 else ["%s/%s" % (label, x) for x in _library_names(e, int(v.n_lib), "names")]
    if len(lib_names) > capi.JOIN_MAX_LIB:
        raise ValueError("join: %d libraries, more than %d" % (len(lib_names), capi.JOIN_MAX_LIB))
    lo = min(int(v.pos0) for v, _ in pairs) if beg0 is None else int(beg0)
    hi = max(int(v.pos0) + int(v.n_pos) for v, _ in pairs) if end is None else int(end)
    n = hi - lo
    if n <= 0:
        raise ValueError("join: the window [%d, %d) is empty" % (lo, hi))
    mem = _memory(pairs[0][0])
    src = capi.join_sources(pairs)
    z = join.sizes(src, lo, n, n)
    L, S = int(z.n_lib), int(z.n_slots)
    shp = {"ncol": ((L, n), np.uint32), "depth": ((L, n), np.uint32), "slotid": ((L, n), np.uint32), "si": ((L, 2, capi.NI, n), np.uint32),
           "sf": ((L, 2, capi.NF, n), np.float32), "xagg": ((int(z.n_xagg), 16), np.uint32), "slots": ((S, 18), np.uint32), "seq_off": ((S,), np.uint64),
           "l_qseq": ((S,), np.int32), "ref": ((int(z.ref_bytes),), np.uint8)}
    arrays = {k: mem.empty(*shp[k]) for k in shp}
    wsb = int(z.workspace_bytes)
    ws, status = _scratch(mem, wsb), mem.zeros(1, np.uint32)
    view, indels = capi.DeviceView(), capi.DeviceIndels()

    def call(counts=None, seq_cap=0, seq4=None, **_):
        if counts is not None:                                    # (the counts alone)
            join.views(src, lo, n, n, counts=counts, workspace=mem.ptr(ws), workspace_bytes=wsb, stream=mem.stream)
            return
        dest = capi.JoinDest(seq4=seq4, **_ptrs(mem, {k: arrays[k] for k in shp}, null_if_empty=True))
        join.views(src, lo, n, n, dest=dest, out_view=view, out_indels=indels, counts=mem.ptr(counts_out), seq_cap=seq_cap, status=mem.ptr(status),
                   workspace=mem.ptr(ws), workspace_bytes=wsb, stream=mem.stream)
    counts_out = mem.zeros(2, np.uint32)
    if S:                                                         # ONE WAIT: the bytes of the synthetic reads are data
        _, filled = _sized_by_data(mem, call, 2, lambda kept, nbytes: {"seq4": ((nbytes,), np.uint8)}, ("seq4",), ("kept", "seq_cap"), fill_empty=True)
        arrays["seq4"] = filled["seq4"]
    else:                                                         # NOTHING SYNCHRONISES: no indel record, no read
        arrays["seq4"] = mem.empty((0,), np.uint8)
        call(seq_cap=0, seq4=mem.ptr(arrays["seq4"]))
    return Joined(view, indels, [x.encode() for x in lib_names], arrays, status, counts_out)


CONS_KINDS = ("seq", "off", "call", "cnt", "ins_rec")
_CONS_NEED = ("pos", "lib", "len", "istat", "allele_off", "alleles")


def cons_shapes(n, seq_bytes):
    """kind -> (shape, numpy dtype) of consensus()'s arrays for a window of n positions and a sequence of seq_bytes bytes"""
    return {"seq": ((seq_bytes,), np.uint8), "off": ((n + 1,), np.uint32), "call": ((n,), np.uint8), "cnt": ((cons_api.CONS_NCNT, n), np.uint32),
            "ins_rec": ((n,), np.uint32)}


def _fraction(x, what):
    try:
        num, den = x
    except (TypeError, ValueError):
        raise ValueError("%s: a pair (numerator, denominator)" % what)
    num, den = _u32(num, what), _u32(den, what)
    if not 1 <= den <= 65535 or num > den:
        raise ValueError("%s: a fraction of at most 1 with a denominator in [1, 65535]" % what)
    return num, den


def _character(x, what):
    if isinstance(x, str):
        x = x.encode("latin-1")
    if isinstance(x, bytes) and len(x) == 1:
        return x[0]
    raise ValueError("%s: one character" % what)


def consensus(engine, cons, *, table=None, indels=None, libs=None, min_depth, min_count=1, frac=(1, 2), ins_min_count=None, ins_frac=None,
              aligned=False, fill="N", gap="-", ins_centric=False, beg0=None, end=None, want=CONS_KINDS):
    """The CONSENSUS SEQUENCE of the reference positions [beg0, end) of the engine's last computed region (clipped as region() clips) —
    include/brc_cons.h has the exact rule: per position, pooled over the counted libraries, the read counts c of A C G T and d, the
    reads that carry a deletion across it (the deletion records of the table, each covering the |len| positions behind its anchor);
    T = their sum; a count x qualifies when x >= min_count and x / T >= frac.  The position is uncalled below min_depth, deleted when d
    qualifies and exceeds every base, otherwise the IUPAC code of the qualifying bases.  Behind a position the insertion with the
    largest support (its text's counts pooled over the counted libraries) is placed when it reaches ins_min_count and ins_frac of the
    depth.

    engine: an engine or a Joined.
    table: what indels() or normalize_indels() returned (better the second: it pools the placements of one event in a repeat), of the
         whole view or at least of every deletion that reaches into the window; None: gathered over the whole view through `indels`
         (a capi.Indels handle; one more synchronisation).
    libs: the counted libraries, by the engine's library names or by number (None: all).
    ins_min_count, ins_frac: None: min_count and frac.
    aligned: one byte per position — `gap` on deleted positions, no insertion —, so the sequence has n bytes and NOTHING SYNCHRONISES.
    fill: the character of an uncalled position, or "ref": the reference's own character there ('N' where there is none).
    ins_centric: the engine was configured insertion-centric (the anchor's base counts exclude the insertion's reads).

    Returns every kind in `want` (CONS_KINDS) — "seq": uint8 [counts] the sequence; "off": uint32 [n + 1] the offset in it of every
    position's first byte (off[n] = its length): the liftover map; "call": uint8 [n] one byte per position; "cnt": uint32 [6, n] the low
    32 bits of c[A], c[C], c[G], c[T], d and the chosen insertion's support (consensus.CONS_C_NAMES); "ins_rec": uint32 [n] the table
    index of the accepted insertion, consensus.CONS_NO_INS where there is none — plus "status" (one uint32 element in the arrays'
    memory: consensus.CONS_TABLE_* bits, written by the kernels, not read by this call), "m" (table records) and the ints "first", "n".
    With the HIP libraries the arrays are torch tensors on the engine's device, filled on torch's current stream, the scratch comes from
    torch.empty; with the CPU builds they are numpy arrays.

    SYNCHRONISES ONCE unless aligned: the sequence's length is data.  A first call asks for the count alone, the host reads it (as
    torch.nonzero does), then the sequence is allocated exactly and a second call fills everything without another wait.
    ValueError for what the library would refuse, before anything is queued."""
    want = _check_want(want, CONS_KINDS)
    num, den = _fraction(frac, "frac")
    inum, iden = (num, den) if ins_frac is None else _fraction(ins_frac, "ins_frac")
    min_depth, min_count = _u32(min_depth, "min_depth"), _u32(min_count, "min_count")
    ins_min_count = min_count if ins_min_count is None else _u32(ins_min_count, "ins_min_count")
    flags = (cons_api.CONS_ALIGNED if aligned else 0) | (cons_api.CONS_INS_CENTRIC if ins_centric else 0)
    if fill == "ref":
        flags |= cons_api.CONS_FILL_REF
        fill = "N"
    fill, gap = _character(fill, "fill"), _character(gap, "gap")
    if table is None:
        if indels is None:
            raise ValueError("consensus needs the indel table: table=, or indels= (a capi.Indels handle) to gather it")
        table = globals()["indels"](engine, indels, want=_CONS_NEED)
    v, d = engine.device_view(), engine.device_indels()
    L = int(v.n_lib)
    if L > cons_api.CONS_MAX_LIB:
        raise ValueError("the consensus caller takes at most %d libraries" % cons_api.CONS_MAX_LIB)
    mem = _memory(v)
    params, keepalive = cons_api.cons_params(_counted(engine, L, libs), flags, min_depth, min_count, (num, den), ins_min_count, (inum, iden), fill, gap)
    m, held = _table_arrays(mem, table, _CONS_NEED, ())
    tab = cons_api.ConsTable(m, m, alleles_len=int(held["alleles"].shape[0]))
    for k in ("pos", "lib", "len", "allele_off", "alleles"):
        setattr(tab, k, mem.ptr(held[k]))
    tab.count = mem.ptr(held["istat"])                            # (row I_N = 0 of the contiguous [9, m] planes)
    k0, n = _window(v, beg0, end)
    wsb = cons.workspace(v, n, m)
    ws, status = _scratch(mem, wsb), mem.zeros(1, np.uint32)
    call = partial(cons.call, v, d, params, tab, k0, n, n, status=mem.ptr(status), workspace=mem.ptr(ws), stream=mem.stream)
    if aligned:                                                   # NOTHING SYNCHRONISES: the sequence has n bytes
        arrays = _arrays(mem, cons_shapes(n, n), want)
        if want:
            call(seq_cap=n, **_ptrs(mem, arrays))
    else:                                                         # ONE WAIT: the sequence's length is data
        _, arrays = _sized_by_data(mem, call, 1, partial(cons_shapes, n), want, ("seq_cap",), fill_empty=True)
    del keepalive, held
    return dict({"first": int(v.pos0) + k0, "n": n, "m": m, "status": status}, **arrays)
