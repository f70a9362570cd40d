"""The device-side join of computed regions against what a consumer can do without it, on one box in one invocation (DESIGN.md 6n;
results: profiles/join_bench.json).

Two pairs of resident regions, the shapes behind tools/inorm_bench.py: the shape of BASELINE config 5 (synthgen tumor200x, 1 Mbp, four
libraries) split into two per-library engines of two libraries each, and config 3 (wgs30x, 4 Mbp, all libraries as one) twice.  The legs
ALTERNATE round by round until each has at least --min-seconds of its own timed work, after a warm-up round:

  torch_slice_copies     the yardstick, what a consumer can do today: the joined PLANES assembled by one torch slice assignment per
                         source and plane from tensors wrapped around the sources' pointers, and a torch.cat of the third-allele and of
                         the indel record buffers.  LEFT OUT, because torch has no one-line form of them: the renumbering of the records'
                         libraries, the rebasing of their positions, the synthetic reads and the merged reference slice.
  join_all               tensors.join: every destination, with its one wait for the bytes of the synthetic reads
  join_planes_only       brc_join_views with out_view alone into tensors allocated inside the leg: planes and third-allele records
  join_then_select       tensors.join, then tensors.select over the joined region (its own wait included)

Before timing, the planes of the first two routes are compared for equality.  Per leg: device seconds between two events on torch's
stream around the call (allocation by torch's caching allocator included, as a caller pays it), the wall time of call + wait, the peak
of device memory the call allocates, and for the library's legs the kernel seconds and bytes of brc_join_last_timing (of the filling
call); for join_planes_only also GB/s against the 232 bytes per position and library that the planes kernel must move (116 in, 116
out).  No ratio is written, no threshold gates anything.

    python tools/join_bench.py --out profiles/join_bench.json

--cpu-builds rehearses the script on the CPU builds of the tests (numpy arrays, wall time in place of device time); it writes no file
unless --out is given, and what it prints is no measurement.
"""
import argparse
import ctypes as C
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))

SHAPES = [("config5_tumor200x_1mbp_2x2lib", "tumor200x", 1.0, True), ("config3_wgs30x_4mbp_all_lib_twice", "wgs30x", 4.0, False)]
PLANES = (("ncol", 1), ("depth", 1), ("slotid", 1), ("si", 18), ("sf", 8))


class _Cuda:
    """raw device memory as __cuda_array_interface__, for torch.as_tensor: no copy"""

    def __init__(self, ptr, n_words):
        self.__cuda_array_interface__ = {"shape": (n_words,), "typestr": "<i4", "data": (ptr, False), "version": 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/join_bench.json (none with --cpu-builds)")
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies the regions' lengths (a rehearsal: 0.02)")
    ap.add_argument("--cpu-builds", action="store_true", help="rehearse on the CPU builds of the tests: no measurement")
    a = ap.parse_args()
    import synthgen as gen
    from bam_readcount_amd import capi, tensors
    gen.build()
    gpu = not a.cpu_builds
    if gpu:
        import torch
        lib = capi.load_product()
        join = capi.Join(); select = capi.Select()
        out = a.out or os.path.join(ROOT, "profiles", "join_bench.json")
    else:
        sims = {}
        for name in ("sim", "sim_join", "sim_select"):
            subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", name)], stderr=subprocess.DEVNULL)
            sims[name] = os.path.join(ROOT, "tests", name, "libbrc_%s.so" % (name if name == "sim" else name[4:] + "_sim"))
        lib = capi.Library(sims["sim"])
        join = capi.Join(sims["sim_join"]); select = capi.Select(sims["sim_select"])
        out = a.out
    res = {"box": socket.gethostname(), "device": torch.cuda.get_device_name(0) if gpu else "CPU builds: a rehearsal, no measurement",
           "min_seconds": a.min_seconds, "scale": a.scale,
           "engine_kernel_object_sha256_16": capi.kernel_object_hash(), "join_kernel_object_sha256_16": capi.kernel_object_hash(capi.JOIN_LIB),
           "legs": "alternating round by round; device seconds between torch events around the call; peak_bytes = device memory the call allocates",
           "yardstick_leaves_out": "library renumbering and position rebasing of the records, the synthetic reads, the merged reference slice",
           "shapes": []}

    def words(ptr, n):
        """n 32-bit words at a source's address, where they lie"""
        if gpu:
            return torch.as_tensor(_Cuda(ptr, n), device="cuda") if n else torch.empty(0, dtype=torch.int32, device="cuda")
        return np.ctypeslib.as_array((C.c_int32 * n).from_address(ptr)) if n else np.empty(0, np.int32)

    def empty(*shape):
        return torch.empty(shape, dtype=torch.int32, device="cuda") if gpu else np.empty(shape, np.int32)

    def sync():
        if gpu:
            torch.cuda.synchronize()
    for name, config, mbp, split in SHAPES:
        length = int(mbp * 1e6 * a.scale)
        ref, arrs = gen.generate(length, config, seed=1)
        engines = []
        for half in (0, 1):
            if split:
                idx = np.flatnonzero(np.asarray(arrs["lib"]) // 2 == half)
                sub = capi.select_reads(arrs, idx)
                sub["lib"] = (np.asarray(sub["lib"]) - 2 * half).astype(np.int16)
                eng = capi.Engine(lib, min_mapq=0, min_bq=0, per_lib=True, insertion_centric=True, lib_names=["lib%d" % (2 * half + i) for i in (0, 1)])
            else:
                sub = arrs
                eng = capi.Engine(lib, min_mapq=20, min_bq=13)
            eng.begin_region(0, 0, length, ref); eng.push_reads(sub); eng.upload(); eng.compute()
            engines.append(eng)
        views = [(e.device_view(), e.device_indels()) for e in engines]
        lo = min(int(v.pos0) for v, _ in views); hi = max(int(v.pos0) + int(v.n_pos) for v, _ in views)
        n, L = hi - lo, sum(int(v.n_lib) for v, _ in views)
        src = capi.join_sources(views)
        z = join.sizes(src, lo, n, n)

        def planes_buffers():
            return {k: empty(L * per, n) for k, per in PLANES}, empty(int(z.n_xagg), 16)

        def yardstick():
            bufs, _ = planes_buffers()
            base = 0
            for v, _d in views:
                Ls, P, PS, a0 = int(v.n_lib), int(v.n_pos), int(v.stride), int(v.pos0) - lo
                for k, per in PLANES:
                    if a0 or P != n:                            # (positions this source does not cover)
                        bufs[k][base * per:(base + Ls) * per] = 0x701 if k == "slotid" else 0
                    bufs[k][base * per:(base + Ls) * per, a0:a0 + P] = words(getattr(v, k), Ls * per * PS).reshape(Ls * per, PS)[:, :P]
                base += Ls
            cat = torch.cat if gpu else np.concatenate
            xagg = cat([words(v.xagg, 16 * int(v.n_xagg)) for v, _d in views])
            slots = cat([words(d.slots, 18 * int(d.n_slots)) for _v, d in views])
            return bufs, xagg, slots

        def join_all():
            return tensors.join(engines, join)

        def planes_only():
            bufs, xagg = planes_buffers()
            ptr = (lambda t: t.data_ptr() if t.numel() else None) if gpu else (lambda t: t.ctypes.data if t.size else None)
            v = capi.DeviceView()
            join.views(src, lo, n, n, dest=capi.JoinDest(xagg=ptr(xagg), **{k: ptr(b) for k, b in bufs.items()}), out_view=v,
                       stream=torch.cuda.current_stream().cuda_stream if gpu else None)
            return bufs, v

        def join_then_select():
            J = tensors.join(engines, join)
            return tensors.select(J, select, role=[capi.ROLE_CASE] * (L - L // 2) + [capi.ROLE_CONTROL] * (L // 2), min_depth=10, min_alt=3, min_frac=(1, 20), ctl_max_alt=1)
        legs = [("torch_slice_copies", yardstick), ("join_all", join_all), ("join_planes_only", planes_only), ("join_then_select", join_then_select)]

        def timed(k, fn):
            sync()
            base = 0
            if gpu:
                base = torch.cuda.memory_allocated(); torch.cuda.reset_peak_memory_stats()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            if gpu:
                e0.record()
            o = fn()
            if gpu:
                e1.record()
            sync()
            wall = time.perf_counter() - t0
            x = {"wall_s": wall, "device_s": e0.elapsed_time(e1) * 1e-3 if gpu else wall, "peak_bytes": torch.cuda.max_memory_allocated() - base if gpu else 0}
            if k != "torch_slice_copies":
                x.update(join.last_timing())
            return x, o
        # the two routes' planes, word for word
        _, (wb, wx, wslots) = timed(*legs[0]); _, J = timed(*legs[1])
        same = (lambda p, q: bool(torch.equal(p.reshape(-1), q.reshape(-1).view(torch.int32)))) if gpu else (lambda p, q: np.array_equal(p.reshape(-1), q.reshape(-1).view(np.int32)))
        for k, _per in PLANES:
            assert same(wb[k], J.arrays[k]), "the joined %s differ from the slice copies" % k
        assert int(wx.shape[0]) == 16 * int(z.n_xagg) and int(wslots.shape[0]) == 18 * int(z.n_slots)
        counts = [int(x) & 0xFFFFFFFF for x in (J.counts.cpu().tolist() if gpu else J.counts.tolist())]
        entry = {"shape": name, "config": config, "positions": n, "n_lib": L, "sources": [int(v.n_lib) for v, _ in views], "xagg_records": int(z.n_xagg),
                 "indel_records": int(z.n_slots), "kept_indel_records": counts[0], "seq4_bytes": counts[1], "ref_bytes": int(z.ref_bytes),
                 "planes_bytes_moved": 232 * n * L, "workspace_bytes": int(z.workspace_bytes)}
        del wb, wx, wslots, J
        for k, fn in legs:                                   # warm-up round
            timed(k, fn)
        acc = {k: [] for k, _ in legs}
        own = {k: 0.0 for k, _ in legs}
        while min(own.values()) < a.min_seconds:
            for k, fn in legs:                               # one round: every leg that still needs time, in turn
                if own[k] >= a.min_seconds:
                    continue
                x, _ = timed(k, fn); acc[k].append(x)
                own[k] += x["device_s"]
        for k, rr in acc.items():
            q = len(rr)
            x = {"reps": q, "device_ms": 1e3 * sum(y["device_s"] for y in rr) / q, "device_ms_best": 1e3 * min(y["device_s"] for y in rr),
                 "wall_ms": 1e3 * sum(y["wall_s"] for y in rr) / q, "peak_bytes": max(y["peak_bytes"] for y in rr)}
            if "kernel_s" in rr[0]:
                ks = sum(y["kernel_s"] for y in rr)
                x.update(kernel_ms=1e3 * ks / q, bytes_read=rr[0]["bytes_read"], bytes_written=rr[0]["bytes_written"])
                if k == "join_planes_only" and ks > 0:
                    x["planes_GBps"] = 232e-9 * n * L / (ks / q)
            entry[k] = x
        res["shapes"].append(entry)
        print(json.dumps(entry), flush=True)
        for e in engines:
            e.close()
        del ref, arrs, engines, views, src
        if gpu:
            torch.cuda.empty_cache()
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", out)


if __name__ == "__main__":
    main()
