"""Device-resident site panels against the only route the dense library offers a site list, on one box in one invocation (DESIGN.md
6e; results: profiles/panel_bench.json).

bench.py's site layout (--mode sites: synthgen wgs30x, all libraries, every site's reads and reference laid on a virtual axis of 384
positions per site, the lines announced with brc_region_windows), computed once and kept resident, in two shapes: the 100 000
one-position lines themselves, and windows of 200 positions around each of them.  Three legs ALTERNATE round by round until each has
at least --min-seconds of its own timed work, after a warm-up round:

  expand_whole_then_index_select   tensors.region over the whole axis (istat + fstat) + torch.index_select at the listed positions
  panel_gather                     tensors.sites of a device-resident list, istat + fstat
  panel_gather_metrics             tensors.sites of the same list, metrics alone

Per leg: device seconds between two events on torch's stream around the call (allocation by torch's caching allocator included, as a
caller pays it), the wall time of call + wait, the peak of device memory the call allocates (results included), and for the panel
legs the kernel seconds and bytes of brc_panel_last_timing.  Before timing, the panel's planes are compared with the first leg's,
bit for bit, and the status word is read.  No threshold gates anything.

    python tools/panel_bench.py --out profiles/panel_bench.json
"""
import argparse
import json
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))

SHAPES = [("sites_1", 0, 1), ("windows_200", 100, 100)]       # name, positions before the line, positions from the line on


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "panel_bench.json"))
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--sites", type=int, default=100_000)
    ap.add_argument("--contig-mbp", type=float, default=10.0, help="contig the sites are drawn from (the virtual axis has 384 positions per site whatever it is)")
    a = ap.parse_args()
    import torch
    import bench
    import synthgen as gen
    from bam_readcount_amd import capi, tensors
    gen.build()
    hip = capi.load_product()
    dense = capi.Dense(); panel = capi.Panel()
    res = {"box": socket.gethostname(), "device": torch.cuda.get_device_name(0), "min_seconds": a.min_seconds, "sites": a.sites,
           "contig_bp": int(a.contig_mbp * 1e6), "engine_kernel_object_sha256_16": capi.kernel_object_hash(),
           "dense_kernel_object_sha256_16": capi.kernel_object_hash(capi.DENSE_LIB), "panel_kernel_object_sha256_16": capi.kernel_object_hash(capi.PANEL_LIB),
           "legs": "alternating round by round; device seconds between torch events around the call; peak_bytes = device memory the call allocates", "shapes": []}
    length = int(a.contig_mbp * 1e6)
    ref, arrs = gen.generate(length, "wgs30x", seed=1)
    sites = np.sort(np.random.default_rng(3).integers(200, length - 200, a.sites))
    sub, vref, _events, vbeg0 = bench.site_batch(np, capi, arrs, ref, sites)
    del arrs, ref
    for name, before, after in SHAPES:
        b = (vbeg0 - before).astype(np.int32); e = (vbeg0 + after).astype(np.int32)
        eng = capi.Engine(hip)
        eng.begin_region(0, 0, len(vref), vref); eng.push_reads(sub); eng.region_windows(b, e); eng.upload(); eng.compute()
        v = eng.device_view()
        P, pos0 = int(v.n_pos), int(v.pos0)
        cnt = (e - b).astype(np.int64)
        pos = np.repeat(b.astype(np.int64), cnt) + (np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt))
        dpos = torch.from_numpy(pos.astype(np.int32)).cuda()
        didx = (dpos - pos0).to(torch.int64)

        def whole():
            r = tensors.region(eng, dense, want=("istat", "fstat"))
            return {k: torch.index_select(r[k].view(torch.int32), 3, didx) for k in ("istat", "fstat")}

        def gather(want):
            def f():
                return tensors.sites(eng, panel, positions=dpos, want=want)
            return f
        legs = [("expand_whole_then_index_select", whole), ("panel_gather", gather(("istat", "fstat"))), ("panel_gather_metrics", gather(("metrics",)))]

        def timed(k, fn):
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated(); torch.cuda.reset_peak_memory_stats()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(); out = fn(); e1.record()
            torch.cuda.synchronize()
            t = {"wall_s": time.perf_counter() - t0, "device_s": e0.elapsed_time(e1) * 1e-3, "peak_bytes": torch.cuda.max_memory_allocated() - base}
            if k != "expand_whole_then_index_select":
                t.update(panel.last_timing())
            return t, out
        # the panel's planes against the whole-axis route's, bit for bit; the list's verdict
        _, w = timed(*legs[0]); _, g = timed(*legs[1])
        for k in ("istat", "fstat"):
            assert torch.equal(g[k].view(torch.int32), w[k]), k
        assert int(g["status"].cpu().view(torch.int32)[0]) == 0
        del w, g
        for k, fn in legs:                                   # warm-up round
            timed(k, fn)
        acc = {k: [] for k, _ in legs}
        own = {k: 0.0 for k, _ in legs}
        while min(own.values()) < a.min_seconds:
            for k, fn in legs:                               # one round: every leg that still needs time, in turn
                if own[k] >= a.min_seconds:
                    continue
                t, _ = timed(k, fn); acc[k].append(t)
                own[k] += t["device_s"]
        entry = {"shape": name, "window": [before, after], "n_listed": int(pos.size), "axis_positions": P, "view_stride": int(v.stride), "n_lib": int(v.n_lib),
                 "n_xagg_records": int(v.n_xagg)}
        for k, runs in acc.items():
            n = len(runs)
            x = {"reps": n, "device_ms": 1e3 * sum(t["device_s"] for t in runs) / n, "device_ms_best": 1e3 * min(t["device_s"] for t in runs),
                 "wall_ms": 1e3 * sum(t["wall_s"] for t in runs) / n, "peak_bytes": max(t["peak_bytes"] for t in runs)}
            if "kernel_s" in runs[0]:
                ks = sum(t["kernel_s"] for t in runs)
                x.update(kernel_ms=1e3 * ks / n, bytes_read=runs[0]["bytes_read"], bytes_written=runs[0]["bytes_written"],
                         GBps_written=runs[0]["bytes_written"] * n / ks / 1e9)
            entry[k] = x
        for k in ("panel_gather", "panel_gather_metrics"):
            entry[k + "_vs_whole_device"] = entry["expand_whole_then_index_select"]["device_ms"] / entry[k]["device_ms"]
        res["shapes"].append(entry)
        print(json.dumps(entry), flush=True)
        eng.close()
        del dpos, didx
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
