"""Device-side window summaries against the route a GPU consumer had before them, on one box in one invocation (results:
profiles/bins_bench.json).

Two resident regions, the shapes of tools/select_bench.py: BASELINE config 3 (synthgen wgs30x, 4 Mbp, all libraries) and the shape of
config 5 (tumor200x, 1 Mbp, four libraries).  The legs ALTERNATE round by round until each has at least --min-seconds of its own timed
device work, after a warm-up round:

  expand_whole_then_torch_reduce   the yardstick: tensors.region of depth + ncol + istat over the whole region, then the sums, the maximum
                                   and the covered counts of 1-kb bins by torch index_add_ / scatter_reduce_ over the same bins
  bins_1kb                         tensors.bins(width=1000, thresholds=(10, 20, 30))
  bins_64                          tensors.bins(width=64, ...): one bin per wave
  bins_edges_targets               tensors.bins(edges=...): 200-position targets every 1500 positions, the list a device tensor
  bins_with_hist                   bins_1kb plus a histogram of 256 bars

Before timing, the sums 0..8 and 11 and the covered counts of the first two legs are compared for equality (the yardstick has no indel
table: sums 9 and 10 are bins_1kb's alone).  Per leg: device seconds between two events on torch's stream around the call (allocation
by torch's caching allocator included, as a caller pays it), the wall time of call + wait, the peak of device memory the call allocates
(results included), and for the bins legs the kernel seconds and bytes of brc_bins_last_timing.  No threshold gates anything.

    python tools/bins_bench.py --out profiles/bins_bench.json
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

SHAPES = [("config3_wgs30x_4mbp_all_lib", "wgs30x", 4.0, False), ("config5_tumor200x_1mbp_4lib", "tumor200x", 1.0, True)]
THR = (10, 20, 30)


def torch_reduce(torch, r, rb, width, thr):
    """sums 0..8 and 11 and the covered counts of uniform bins in torch ops over the dense planes of tensors.region"""
    n = r["n"]
    nb = (n + width - 1) // width
    b = torch.arange(n, device=rb.device) // width
    D = r["depth"].view(torch.int32).to(torch.int64)                                   # (counts stay far below 2^31)
    c = r["istat"].view(torch.int32)[:, :, 0, :].to(torch.int64)
    base = torch.arange(1, 5, device=rb.device)[:, None]
    nonref = (c[:, 1:5] * ((rb >= 0)[None, :] & (rb[None, :] + 1 != base))[None]).sum(dim=1)
    vals = torch.cat([D[:, None], r["ncol"].view(torch.int32).to(torch.int64)[:, None], c, nonref[:, None]], dim=1)
    sums = torch.zeros(vals.shape[0], 9, nb, dtype=torch.int64, device=rb.device).index_add_(2, b, vals)
    mx = torch.zeros(D.shape[0], nb, dtype=torch.int64, device=rb.device).scatter_reduce_(1, b.expand(D.shape[0], n), D, "amax")
    cov = torch.zeros(D.shape[0], len(thr), nb, dtype=torch.int64, device=rb.device)
    for t, x in enumerate(thr):
        cov[:, t].index_add_(1, b, (D >= x).to(torch.int64))
    return sums, mx, cov


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bins_bench.json"))
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies the two regions' lengths (a rehearsal: 0.01)")
    a = ap.parse_args()
    import torch
    import synthgen as gen
    from bam_readcount_amd import capi, tensors
    gen.build()
    hip = capi.load_product()
    dense = capi.Dense(); bins = capi.Bins()
    res = {"box": socket.gethostname(), "device": torch.cuda.get_device_name(0), "min_seconds": a.min_seconds,
           "engine_kernel_object_sha256_16": capi.kernel_object_hash(), "dense_kernel_object_sha256_16": capi.kernel_object_hash(capi.DENSE_LIB),
           "bins_kernel_object_sha256_16": capi.kernel_object_hash(capi.BINS_LIB),
           "legs": "alternating round by round; device seconds between torch events around the call; peak_bytes = device memory the call allocates",
           "shapes": []}
    code = np.full(256, -1, np.int8)
    for i, ch in enumerate("ACGT"):
        code[ord(ch)] = code[ord(ch.lower())] = i
    for name, config, mbp, per_lib in SHAPES:
        length = int(mbp * 1e6 * a.scale)
        ref, arrs = gen.generate(length, config, seed=1)
        names = ["lib%d" % i for i in range(gen.CONFIGS[config]["n_libs"])] if per_lib else ()
        opts = dict(min_mapq=0, min_bq=0, per_lib=True, insertion_centric=True, lib_names=names) if per_lib else dict(min_mapq=20, min_bq=13)
        eng = capi.Engine(hip, **opts)
        eng.begin_region(0, 0, length, ref); eng.push_reads(arrs); eng.upload(); eng.compute()
        v, d = eng.device_view(), eng.device_indels()
        P, pos0, L = int(v.n_pos), int(v.pos0), int(v.n_lib)
        rb = torch.from_numpy(code[np.asarray(ref[max(pos0, 0):pos0 + P]).view(np.uint8)].astype(np.int64)).cuda()
        if pos0 < 0:                                         # (the lead position in front of the reference: no reference character)
            rb = torch.cat([torch.full((-pos0,), -1, dtype=torch.int64, device="cuda"), rb])
        targets = np.arange(pos0 + 100, pos0 + P - 200, 1500, dtype=np.int64)
        edges = torch.from_numpy(np.stack([targets, targets + 200], axis=1).reshape(-1).astype(np.int32)).cuda()

        def whole():
            return torch_reduce(torch, tensors.region(eng, dense, want=("depth", "ncol", "istat")), rb, 1000, THR)

        def leg(**kw):
            def f():
                return tensors.bins(eng, bins, thresholds=THR, **kw)
            return f
        legs = [("expand_whole_then_torch_reduce", whole), ("bins_1kb", leg(width=1000, want=("sums", "covered"))),
                ("bins_64", leg(width=64, want=("sums", "covered"))), ("bins_edges_targets", leg(edges=edges, want=("sums", "covered"))),
                ("bins_with_hist", leg(width=1000, hist=256))]

        def timed(k, fn):
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated(); torch.cuda.reset_peak_memory_stats()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(); out = fn(); e1.record()
            torch.cuda.synchronize()
            t = {"wall_s": time.perf_counter() - t0, "device_s": e0.elapsed_time(e1) * 1e-3, "peak_bytes": torch.cuda.max_memory_allocated() - base}
            if k != "expand_whole_then_torch_reduce":
                t.update(bins.last_timing())
            return t, out
        # the two routes' outputs, element for element
        _, (wsum, wmax, wcov) = timed(*legs[0]); _, r = timed(*legs[1])
        gs = r["sums"].view(torch.int64)
        assert torch.equal(gs[:, :9], wsum) and torch.equal(gs[:, 11], wmax) and torch.equal(r["covered"].view(torch.int64), wcov)
        assert int(r["status"].view(torch.int32)[0]) == 0
        n_ins, n_del = int(gs[:, 9].sum()), int(gs[:, 10].sum())
        del wsum, wmax, wcov, r, gs
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
        entry = {"shape": name, "config": config, "positions": P, "view_stride": int(v.stride), "n_lib": L, "thresholds": list(THR),
                 "n_xagg_records": int(v.n_xagg), "n_indel_records": int(d.n_slots), "insertion_reads": n_ins, "deletion_reads": n_del,
                 "targets": int(targets.size)}
        for k, runs in acc.items():
            n = len(runs)
            x = {"reps": n, "device_ms": 1e3 * sum(t["device_s"] for t in runs) / n, "device_ms_best": 1e3 * min(t["device_s"] for t in runs),
                 "wall_ms": 1e3 * sum(t["wall_s"] for t in runs) / n, "peak_bytes": max(t["peak_bytes"] for t in runs)}
            if "kernel_s" in runs[0]:
                ks = sum(t["kernel_s"] for t in runs)
                x.update(kernel_ms=1e3 * ks / n, bytes_read=runs[0]["bytes_read"], bytes_written=runs[0]["bytes_written"],
                         GBps_asked_for=runs[0]["bytes_read"] * n / ks / 1e9)
            entry[k] = x
        for k, _ in legs[1:]:
            entry[k + "_vs_whole_device"] = entry["expand_whole_then_torch_reduce"]["device_ms"] / entry[k]["device_ms"]
        res["shapes"].append(entry)
        print(json.dumps(entry), flush=True)
        eng.close()
        del rb, edges, ref, arrs
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
