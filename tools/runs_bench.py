"""Device-side depth-class intervals against the route a GPU consumer had before them, on one box in one invocation (results:
profiles/runs_bench.json).

Two resident regions, the shapes of tools/select_bench.py: BASELINE config 3 (synthgen wgs30x, 4 Mbp, all libraries) and the shape of
config 5 (tumor200x, 1 Mbp, four libraries).  The legs ALTERNATE round by round until each has at least --min-seconds of its own timed
work, after a warm-up round:

  expand_depth_then_torch_runs   the yardstick: tensors.region of depth over the whole region, then min over the libraries, bucketize, the
                                 neighbours' difference and nonzero in torch
  runs_counts                    brc_runs_find asked for the count and per_class alone (what tensors.runs does first)
  runs_all                       tensors.runs, every class kept: the count, the one wait, the list
  runs_keep_callable             tensors.runs(keep=(the deepest class,), ref_n=True): the callable intervals alone
  runs_then_bins_edges           runs_keep_callable, then tensors.bins(edges=...) over those intervals with the list left where it lies

Before timing, start / end / cls of the first leg and of runs_all are compared for equality.  Per leg: device seconds between two events
on torch's stream around the call (allocation by torch's caching allocator and the one wait included, as a caller pays them), the wall
time of call + wait, the peak of device memory the call allocates (results included), and for the runs legs the kernel seconds and bytes
of brc_runs_last_timing.  No threshold gates anything.

    python tools/runs_bench.py --out profiles/runs_bench.json

--cpu-builds rehearses the script on the CPU builds of the tests (libbrc_sim.so and the sim_* libraries: numpy arrays, torch on the
CPU for the yardstick, wall time in place of device time); it writes no file unless --out is given, and what it prints is no measurement.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))

SHAPES = [("config3_wgs30x_4mbp_all_lib", "wgs30x", 4.0, False, (1, 5, 10, 20)), ("config5_tumor200x_1mbp_4lib", "tumor200x", 1.0, True, (1, 5, 10, 20))]


def torch_runs(torch, depth, cuts):
    """(start, end, cls) of every run of the window in torch ops over the depth planes of tensors.region"""
    D = depth.view(torch.int32).to(torch.int64)                                          # (counts stay far below 2^31)
    c = torch.bucketize(D.min(dim=0).values, torch.tensor(cuts, dtype=torch.int64, device=D.device), right=True)
    b = (c[1:] != c[:-1]).nonzero().reshape(-1) + 1
    zero = torch.zeros(1, dtype=torch.int64, device=D.device)
    start = torch.cat([zero, b]); end = torch.cat([b, zero + c.numel()])
    return start, end, c[start]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/runs_bench.json (none with --cpu-builds)")
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies the two regions' lengths (a rehearsal: 0.01)")
    ap.add_argument("--cpu-builds", action="store_true", help="rehearse on the CPU builds of the tests: no measurement")
    a = ap.parse_args()
    import torch
    import synthgen as gen
    from bam_readcount_amd import capi, tensors
    gen.build()
    gpu = not a.cpu_builds
    if gpu:
        lib = capi.load_product()
        dense = capi.Dense(); bins = capi.Bins(); runs = capi.Runs()
        out = a.out or os.path.join(ROOT, "profiles", "runs_bench.json")
    else:
        sims = {}
        for name in ("sim", "sim_dense", "sim_bins", "sim_runs"):
            subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", name)])
            sims[name] = os.path.join(ROOT, "tests", name, "libbrc_%s.so" % (name if name == "sim" else name[4:] + "_sim"))
        lib = capi.Library(sims["sim"])
        dense = capi.Dense(sims["sim_dense"]); bins = capi.Bins(sims["sim_bins"]); runs = capi.Runs(sims["sim_runs"])
        out = a.out
    res = {"box": socket.gethostname(), "device": torch.cuda.get_device_name(0) if gpu else "CPU builds: a rehearsal, no measurement",
           "min_seconds": a.min_seconds, "scale": a.scale,
           "engine_kernel_object_sha256_16": capi.kernel_object_hash(), "dense_kernel_object_sha256_16": capi.kernel_object_hash(capi.DENSE_LIB),
           "bins_kernel_object_sha256_16": capi.kernel_object_hash(capi.BINS_LIB), "runs_kernel_object_sha256_16": capi.kernel_object_hash(capi.RUNS_LIB),
           "legs": "alternating round by round; device seconds between torch events around the call; peak_bytes = device memory the call allocates",
           "shapes": []}

    def as_torch(x):
        return x if gpu else torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x)

    def sync():
        if gpu:
            torch.cuda.synchronize()
    for name, config, mbp, per_lib, cuts in SHAPES:
        length = int(mbp * 1e6 * a.scale)
        ref, arrs = gen.generate(length, config, seed=1)
        names = ["lib%d" % i for i in range(gen.CONFIGS[config]["n_libs"])] if per_lib else ()
        opts = dict(min_mapq=0, min_bq=0, per_lib=True, insertion_centric=True, lib_names=names) if per_lib else dict(min_mapq=20, min_bq=13)
        eng = capi.Engine(lib, **opts)
        eng.begin_region(0, 0, length, ref); eng.push_reads(arrs); eng.upload(); eng.compute()
        v = eng.device_view()
        P, pos0, L = int(v.n_pos), int(v.pos0), int(v.n_lib)
        top = len(cuts)
        params, keep = capi.runs_params(cuts)
        if gpu:
            ws = torch.empty(max(runs.workspace(P) // 4, 1), dtype=torch.int32, device="cuda")
            cnt = torch.zeros(1, dtype=torch.int32, device="cuda"); per = torch.zeros(top + 2, dtype=torch.int64, device="cuda")
            ptr = lambda t: t.data_ptr()
        else:
            ws = np.empty(max(runs.workspace(P) // 4, 1), np.int32); cnt = np.zeros(1, np.int32); per = np.zeros(top + 2, np.uint64)
            ptr = lambda t: t.ctypes.data

        def whole():
            return torch_runs(torch, as_torch(tensors.region(eng, dense, want=("depth",))["depth"]), cuts)

        def counts():
            runs.find(v, None, params, 0, P, counts=ptr(cnt), per_class=ptr(per), workspace=ptr(ws), stream=torch.cuda.current_stream().cuda_stream if gpu else None)
            return cnt

        def everything():
            return tensors.runs(eng, runs, cuts=cuts)

        def callable_():
            return tensors.runs(eng, runs, cuts=cuts, keep=(top,), ref_n=True)

        def chain():
            r = callable_()
            if gpu:
                e = torch.stack([r["start"], r["end"]], dim=1).reshape(-1).contiguous()
            else:
                e = np.stack([r["start"], r["end"]], axis=1).reshape(-1)
            return tensors.bins(eng, bins, edges=e, thresholds=(cuts[-1],), want=("sums", "covered")) if r["n"] else r
        legs = [("expand_depth_then_torch_runs", whole), ("runs_counts", counts), ("runs_all", everything), ("runs_keep_callable", callable_),
                ("runs_then_bins_edges", chain)]

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
            t = {"wall_s": wall, "device_s": e0.elapsed_time(e1) * 1e-3 if gpu else wall, "peak_bytes": torch.cuda.max_memory_allocated() - base if gpu else 0}
            if k in ("runs_counts", "runs_all", "runs_keep_callable"):
                t.update(runs.last_timing())
            return t, o
        # the two routes' lists, element for element
        _, (ws_, we, wc) = timed(*legs[0]); _, r = timed(*legs[2])
        assert r["n"] == int(ws_.numel())
        for k, w in (("k0", ws_), ("k1", we), ("cls", wc)):
            assert torch.equal(as_torch(r[k]).to(torch.int64), w), k
        n_runs = r["n"]
        _, c = timed(*legs[1])
        assert int(c[0]) == n_runs and int(as_torch(per.view(np.int64) if not gpu else per).sum()) == P
        _, rc = timed(*legs[3])
        n_callable = rc["n"]
        _, rb = timed(*legs[4])
        if n_callable:                                       # every position of a callable interval is at or above the last cut in every library
            cov = as_torch(rb["covered"].view(np.int64) if not gpu else rb["covered"].view(torch.int64))[:, 0, ::2]
            wid = (as_torch(rc["k1"]) - as_torch(rc["k0"])).to(torch.int64)
            assert torch.equal(cov, wid[None, :].expand(L, -1))
        del ws_, we, wc, r, rc, rb
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
        entry = {"shape": name, "config": config, "positions": P, "view_stride": int(v.stride), "n_lib": L, "cuts": list(cuts), "n_runs": n_runs,
                 "n_callable_runs": n_callable, "workspace_bytes": runs.workspace(P)}
        for k, rr in acc.items():
            n = len(rr)
            x = {"reps": n, "device_ms": 1e3 * sum(t["device_s"] for t in rr) / n, "device_ms_best": 1e3 * min(t["device_s"] for t in rr),
                 "wall_ms": 1e3 * sum(t["wall_s"] for t in rr) / n, "peak_bytes": max(t["peak_bytes"] for t in rr)}
            if "kernel_s" in rr[0]:
                ks = sum(t["kernel_s"] for t in rr)
                x.update(kernel_ms=1e3 * ks / n, bytes_read=rr[0]["bytes_read"], bytes_written=rr[0]["bytes_written"],
                         GBps_asked_for=rr[0]["bytes_read"] * n / ks / 1e9)
            entry[k] = x
        for k, _ in legs[1:]:
            entry[k + "_vs_whole_device"] = entry["expand_depth_then_torch_runs"]["device_ms"] / entry[k]["device_ms"]
        res["shapes"].append(entry)
        print(json.dumps(entry), flush=True)
        eng.close()
        del ws, cnt, per, ref, arrs, keep
        if gpu:
            torch.cuda.empty_cache()
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", out)


if __name__ == "__main__":
    main()
