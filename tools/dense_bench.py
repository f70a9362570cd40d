"""Device-resident results against the host route, on one box in one invocation (results: profiles/dense_bench.json).

For a config-3 region (synthgen wgs30x, all libraries) and the config-5 shape (tumor200x, four libraries, -p -i), computed once and
kept resident, four legs ALTERNATE round by round until each has at least --min-seconds of its own timed work, after a warm-up round:

  host_fetch       brc_fetch_result as it stands: the compact planes cross PCIe, expand_slots builds the dense planes on host threads
                   (wall time of the call)
  dense_if         brc_dense_expand, istat + fstat        \\
  dense_metrics    brc_dense_expand, metrics alone         >  seconds between the HIP events around the launches (brc_dense_last_timing),
  dense_all        brc_dense_expand, every destination    /   and the wall time of call + wait beside them

GB/s = bytes read + written by the planes kernel (brc_dense_last_timing) per kernel second, and as a share of the 8 TB/s of HBM;
events/s = the region's pileup events per second of the leg.  Before timing, the device planes of a window are compared with the
host route's, bit for bit.

    python tools/dense_bench.py --out profiles/dense_bench.json
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

HBM_PEAK = 8.0e12
SHAPES = [
    # name, synthgen config, contig bp, engine options
    ("config3_wgs30x", "wgs30x", "mbp3", dict()),
    ("config5_tumor200x_4lib", "tumor200x", "mbp5", dict(lib_names=["libA", "libB", "libC", "libD"], per_lib=True, insertion_centric=True, min_mapq=20, min_bq=13)),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_bench.json"))
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--mbp3", type=float, default=4.0, help="contig length of the config-3 region, Mbp")
    ap.add_argument("--mbp5", type=float, default=1.0, help="contig length of the config-5 shape, Mbp")
    ap.add_argument("--check-positions", type=int, default=200_000)
    a = ap.parse_args()
    import torch
    import synthgen as gen
    from bam_readcount_amd import capi
    gen.build()
    hip = capi.load_product()
    dense = capi.Dense()
    res = {"box": socket.gethostname(), "device": torch.cuda.get_device_name(0), "min_seconds": a.min_seconds, "hbm_peak_Bps": HBM_PEAK,
           "engine_kernel_object_sha256_16": capi.kernel_object_hash(), "dense_kernel_object_sha256_16": capi.kernel_object_hash(capi.DENSE_LIB),
           "legs": "alternating round by round; kernel seconds from HIP events; GB/s = bytes read + written by the planes kernel", "shapes": []}
    for name, cfg, len_arg, opts in SHAPES:
        length = int(getattr(a, len_arg) * 1e6)
        ref, arrs = gen.generate(length, cfg, seed=7, n_chunks=64)
        eng = capi.Engine(hip, **opts)
        eng.begin_region(0, 0, length, ref); eng.push_reads(arrs); eng.upload(); eng.compute()
        n_events, n_positions = eng.counts()
        v = eng.device_view()
        P, L = int(v.n_pos), int(v.n_lib)
        stream = torch.cuda.current_stream().cuda_stream

        def dev(planes, dt):
            return torch.empty((planes, P), dtype=dt, device="cuda")
        bufs = {"ncol": dev(L, torch.int32), "depth": dev(L, torch.int32), "unavail": dev(1, torch.int32), "istat": dev(L * 54, torch.int32),
                "fstat": dev(L * 24, torch.float32), "metrics": dev(L * 78, torch.float32)}
        wants = {"dense_if": ("istat", "fstat"), "dense_metrics": ("metrics",), "dense_all": tuple(bufs)}

        def host_fetch():
            t0 = time.perf_counter(); r = eng.L.lib.brc_fetch_result(eng.h, eng._res); t = time.perf_counter() - t0
            assert r == 0
            return {"wall_s": t}

        def dense_leg(kinds):
            def f():
                t0 = time.perf_counter()
                dense.expand(v, 0, P, P, stream=stream, **{k: bufs[k].data_ptr() for k in kinds})
                t = dense.last_timing()                      # (waits for the launches)
                t["wall_s"] = time.perf_counter() - t0
                return t
            return f
        legs = [("host_fetch", host_fetch)] + [(k, dense_leg(w)) for k, w in wants.items()]
        # the device planes of a window against the host route's, bit for bit
        host = eng.fetch_result()
        dense_leg(wants["dense_all"])()
        n_chk = min(P, a.check_positions)
        for k, want in (("istat", host.istat), ("fstat", host.fstat), ("depth", host.depth), ("ncol", host.ncol)):
            got = bufs[k][:, P - n_chk:].cpu().numpy().view(np.uint32)
            assert np.array_equal(got, want.view(np.uint32).reshape(got.shape[0], P)[:, P - n_chk:]), k
        del host
        for _, fn in legs:                                   # warm-up round
            fn()
        acc = {k: [] for k, _ in legs}
        own = {k: 0.0 for k, _ in legs}
        while min(own.values()) < a.min_seconds:
            for k, fn in legs:                               # one round: every leg that still needs time, in turn
                if own[k] >= a.min_seconds:
                    continue
                t = fn(); acc[k].append(t)
                own[k] += t.get("kernel_s", t["wall_s"])
        entry = {"shape": name, "synthgen": cfg, "contig_bp": length, "options": {k: x for k, x in opts.items() if k != "lib_names"}, "n_lib": L,
                 "n_pos": P, "view_stride": int(v.stride), "n_xagg_records": int(v.n_xagg), "events": n_events, "positions": n_positions,
                 "dense_bytes": 4 * P * L * 78}
        for k, runs in acc.items():
            wall = sum(t["wall_s"] for t in runs)
            e = {"reps": len(runs), "wall_ms": 1e3 * wall / len(runs), "wall_events_per_s": n_events * len(runs) / wall}
            if "kernel_s" in runs[0]:
                ks = sum(t["kernel_s"] for t in runs); by = sum(t["bytes_read"] + t["bytes_written"] for t in runs)
                e.update(kernel_ms=1e3 * ks / len(runs), kernel_ms_best=1e3 * min(t["kernel_s"] for t in runs), bytes_read=runs[0]["bytes_read"],
                         bytes_written=runs[0]["bytes_written"], GBps=by / ks / 1e9, share_of_hbm_peak=by / ks / HBM_PEAK,
                         kernel_events_per_s=n_events * len(runs) / ks)
            entry[k] = e
        entry["dense_all_vs_host_fetch_wall"] = entry["host_fetch"]["wall_ms"] / entry["dense_all"]["wall_ms"]
        res["shapes"].append(entry)
        print(json.dumps(entry), flush=True)
        del bufs
        eng.close()
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
