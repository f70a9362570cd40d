"""The device-side consensus caller against what a consumer can do without it, on one box in one invocation (results:
profiles/cons_bench.json).

Two resident regions: BASELINE config 3 (synthgen wgs30x, 4 Mbp, all libraries as one) and the shape of config 5 (tumor200x, 1 Mbp, four
libraries, insertion-centric).  The indel table is gathered and normalised once, outside the timing.  The legs ALTERNATE round by
round until each has at least --min-seconds of its own timed device work, after a warm-up round:

  region_torch_aligned   the yardstick, what a consumer can do today: tensors.region(want=("istat",)) — 216 of the 312 dense bytes per
                         position and library — and the rule in torch operations over the four base counts.  It computes the ALIGNED
                         string only, places no insertion, and cannot count the reads that carry a deletion across a position.
  cons_aligned           tensors.consensus(aligned=True): no wait
  cons_with_insertions   tensors.consensus(): the sequence with insertions placed and deletions left out, with its one wait

Before timing, the yardstick's string is compared for equality with cons_aligned over an EMPTY table (d = 0 everywhere, which is all
the yardstick can know), and with cons_aligned over the real table on every position no deletion covers.  Per leg: device seconds
between two events on torch's stream around the call (allocation by torch's caching allocator included, as a caller pays it), the wall
time of call + wait, the peak of device memory the call allocates, and for the library's legs the kernel seconds and bytes of
brc_cons_last_timing (of the filling call).  No ratio is written, no threshold gates anything.

    python tools/cons_bench.py --out profiles/cons_bench.json

--cpu-builds rehearses the script on the CPU builds of the tests (numpy arrays, wall time in place of device time); it writes no file
unless --out is given, and what it prints is no measurement.
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

SHAPES = [("config3_wgs30x_4mbp_all_lib", "wgs30x", 4.0, False), ("config5_tumor200x_1mbp_4lib", "tumor200x", 1.0, True)]
RULE = dict(min_depth=8, min_count=2, frac=(1, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/cons_bench.json (none with --cpu-builds)")
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies the regions' lengths (a rehearsal: 0.02)")
    ap.add_argument("--cpu-builds", action="store_true", help="rehearse on the CPU builds of the tests: no measurement")
    a = ap.parse_args()
    import synthgen as gen
    from bam_readcount_amd import capi, consensus, tensors
    gen.build()
    gpu = not a.cpu_builds
    if gpu:
        import torch
        lib = capi.load_product()
        dense, indels, inorm, cons = capi.Dense(), capi.Indels(), capi.INorm(), consensus.Cons()
        out = a.out or os.path.join(ROOT, "profiles", "cons_bench.json")
    else:
        sims = {}
        for d, so in (("sim", "libbrc_sim.so"), ("sim_dense", "libbrc_dense_sim.so"), ("sim_indels", "libbrc_indels_sim.so"), ("sim_inorm", "libbrc_inorm_sim.so"),
                      ("cpu_cons", "libbrc_cons_sim.so")):
            subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", d)], stderr=subprocess.DEVNULL)
            sims[d] = os.path.join(ROOT, "tests", d, so)
        lib = capi.Library(sims["sim"])
        dense, indels, inorm, cons = capi.Dense(sims["sim_dense"]), capi.Indels(sims["sim_indels"]), capi.INorm(sims["sim_inorm"]), consensus.Cons(sims["cpu_cons"])
        out = a.out
    res = {"box": socket.gethostname(), "device": torch.cuda.get_device_name(0) if gpu else "CPU builds: a rehearsal, no measurement",
           "min_seconds": a.min_seconds, "scale": a.scale, "rule": dict(RULE, frac=list(RULE["frac"]), ins_min_count=2, ins_frac=[1, 20]),
           "engine_kernel_object_sha256_16": capi.kernel_object_hash(), "cons_kernel_object_sha256_16": capi.kernel_object_hash(consensus.CONS_LIB),
           "legs": "alternating round by round; device seconds between torch events around the call; peak_bytes = device memory the call allocates",
           "yardstick_leaves_out": "the reads that carry a deletion across a position, the insertions, the liftover offsets",
           "shapes": []}
    xp = torch if gpu else np
    lut = np.frombuffer(consensus.CONS_IUPAC.encode(), np.uint8).copy(); lut[0] = ord("N")
    num, den = RULE["frac"]

    def sync():
        if gpu:
            torch.cuda.synchronize()

    def host(x):
        return x.cpu().numpy() if gpu else np.asarray(x)
    for name, config, mbp, per_lib in SHAPES:
        length = int(mbp * 1e6 * a.scale)
        ref, arrs = gen.generate(length, config, seed=1)
        if per_lib:
            eng = capi.Engine(lib, min_mapq=0, min_bq=0, per_lib=True, insertion_centric=True, lib_names=["lib%d" % i for i in range(4)])
        else:
            eng = capi.Engine(lib, min_mapq=20, min_bq=13)
        eng.begin_region(0, 0, length, ref); eng.push_reads(arrs); eng.upload(); eng.compute()
        v = eng.device_view()
        n, L = int(v.n_pos), int(v.n_lib)
        table = tensors.normalize_indels(eng, inorm, tensors.indels(eng, indels))
        empty = tensors.indels(eng, indels, beg0=int(v.pos0), end=int(v.pos0))           # (a window of no positions: a table of no records)
        assert empty["m"] == 0
        kw = dict(RULE, ins_min_count=2, ins_frac=(1, 20), ins_centric=per_lib)
        codes = (torch.from_numpy(lut).cuda() if gpu else lut)
        weights = (torch.tensor([1, 2, 4, 8], device="cuda") if gpu else np.array([1, 2, 4, 8]))[:, None]

        def yardstick():
            r = tensors.region(eng, dense, want=("istat",))
            c = r["istat"][:, 1:5, 0, :]
            c = (c.to(torch.int64) if gpu else c.astype(np.int64)).sum(0)
            T = c.sum(0)
            q = (c >= RULE["min_count"]) & (c * den >= num * T)
            mask = (q * weights).sum(0)
            mask = xp.where(T >= RULE["min_depth"], mask, xp.zeros_like(mask))
            return codes[mask]

        def cons_aligned():
            return tensors.consensus(eng, cons, table=table, aligned=True, want=("seq",), **kw)

        def cons_with_insertions():
            return tensors.consensus(eng, cons, table=table, want=("seq", "off"), **kw)
        legs = [("region_torch_aligned", yardstick), ("cons_aligned", cons_aligned), ("cons_with_insertions", cons_with_insertions)]

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
            if k != "region_torch_aligned":
                x.update(cons.last_timing())
            return x, o
        # the outputs first: the yardstick's string equals the aligned call over an empty table, and over the real one wherever d == 0
        _, ys = timed(*legs[0])
        e = tensors.consensus(eng, cons, table=empty, aligned=True, want=("seq",), **kw)
        full = tensors.consensus(eng, cons, table=table, aligned=True, want=("seq", "cnt"), **kw)
        ys, es, fs, d = host(ys), host(e["seq"]), host(full["seq"]), host(full["cnt"]).view(np.uint32)[consensus.CONS_C_DEL]
        assert np.array_equal(ys, es), "the yardstick's string differs from the aligned call over an empty table"
        assert np.array_equal(ys[d == 0], fs[d == 0]), "the yardstick's string differs from the aligned call where no deletion covers"
        wi = tensors.consensus(eng, cons, table=table, want=("seq", "ins_rec", "call"), **kw)
        entry = {"shape": name, "config": config, "positions": n, "n_lib": L, "table_records": int(table["m"]), "xagg_records": int(v.n_xagg),
                 "positions_under_deletions": int((d != 0).sum()), "positions_deleted": int((host(wi["call"]) == ord("-")).sum()),
                 "insertions_placed": int((host(wi["ins_rec"]).view(np.uint32) != consensus.CONS_NO_INS).sum()), "sequence_bytes": int(host(wi["seq"]).size),
                 "differs_from_yardstick_at": int((ys != fs).sum()), "workspace_bytes": cons.workspace(v, n, int(table["m"]))}
        del ys, es, fs, d, e, full, wi
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
                if ks > 0:
                    x["GBps_of_bytes_asked_and_written"] = 1e-9 * (rr[0]["bytes_read"] + rr[0]["bytes_written"]) / (ks / q)
            entry[k] = x
        res["shapes"].append(entry)
        print(json.dumps(entry), flush=True)
        eng.close()
        del ref, arrs, eng, table, empty
        if gpu:
            torch.cuda.empty_cache()
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", out)


if __name__ == "__main__":
    main()
