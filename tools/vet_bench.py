"""The device-side candidate filter against the route a GPU consumer had before it, on one box in one invocation (results:
profiles/vet_bench.json).

Two resident regions, the shapes behind tools/select_bench.py: BASELINE config 3 (synthgen wgs30x, 4 Mbp, all libraries) and the shape of
config 5 (tumor200x, 1 Mbp, four libraries).  The candidates are what tensors.select finds (bases only); the list stays where it lies.
The legs ALTERNATE round by round until each has at least --min-seconds of its own timed work, after a warm-up round:

  sites_then_torch_predicate   the yardstick: tensors.sites of the list with depth, istat and metrics (six buckets x 13 columns per element
                               and library), then the header's predicate in torch ops — the reference's and the variants' buckets gathered
                               by index, the eighteen tests, the OR over the libraries
  vet_fail_keep                tensors.vet(want=("fail", "keep"))
  vet_all                      tensors.vet with vals as well

Before timing, fail and keep of the first leg and of vet_all are compared for equality.  Per leg: device seconds between two events on
torch's stream around the call (allocation by torch's caching allocator included, as a caller pays it), the wall time of call + wait, the
peak of device memory the call allocates (results included), and for the vet legs the kernel seconds and bytes of brc_vet_last_timing.
No threshold gates anything.

    python tools/vet_bench.py --out profiles/vet_bench.json

--cpu-builds rehearses the script on the CPU builds of the tests (libbrc_sim.so and the sim_* libraries: numpy arrays, torch on the CPU
for the yardstick, wall time in place of device time); it writes no file unless --out is given, and what it prints is no measurement.
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

SELECT = dict(min_depth=8, min_alt=2, min_frac=(1, 50))
SHAPES = [("config3_wgs30x_4mbp_all_lib", "wgs30x", 4.0, False), ("config5_tumor200x_1mbp_4lib", "tumor200x", 1.0, True)]
# (name, column of the thirteen, variant-side threshold, reference-side threshold): "<" tests
SIDE_TESTS = (("READPOS", 6, "min_var_readpos", "min_ref_readpos"), ("DIST3", 12, "min_var_dist3", "min_ref_dist3"), ("BQ", 2, "min_var_bq", "min_ref_bq"),
              ("MAPQ", 1, "min_var_mapq", "min_ref_mapq"), ("RL", 11, "min_var_rl", "min_ref_rl"))


def torch_predicate(torch, capi, r, rb, alt, t):
    """include/brc_vet.h's predicate in torch ops over tensors.sites' planes -> (fail int64 [L, 4, n], keep int64 [n]); rb: the reference's
    base 0..3 per element (-1: none), alt: the asked bases per element"""
    B = capi.VET_BIT
    i64 = torch.int64
    D = r["depth"].view(torch.int32).to(i64)[:, None, :]                                  # [L, 1, n]  (counts stay far below 2^31)
    ist = r["istat"].view(torch.int32).to(i64)                                           # [L, 6, 9, n]
    m = r["metrics"]                                                                     # [L, 6, 13, n]
    L, n = D.shape[0], D.shape[2]
    ri = (rb.clamp(min=0) + 1)[None, None, None, :]
    Cr = ist[:, :, 0, :].gather(1, ri[:, :, 0, :].expand(L, 1, n))                       # [L, 1, n]
    mr = m.gather(1, ri.expand(L, 1, 13, n))[:, 0]                                       # [L, 13, n]
    Cv, Pv, Mv = ist[:, 1:5, 0, :], ist[:, 1:5, 3, :], ist[:, 1:5, 4, :]                 # [L, 4, n]
    mv = m[:, 1:5]                                                                       # [L, 4, 13, n]
    S = Pv + Mv
    f = torch.zeros_like(Cv)
    f |= (D < t["min_depth"]).to(i64) * B["DEPTH"]
    f |= (Cv < t["min_var_count"]).to(i64) * B["VAR_COUNT"]
    f |= (Cv * t["freq_den"] < t["freq_num"] * D).to(i64) * B["VAR_FREQ"]
    f |= ((S >= t["min_strand_reads"]) & (torch.minimum(Pv, Mv) * t["strand_den"] < t["strand_num"] * S)).to(i64) * B["STRAND"]
    var, ref = Cv > 0, (Cr >= t["min_ref_reads"])
    for name, c, kv, kr in SIDE_TESTS:
        f |= (var & (mv[:, :, c] < t[kv])).to(i64) * B["VAR_" + name]
        f |= (ref & (mr[:, None, c] < t[kr])).to(i64) * B["REF_" + name]
    f |= (var & (mv[:, :, 8] > t["max_var_mmqs"])).to(i64) * B["VAR_MMQS"]
    both = var & ref
    f |= (both & ((mv[:, :, 8] - mr[:, None, 8]) > t["max_mmqs_diff"])).to(i64) * B["MMQS_DIFF"]
    f |= (both & ((mr[:, None, 1] - mv[:, :, 1]) > t["max_mapq_diff"])).to(i64) * B["MAPQ_DIFF"]
    f |= (both & ((mr[:, None, 11] - mv[:, :, 11]) > (torch.tensor(t["max_rl_diff"], dtype=torch.float32, device=m.device) * mr[:, None, 11]))).to(i64) * B["RL_DIFF"]
    b = torch.arange(4, device=m.device)[None, :, None]
    judged = ((rb >= 0)[None, None, :] & (rb[None, None, :] != b) & (((alt[None, None, :] >> b) & 1) != 0)).expand(L, 4, n)
    fail = torch.where(judged, f, torch.full_like(f, capi.VET_NOT_ASKED))
    fail = torch.where((rb < 0)[None, None, :].expand(L, 4, n), torch.full_like(f, capi.VET_NO_SITE), fail)
    keep = (((fail == 0).any(dim=0)).to(i64) << b[0]).sum(dim=0)
    return fail, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/vet_bench.json (none with --cpu-builds)")
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies the two regions' lengths (a rehearsal: 0.02)")
    ap.add_argument("--cpu-builds", action="store_true", help="rehearse on the CPU builds of the tests: no measurement")
    a = ap.parse_args()
    import torch
    import synthgen as gen
    from bam_readcount_amd import capi, tensors
    gen.build()
    gpu = not a.cpu_builds
    if gpu:
        lib = capi.load_product()
        panel = capi.Panel(); select = capi.Select(); vet = capi.Vet()
        out = a.out or os.path.join(ROOT, "profiles", "vet_bench.json")
    else:
        sims = {}
        for name in ("sim", "sim_panel", "sim_select", "sim_vet"):
            subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", name)])
            sims[name] = os.path.join(ROOT, "tests", name, "libbrc_%s.so" % (name if name == "sim" else name[4:] + "_sim"))
        lib = capi.Library(sims["sim"])
        panel = capi.Panel(sims["sim_panel"]); select = capi.Select(sims["sim_select"]); vet = capi.Vet(sims["sim_vet"])
        out = a.out
    t = dict(capi.VET_DEFAULTS)
    res = {"box": socket.gethostname(), "device": torch.cuda.get_device_name(0) if gpu else "CPU builds: a rehearsal, no measurement",
           "min_seconds": a.min_seconds, "scale": a.scale, "thresholds": t, "select": {k: list(x) if isinstance(x, tuple) else x for k, x in SELECT.items()},
           "engine_kernel_object_sha256_16": capi.kernel_object_hash(), "vet_kernel_object_sha256_16": capi.kernel_object_hash(capi.VET_LIB),
           "panel_kernel_object_sha256_16": capi.kernel_object_hash(capi.PANEL_LIB), "select_kernel_object_sha256_16": capi.kernel_object_hash(capi.SELECT_LIB),
           "legs": "alternating round by round; device seconds between torch events around the call; peak_bytes = device memory the call allocates",
           "shapes": []}
    code = np.full(256, -1, np.int64)
    for i, ch in enumerate("ACGT"):
        code[ord(ch)] = code[ord(ch.lower())] = i

    def as_torch(x):
        return x if gpu else torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x)

    def sync():
        if gpu:
            torch.cuda.synchronize()
    for name, config, mbp, per_lib in SHAPES:
        length = int(mbp * 1e6 * a.scale)
        ref, arrs = gen.generate(length, config, seed=1)
        names = ["lib%d" % i for i in range(gen.CONFIGS[config]["n_libs"])] if per_lib else ()
        opts = dict(min_mapq=0, min_bq=0, per_lib=True, insertion_centric=True, lib_names=names) if per_lib else dict(min_mapq=20, min_bq=13)
        eng = capi.Engine(lib, **opts)
        eng.begin_region(0, 0, length, ref); eng.push_reads(arrs); eng.upload(); eng.compute()
        v = eng.device_view()
        P, pos0, L = int(v.n_pos), int(v.pos0), int(v.n_lib)
        sel = tensors.select(eng, select, indel=False, **SELECT)
        n = sel["n"]
        assert n > 0, "the selection is empty: nothing to vet"
        rb_all = torch.from_numpy(code[np.asarray(ref[pos0:pos0 + P]).view(np.uint8)])
        rb_all = rb_all.cuda() if gpu else rb_all
        idx64 = as_torch(sel["idx"]).to(torch.int64)
        rb = rb_all[idx64]
        alt = as_torch(sel["why"]).to(torch.int64)

        def yardstick():
            r = tensors.sites(eng, panel, positions=sel["pos"], want=("depth", "istat", "metrics"))
            return torch_predicate(torch, capi, {k: as_torch(r[k]) for k in ("depth", "istat", "metrics")}, rb, alt, t)

        def fail_keep():
            return tensors.vet(eng, vet, idx=sel["idx"], alt=sel["why"], want=("fail", "keep"), **t)

        def everything():
            return tensors.vet(eng, vet, idx=sel["idx"], alt=sel["why"], **t)
        legs = [("sites_then_torch_predicate", yardstick), ("vet_fail_keep", fail_keep), ("vet_all", everything)]

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
            if k != "sites_then_torch_predicate":
                x.update(vet.last_timing())
            return x, o
        # the two routes' words, element for element
        _, (wf, wk) = timed(*legs[0]); _, r = timed(*legs[2])
        gf = as_torch(r["fail"]).to(torch.int64) & 0xFFFFFFFF
        assert torch.equal(gf, wf), "fail differs at %r" % ((gf != wf).nonzero()[:4].tolist(),)
        assert torch.equal(as_torch(r["keep"]).to(torch.int64), wk)
        n_kept = int((wk != 0).sum())
        judged = int((wf < capi.VET_NOT_ASKED).sum())
        del wf, wk, r, gf
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
        entry = {"shape": name, "config": config, "positions": P, "n_lib": L, "candidates": n, "judged_alleles": judged, "kept": n_kept,
                 "n_xagg": int(v.n_xagg), "workspace_bytes": vet.workspace(v, n)}
        for k, rr in acc.items():
            m = len(rr)
            x = {"reps": m, "device_ms": 1e3 * sum(y["device_s"] for y in rr) / m, "device_ms_best": 1e3 * min(y["device_s"] for y in rr),
                 "wall_ms": 1e3 * sum(y["wall_s"] for y in rr) / m, "peak_bytes": max(y["peak_bytes"] for y in rr)}
            if "kernel_s" in rr[0]:
                ks = sum(y["kernel_s"] for y in rr)
                x.update(kernel_ms=1e3 * ks / m, bytes_read=rr[0]["bytes_read"], bytes_written=rr[0]["bytes_written"])
            entry[k] = x
        for k, _ in legs[1:]:
            entry[k + "_vs_yardstick_device"] = entry["sites_then_torch_predicate"]["device_ms"] / entry[k]["device_ms"]
        res["shapes"].append(entry)
        print(json.dumps(entry), flush=True)
        eng.close()
        del ref, arrs, sel
        if gpu:
            torch.cuda.empty_cache()
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", out)


if __name__ == "__main__":
    main()
