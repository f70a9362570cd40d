"""The device-resident indel table against the host route, on one box in one invocation (results:
profiles/indels_bench.json).

For a config-3 region (synthgen wgs30x, all libraries) and the config-5 shape (tumor200x, four libraries, -p -i), computed once on a
BRC_OPT_TEXT_ONLY engine and kept resident, three legs ALTERNATE round by round until each has at least --min-seconds of its own
timed work, after a warm-up round:

  host_fetch       brc_fetch_result as it stands on a text-only engine: the slots cross PCIe, assemble_indels spells and sorts them on
                   the host (wall time of the call; the text-only engine downloads its compact planes in the same call — that is the
                   route a caller has today)
  gather_counts    brc_indels_gather for the two counts alone     \\  seconds between the HIP events around the launches
  gather_all       brc_indels_gather, every destination           /  (brc_indels_last_timing), and the wall time of call + wait

records/s = the region's indel records per second of the leg.  Before timing, the device table is compared with the host route's
list, field by field.

    python tools/indels_bench.py --out profiles/indels_bench.json
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

SHAPES = [
    # name, synthgen config, contig bp, engine options
    ("config3_wgs30x", "wgs30x", "mbp3", dict()),
    ("config5_tumor200x_4lib", "tumor200x", "mbp5", dict(lib_names=["libA", "libB", "libC", "libD"], per_lib=True, insertion_centric=True, min_mapq=20, min_bq=13)),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "indels_bench.json"))
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--mbp3", type=float, default=4.0, help="contig length of the config-3 region, Mbp")
    ap.add_argument("--mbp5", type=float, default=1.0, help="contig length of the config-5 shape, Mbp")
    a = ap.parse_args()
    import torch
    import synthgen as gen
    from bam_readcount_amd import capi, tensors
    gen.build()
    hip = capi.load_product()
    ind = capi.Indels()
    res = {"box": socket.gethostname(), "device": torch.cuda.get_device_name(0), "min_seconds": a.min_seconds,
           "engine_kernel_object_sha256_16": capi.kernel_object_hash(), "indels_kernel_object_sha256_16": capi.kernel_object_hash(capi.INDELS_LIB),
           "legs": "alternating round by round; kernel seconds from HIP events; host_fetch is the wall time of brc_fetch_result on a text-only engine",
           "shapes": []}
    for name, cfg, len_arg, opts in SHAPES:
        length = int(getattr(a, len_arg) * 1e6)
        ref, arrs = gen.generate(length, cfg, seed=7, n_chunks=64)
        eng = capi.Engine(hip, text_only=True, **opts)
        eng.begin_region(0, 0, length, ref); eng.push_reads(arrs); eng.upload(); eng.compute()
        v = eng.device_indels()
        P = int(v.n_pos)
        stream = torch.cuda.current_stream().cuda_stream
        # the device table against the host route's list, field by field
        host = eng.fetch_result()
        t = tensors.indels(eng, ind)
        m, nbytes = t["m"], int(t["alleles"].numel())
        assert m == len(host.indels)
        for k in ("pos", "lib", "len", "rep_read", "rep_qpos"):
            assert t[k].cpu().numpy().astype(np.int64).tolist() == [int(d[k]) & (0xFFFFFFFF if k == "rep_read" else -1) for d in host.indels], k
        assert np.array_equal(t["istat"].cpu().numpy().view(np.uint32), np.array([d["i"] for d in host.indels], np.uint32).reshape(m, 9).T)
        assert np.array_equal(t["fstat"].cpu().numpy().view(np.uint32), np.array([d["f"] for d in host.indels], np.float32).reshape(m, 4).T.copy().view(np.uint32))
        assert bytes(t["alleles"].cpu().numpy()) == "".join(d["allele"] for d in host.indels).encode("latin1")
        del host
        wsb = ind.workspace(v, P)
        ws = torch.empty(max(wsb // 4, 1), dtype=torch.int32, device="cuda")
        counts = torch.zeros(2, dtype=torch.int32, device="cuda")
        dst = {k: t[k].data_ptr() for k in tensors.INDEL_KINDS}

        def host_fetch():
            t0 = time.perf_counter(); r = eng.L.lib.brc_fetch_result(eng.h, eng._res); w = time.perf_counter() - t0
            assert r == 0
            return {"wall_s": w}

        def gather_leg(whole):
            def f():
                t0 = time.perf_counter()
                ind.gather(v, 0, P, workspace=ws.data_ptr(), workspace_bytes=wsb, counts=counts.data_ptr(), cap=m if whole else 0,
                           alleles_cap=nbytes if whole else 0, stream=stream, **(dst if whole else {}))
                w = ind.last_timing()                        # (waits for the launches)
                w["wall_s"] = time.perf_counter() - t0
                return w
            return f
        legs = [("host_fetch", host_fetch), ("gather_counts", gather_leg(False)), ("gather_all", gather_leg(True))]
        for _, fn in legs:                                   # warm-up round
            fn()
        assert counts.cpu().tolist() == [m, nbytes]
        acc = {k: [] for k, _ in legs}
        own = {k: 0.0 for k, _ in legs}
        while min(own.values()) < a.min_seconds:
            for k, fn in legs:                               # one round: every leg that still needs time, in turn
                if own[k] >= a.min_seconds:
                    continue
                w = fn(); acc[k].append(w)
                own[k] += w.get("kernel_s", w["wall_s"])
        entry = {"shape": name, "synthgen": cfg, "contig_bp": length, "options": {k: x for k, x in opts.items() if k != "lib_names"},
                 "n_lib": int(v.n_lib), "n_pos": P, "n_slots": int(v.n_slots), "records": m, "allele_bytes": nbytes, "workspace_bytes": wsb}
        for k, runs in acc.items():
            wall = sum(w["wall_s"] for w in runs)
            e = {"reps": len(runs), "wall_ms": 1e3 * wall / len(runs), "wall_records_per_s": m * len(runs) / wall}
            if "kernel_s" in runs[0]:
                ks = sum(w["kernel_s"] for w in runs)
                e.update(kernel_ms=1e3 * ks / len(runs), kernel_ms_best=1e3 * min(w["kernel_s"] for w in runs), kernel_records_per_s=m * len(runs) / ks)
            entry[k] = e
        entry["gather_all_vs_host_fetch_wall"] = entry["host_fetch"]["wall_ms"] / entry["gather_all"]["wall_ms"]
        res["shapes"].append(entry)
        print(json.dumps(entry), flush=True)
        del t, ws
        eng.close()
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
