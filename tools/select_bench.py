"""Device-side site selection against the route a GPU consumer had before it, on one box in one invocation (results:
profiles/select_bench.json).

Two resident regions: BASELINE config 3 (synthgen wgs30x, 4 Mbp, all libraries: every library a case library) and the shape of
config 5 (tumor200x, 1 Mbp, four libraries: two case, two control).  The legs ALTERNATE round by round until each has at least
--min-seconds of its own timed device work, after a warm-up round:

  expand_whole_then_torch_filter   tensors.region of depth + istat over the whole region, the predicate in torch ops, nonzero
  select_counts                    brc_select_sites asked for the count alone (what tensors.select does first)
  select_all                       tensors.select: the count, the one wait, the list
  select_all_with_indels           tensors.select with the indel records looked at too (no counterpart in the first leg: information only)
  select_then_sites                tensors.select + tensors.sites(positions=sel["pos"]) of depth + istat

The first four look for bases alone (BRC_SELECT_SNV): that is what the dense planes can answer without the indel table.  Before
timing, the lists of the first leg and of select_all are compared, element for element, reason words included.  Per leg: device
seconds between two events on torch's stream around the call (allocation by torch's caching allocator and the one wait included, as a
caller pays them), the wall time of call + wait, the peak of device memory the call allocates (results included), and for the selector's
legs the kernel seconds and bytes of brc_select_last_timing — read against a streaming copy's 6.0-6.3 TB/s.  No
threshold gates anything.

    python tools/select_bench.py --out profiles/select_bench.json
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

# name, synthgen config, Mbp, engine options, roles, thresholds
SHAPES = [("config3_wgs30x_4mbp_all_lib", "wgs30x", 4.0, None, dict(min_depth=10, min_alt=3, min_frac=(1, 10))),
          ("config5_tumor200x_1mbp_2case_2control", "tumor200x", 1.0, [1, 1, 2, 2],
           dict(min_depth=20, min_alt=2, min_frac=(1, 50), ctl_min_depth=10, ctl_max_alt=0, ctl_max_frac=(1, 100)))]


def torch_filter(torch, r, rb, role, kw):
    """the header's predicate for bases in torch ops over the dense planes of tensors.region -> (idx int64, why int64)"""
    D = r["depth"].view(torch.int32).to(torch.int64)[:, None, :]                     # (counts stay far below 2^31)
    c = r["istat"].view(torch.int32)[:, 1:5, 0, :].to(torch.int64)
    fn, fd = kw.get("min_frac", (0, 1)); cn, cd = kw.get("ctl_max_frac", (1, 1))
    case_ok = (D >= kw["min_depth"]) & (c >= kw["min_alt"]) & (c * fd >= fn * D)
    ctl_ok = (D >= kw.get("ctl_min_depth", 0)) & (c <= kw.get("ctl_max_alt", 2 ** 32 - 1)) & (c * cd <= cn * D)
    role = torch.tensor(role, device=D.device)
    ok = case_ok[role == 1].any(dim=0) & ctl_ok[role == 2].all(dim=0)
    b = torch.arange(4, device=D.device)[:, None]
    why = ((ok & (rb >= 0)[None, :] & (rb[None, :] != b)).to(torch.int64) << b).sum(dim=0)
    idx = why.nonzero().reshape(-1)
    return idx, why[idx]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_bench.json"))
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies the two regions' lengths (a rehearsal: 0.01)")
    a = ap.parse_args()
    import torch
    import synthgen as gen
    from bam_readcount_amd import capi, tensors
    gen.build()
    hip = capi.load_product()
    dense = capi.Dense(); panel = capi.Panel(); select = capi.Select()
    res = {"box": socket.gethostname(), "device": torch.cuda.get_device_name(0), "min_seconds": a.min_seconds,
           "engine_kernel_object_sha256_16": capi.kernel_object_hash(), "dense_kernel_object_sha256_16": capi.kernel_object_hash(capi.DENSE_LIB),
           "panel_kernel_object_sha256_16": capi.kernel_object_hash(capi.PANEL_LIB), "select_kernel_object_sha256_16": capi.kernel_object_hash(capi.SELECT_LIB),
           "legs": "alternating round by round; device seconds between torch events around the call; peak_bytes = device memory the call allocates",
           "shapes": []}
    code = np.full(256, -1, np.int8)
    for i, ch in enumerate("ACGT"):
        code[ord(ch)] = code[ord(ch.lower())] = i
    for name, config, mbp, role, kw in SHAPES:
        length = int(mbp * 1e6 * a.scale)
        ref, arrs = gen.generate(length, config, seed=1)
        per_lib = role is not None
        names = ["lib%d" % i for i in range(gen.CONFIGS[config]["n_libs"])] if per_lib else ()
        opts = dict(min_mapq=0, min_bq=0, per_lib=True, insertion_centric=True, lib_names=names) if per_lib else dict(min_mapq=20, min_bq=13)
        eng = capi.Engine(hip, **opts)
        eng.begin_region(0, 0, length, ref); eng.push_reads(arrs); eng.upload(); eng.compute()
        v, d = eng.device_view(), eng.device_indels()
        P, pos0, L = int(v.n_pos), int(v.pos0), int(v.n_lib)
        roles = role or [1] * L
        assert len(roles) == L
        rb = torch.from_numpy(code[np.asarray(ref[pos0:pos0 + P]).view(np.uint8)].astype(np.int64)).cuda()
        params, keep = capi.select_params(roles, capi.SELECT_SNV, kw["min_depth"], kw["min_alt"], kw.get("min_frac", (0, 1)), kw.get("ctl_min_depth", 0),
                                          kw.get("ctl_max_alt", 2 ** 32 - 1), kw.get("ctl_max_frac", (1, 1)))
        ws = torch.empty(max(select.workspace(v, d, P) // 4, 1), dtype=torch.int32, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int32, device="cuda")

        def whole():
            return torch_filter(torch, tensors.region(eng, dense, want=("depth", "istat")), rb, roles, kw)

        def counts():
            select.sites(v, d, params, 0, P, counts=cnt.data_ptr(), workspace=ws.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
            return cnt

        def sel(indel):
            def f():
                return tensors.select(eng, select, role=roles, indel=indel, **kw)
            return f

        def chain():
            s = tensors.select(eng, select, role=roles, indel=False, **kw)
            return tensors.sites(eng, panel, positions=s["pos"], want=("depth", "istat"))
        legs = [("expand_whole_then_torch_filter", whole), ("select_counts", counts), ("select_all", sel(False)), ("select_all_with_indels", sel(True)),
                ("select_then_sites", chain)]

        def timed(k, fn):
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated(); torch.cuda.reset_peak_memory_stats()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(); out = fn(); e1.record()
            torch.cuda.synchronize()
            t = {"wall_s": time.perf_counter() - t0, "device_s": e0.elapsed_time(e1) * 1e-3, "peak_bytes": torch.cuda.max_memory_allocated() - base}
            if k in ("select_counts", "select_all", "select_all_with_indels"):
                t.update(select.last_timing())
            return t, out
        # the two routes' lists, element for element
        _, (widx, wwhy) = timed(*legs[0]); _, s = timed(*legs[2])
        assert s["n"] == int(widx.numel()) and torch.equal(s["idx"].to(torch.int64), widx) and torch.equal(s["why"].to(torch.int64), wwhy)
        n_sel = s["n"]
        _, c = timed(*legs[1])
        assert int(c[0]) == n_sel
        n_sel_indels = timed(*legs[3])[1]["n"]
        del widx, wwhy, s
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
        entry = {"shape": name, "config": config, "positions": P, "view_stride": int(v.stride), "n_lib": L, "roles": roles, "thresholds": kw,
                 "n_xagg_records": int(v.n_xagg), "n_indel_records": int(d.n_slots), "n_selected": n_sel, "n_selected_with_indels": n_sel_indels,
                 "workspace_bytes": select.workspace(v, d, P)}
        for k, runs in acc.items():
            n = len(runs)
            x = {"reps": n, "device_ms": 1e3 * sum(t["device_s"] for t in runs) / n, "device_ms_best": 1e3 * min(t["device_s"] for t in runs),
                 "wall_ms": 1e3 * sum(t["wall_s"] for t in runs) / n, "peak_bytes": max(t["peak_bytes"] for t in runs)}
            if "kernel_s" in runs[0]:
                ks = sum(t["kernel_s"] for t in runs)
                x.update(kernel_ms=1e3 * ks / n, bytes_read=runs[0]["bytes_read"], bytes_written=runs[0]["bytes_written"],
                         GBps_asked_for=runs[0]["bytes_read"] * n / ks / 1e9)
            entry[k] = x
        for k in ("select_counts", "select_all", "select_all_with_indels", "select_then_sites"):
            entry[k + "_vs_whole_device"] = entry["expand_whole_then_torch_filter"]["device_ms"] / entry[k]["device_ms"]
        res["shapes"].append(entry)
        print(json.dumps(entry), flush=True)
        eng.close()
        del rb, ws, cnt, ref, arrs, keep
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
