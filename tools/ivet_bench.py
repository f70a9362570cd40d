"""The device-side indel candidate filter against the route a GPU consumer had before it, on one box in one invocation (DESIGN.md 6k;
results: profiles/ivet_bench.json).

Two resident regions, the shapes behind tools/vet_bench.py: BASELINE config 3 (synthgen wgs30x, 4 Mbp, all libraries: one library, so
no control test can fail) and the shape of config 5 (tumor200x, 1 Mbp, four libraries, two of them control).  The list is what
tensors.select finds (insertions and deletions only, the control libraries IGNORED as tensors.vet_indels' docstring says); it stays
where it lies.  The legs ALTERNATE round by round until each has at least --min-seconds of its own timed work, after a warm-up round:

  table_sites_then_torch_predicate   the yardstick: tensors.indels (the sorted table: one wait for its sizes), tensors.sites at the
                                     records' positions with depth, istat and metrics (six buckets x 13 columns per record and library),
                                     then the header's predicate in torch ops — the record's library and the reference's bucket gathered
                                     by index, the seventeen tests, the control depths, and the same-allele match: the texts padded to
                                     one width (one wait for the width), numbered by torch.unique, and the control records' verdicts
                                     reduced per (position, length, text); keep by a search of the passing records' positions in the list
  indels_then_ivet_all               the same scope through the library: tensors.indels (with its wait), then tensors.vet_indels(idx=, why=)
                                     with every destination
  ivet_fail_keep                     tensors.vet_indels(idx=, why=, want=("fail", "keep")) over a table gathered once, OUTSIDE the timed part
  ivet_all                           the same with vals and ctl_count as well

Only the first two legs do the same work (table included); the last two time the filter alone, and no ratio is written.
Before timing, fail and keep of the first leg and of ivet_all are compared for equality.  Per leg: device seconds between two events on torch's
stream around the call (allocation by torch's caching allocator included, as a caller pays it), the wall time of call + wait, the peak
of device memory the call allocates (results included), and for the ivet legs the kernel seconds (the kernels alone) and bytes of
brc_ivet_last_timing.  No threshold gates anything.

    python tools/ivet_bench.py --out profiles/ivet_bench.json

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

SHAPES = [("config3_wgs30x_4mbp_all_lib", "wgs30x", 4.0, False, None), ("config5_tumor200x_1mbp_4lib", "tumor200x", 1.0, True, [1, 1, 2, 2])]
# (name, column of the thirteen, variant-side threshold or None, reference-side threshold): "<" tests
SIDE_TESTS = (("READPOS", 6, "min_var_readpos", "min_ref_readpos"), ("DIST3", 12, "min_var_dist3", "min_ref_dist3"), ("BQ", 2, None, "min_ref_bq"),
              ("MAPQ", 1, "min_var_mapq", "min_ref_mapq"), ("RL", 11, "min_var_rl", "min_ref_rl"))
# capi.IVET_DEFAULTS but for: a control test of its own, and thresholds the generator's reads can meet (its reads are 100 .. 150 bases and
# its indels sit anywhere in a read, one read each), so that records pass and the list's OR path runs
OVERRIDES = dict(ctl_min_depth=8, ctl_max_count=1, ctl_frac_num=1, ctl_frac_den=50, min_var_count=1, freq_num=1, freq_den=100, min_var_rl=60.0, min_ref_rl=60.0,
                 min_var_readpos=0.05, min_var_dist3=0.05, max_rl_diff=0.5)
SELECT = dict(snv=False, indel=True, min_depth=8, min_alt=1, min_frac=(1, 100))


def torch_predicate(torch, capi, tab, planes, rb_all, pos0, role, t, idx, why):
    """include/brc_ivet.h's predicate in torch ops over the table and tensors.sites' planes at the records' positions -> (fail int64 [m],
    keep int64 [n]); idx, why: select's list (strictly ascending) as int64.
    tab: pos, lib, len, istat [9, m], metrics [13, m], allele_off, alleles; planes: depth [L, m], istat [L, 6, 9, m], metrics [L, 6, 13, m];
    rb_all: the reference's base 0..3 per plane position (-1: none); role: int64 [L]"""
    B = capi.IVET_BIT
    i64 = torch.int64
    dev = tab["pos"].device
    pos, lib, ln = tab["pos"].to(i64), tab["lib"].to(i64), tab["len"].to(i64)
    m = pos.shape[0]
    L = planes["depth"].shape[0]
    rb = rb_all[pos - pos0]
    Dall = planes["depth"].view(torch.int32).to(i64)                                     # [L, m]
    ar = torch.arange(m, device=dev)
    D = Dall[lib, ar]
    ri = rb.clamp(min=0) + 1
    Cr = planes["istat"].view(torch.int32)[lib, ri, 0, ar].to(i64)
    mr = planes["metrics"][lib, ri, :, ar].T                                             # [13, m]
    ist = tab["istat"].view(torch.int32).to(i64)
    mv = tab["metrics"]
    Cv, Pv, Mv = ist[0], ist[3], ist[4]
    S = Pv + Mv
    f = torch.zeros_like(Cv)
    f |= (D < t["min_depth"]).to(i64) * B["DEPTH"]
    f |= (Cv < t["min_var_count"]).to(i64) * B["VAR_COUNT"]
    f |= (Cv * t["freq_den"] < t["freq_num"] * D).to(i64) * B["VAR_FREQ"]
    f |= ((S >= t["min_strand_reads"]) & (torch.minimum(Pv, Mv) * t["strand_den"] < t["strand_num"] * S)).to(i64) * B["STRAND"]
    var, ref = Cv > 0, (Cr >= t["min_ref_reads"])
    for name, c, kv, kr in SIDE_TESTS:
        if kv:
            f |= (var & (mv[c] < t[kv])).to(i64) * B["VAR_" + name]
        f |= (ref & (mr[c] < t[kr])).to(i64) * B["REF_" + name]
    f |= (var & (mv[8] > t["max_var_mmqs"])).to(i64) * B["VAR_MMQS"]
    both = var & ref
    f |= (both & ((mv[8] - mr[8]) > t["max_mmqs_diff"])).to(i64) * B["MMQS_DIFF"]
    f |= (both & ((mr[1] - mv[1]) > t["max_mapq_diff"])).to(i64) * B["MAPQ_DIFF"]
    f |= (both & ((mr[11] - mv[11]) > (torch.tensor(t["max_rl_diff"], dtype=torch.float32, device=dev) * mr[11]))).to(i64) * B["RL_DIFF"]
    ctl = role == capi.ROLE_CONTROL
    if bool(ctl.any()) and m:
        f |= (Dall[ctl] < t["ctl_min_depth"]).any(dim=0).to(i64) * B["CTL_DEPTH"]
        # the same-allele match: texts padded to one width, numbered, and the control records' verdicts reduced per (position, length, text)
        off = tab["allele_off"].view(torch.int32).to(i64)
        n_text = off[1:] - off[:-1]
        W = int(n_text.max())                                                            # (a wait: the width is data)
        col = torch.arange(W, device=dev)[None, :]
        inside = col < n_text[:, None]
        A = tab["alleles"].shape[0]
        chars = tab["alleles"][(off[:-1, None] + col).clamp(max=max(A - 1, 0))].to(i64) * inside
        key = torch.cat([pos[:, None], ln[:, None], chars], dim=1)
        _, group = torch.unique(key, dim=0, return_inverse=True)
        is_ctl = ctl[lib]
        fails = is_ctl & ~((Cv <= t["ctl_max_count"]) & (Cv * t["ctl_frac_den"] <= t["ctl_frac_num"] * D))
        veto = torch.zeros(int(group.max()) + 1, dtype=i64, device=dev).scatter_reduce(0, group, fails.to(i64), "amax")
        f |= veto[group] * B["CTL_ALLELE"]
    judged = (ln != 0) & (role[lib] == capi.ROLE_CASE) & (rb >= 0)
    fail = torch.where(judged, f, torch.full_like(f, capi.IVET_NOT_ASKED))
    fail = torch.where((ln != 0) & (role[lib] == capi.ROLE_CASE) & (rb < 0), torch.full_like(f, capi.IVET_NO_SITE), fail)
    # keep: the passing records' kinds at the list elements of their positions (a strictly ascending list: one element each)
    n = idx.shape[0]
    keep = torch.zeros(n, dtype=i64, device=dev)
    if n and m:
        k = pos - pos0
        j = torch.searchsorted(idx, k).clamp(max=n - 1)
        kind = torch.where(ln > 0, capi.WHY_INS, capi.WHY_DEL)
        hit = (fail == 0) & (idx[j] == k) & ((why[j] & kind) != 0)
        for bit in (capi.WHY_INS, capi.WHY_DEL):
            keep |= torch.zeros_like(keep).scatter_reduce(0, j, (hit & (kind == bit)).to(i64), "amax") * bit
    return fail, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/ivet_bench.json (none with --cpu-builds)")
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
        panel = capi.Panel(); indels = capi.Indels(); ivet = capi.IVet(); select = capi.Select()
        out = a.out or os.path.join(ROOT, "profiles", "ivet_bench.json")
    else:
        sims = {}
        for name in ("sim", "sim_panel", "sim_indels", "sim_ivet", "sim_select"):
            subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", name)], stderr=subprocess.DEVNULL)
            sims[name] = os.path.join(ROOT, "tests", name, "libbrc_%s.so" % (name if name == "sim" else name[4:] + "_sim"))
        lib = capi.Library(sims["sim"])
        panel = capi.Panel(sims["sim_panel"]); indels = capi.Indels(sims["sim_indels"]); ivet = capi.IVet(sims["sim_ivet"]); select = capi.Select(sims["sim_select"])
        out = a.out
    t = dict(capi.IVET_DEFAULTS, **OVERRIDES)
    res = {"box": socket.gethostname(), "device": torch.cuda.get_device_name(0) if gpu else "CPU builds: a rehearsal, no measurement",
           "min_seconds": a.min_seconds, "scale": a.scale, "thresholds": t, "select": {k: list(x) if isinstance(x, tuple) else x for k, x in SELECT.items()},
           "engine_kernel_object_sha256_16": capi.kernel_object_hash(), "ivet_kernel_object_sha256_16": capi.kernel_object_hash(capi.IVET_LIB),
           "panel_kernel_object_sha256_16": capi.kernel_object_hash(capi.PANEL_LIB), "indels_kernel_object_sha256_16": capi.kernel_object_hash(capi.INDELS_LIB),
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
    for name, config, mbp, per_lib, role in SHAPES:
        length = int(mbp * 1e6 * a.scale)
        ref, arrs = gen.generate(length, config, seed=1)
        names = ["lib%d" % i for i in range(gen.CONFIGS[config]["n_libs"])] if per_lib else ()
        opts = dict(min_mapq=0, min_bq=0, per_lib=True, insertion_centric=True, lib_names=names) if per_lib else dict(min_mapq=20, min_bq=13)
        eng = capi.Engine(lib, **opts)
        eng.begin_region(0, 0, length, ref); eng.push_reads(arrs); eng.upload(); eng.compute()
        v = eng.device_view()
        P, pos0, L = int(v.n_pos), int(v.pos0), int(v.n_lib)
        role = role if role is not None and len(role) == L else None
        rb_all = torch.from_numpy(code[np.asarray(ref[pos0:pos0 + P]).view(np.uint8)])
        rb_all = rb_all.cuda() if gpu else rb_all
        role_t = torch.tensor(role if role is not None else [capi.ROLE_CASE] * L, dtype=torch.int64, device=rb_all.device)
        table = tensors.indels(eng, indels)                    # the ivet legs' table: gathered once, where it stays
        m = table["m"]
        assert m > 0, "the table is empty: nothing to vet"
        sel_role = None if role is None else [r if r == capi.ROLE_CASE else capi.ROLE_IGNORE for r in role]
        sel = tensors.select(eng, select, role=sel_role, **SELECT)           # the list: candidates of the case libraries, where it lies
        n = sel["n"]
        assert n > 0, "the selection is empty: no list to keep"
        idx64, why64 = as_torch(sel["idx"]).to(torch.int64), as_torch(sel["why"]).to(torch.int64)

        def yardstick():
            tab = tensors.indels(eng, indels, want=("pos", "lib", "len", "istat", "metrics", "allele_off", "alleles"))
            r = tensors.sites(eng, panel, positions=tab["pos"], want=("depth", "istat", "metrics"))
            return torch_predicate(torch, capi, {k: as_torch(x) for k, x in tab.items() if not isinstance(x, int)},
                                   {k: as_torch(r[k]) for k in ("depth", "istat", "metrics")}, rb_all, pos0, role_t, t, idx64, why64)

        def gather_and_all():
            return tensors.vet_indels(eng, ivet, tensors.indels(eng, indels), idx=sel["idx"], why=sel["why"], role=role, **t)

        def fail_keep():
            return tensors.vet_indels(eng, ivet, table, idx=sel["idx"], why=sel["why"], role=role, want=("fail", "keep"), **t)

        def everything():
            return tensors.vet_indels(eng, ivet, table, idx=sel["idx"], why=sel["why"], role=role, **t)
        legs = [("table_sites_then_torch_predicate", yardstick), ("indels_then_ivet_all", gather_and_all), ("ivet_fail_keep", fail_keep), ("ivet_all", everything)]

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
            if k != "table_sites_then_torch_predicate":
                x.update(ivet.last_timing())
            return x, o
        # the two routes' words, record for record
        _, (wf, wk) = timed(*legs[0]); _, r = timed(*legs[3])
        gf = as_torch(r["fail"]).to(torch.int64) & 0xFFFFFFFF
        assert torch.equal(gf, wf), "fail differs at %r" % ((gf != wf).nonzero()[:4].tolist(),)
        assert torch.equal(as_torch(r["keep"]).to(torch.int64), wk), "keep differs"
        kept = int((wk != 0).sum())
        bits = {name: int(((wf < capi.IVET_NOT_ASKED) & ((wf & b) != 0)).sum()) for name, b in capi.IVET_BIT.items()}
        judged = int((wf < capi.IVET_NOT_ASKED).sum()); passed = int((wf == 0).sum())
        vetoed = int(((wf < capi.IVET_NOT_ASKED) & ((wf & capi.IVET_BIT["CTL_ALLELE"]) != 0)).sum())
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
        entry = {"shape": name, "config": config, "positions": P, "n_lib": L, "records": m, "records_x_libraries": m * L, "judged": judged, "passed": passed,
                 "vetoed_by_ctl_allele": vetoed, "failed_per_test": bits, "list_elements": n, "kept_elements": kept, "role": role, "n_xagg": int(v.n_xagg), "workspace_bytes": ivet.workspace(v, m)}
        for k, rr in acc.items():
            q = len(rr)
            x = {"reps": q, "device_ms": 1e3 * sum(y["device_s"] for y in rr) / q, "device_ms_best": 1e3 * min(y["device_s"] for y in rr),
                 "wall_ms": 1e3 * sum(y["wall_s"] for y in rr) / q, "peak_bytes": max(y["peak_bytes"] for y in rr)}
            if "kernel_s" in rr[0]:
                ks = sum(y["kernel_s"] for y in rr)
                x.update(kernel_ms=1e3 * ks / q, bytes_read=rr[0]["bytes_read"], bytes_written=rr[0]["bytes_written"])
            entry[k] = x
        res["shapes"].append(entry)
        print(json.dumps(entry), flush=True)
        eng.close()
        del ref, arrs, table, sel
        if gpu:
            torch.cuda.empty_cache()
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", out)


if __name__ == "__main__":
    main()
