"""The device-side indel normalisation against what a consumer did before it, on one box in one invocation (results:
profiles/inorm_bench.json).

Two resident regions, the shapes behind tools/ivet_bench.py: BASELINE config 3 (synthgen wgs30x, 4 Mbp, all libraries) and the shape
of config 5 (tumor200x, 1 Mbp, four libraries).  The legs ALTERNATE round by round until each has at least --min-seconds of its own
timed work, after a warm-up round:

  table_to_host_then_numpy     the yardstick: the gathered table copied to the host, the left steps of include/brc_inorm.h as a
                               vectorised numpy loop over all records at once (one pass per step), the normalised texts padded to one
                               width, the classes by numpy.unique over (position, library, length, text), the integer sums by add.at
  normalize_all                tensors.normalize_indels over a table gathered once, OUTSIDE the timed part: every destination (its one
                               wait for the merged sizes included)
  normalize_src_only           the same with want=(): the per-record arrays and the counts, no merged table
  indels_then_normalize_all    tensors.indels (with its wait), then tensors.normalize_indels with every destination

The first two do the same work (a table that lies on the device in, a normalised table out — on the host for the yardstick, on the
device for the library); no ratio is written.  Before timing, the two routes' npos, shift and, per input record, the position, length
and read count of the merged record it went into are compared for equality.  Per leg: device seconds between two events on torch's
stream around the call (allocation by torch's caching allocator included, as a caller pays it), the wall time of call + wait, the peak
of device memory the call allocates, and for the library's legs the kernel seconds and bytes of brc_inorm_last_timing (of the filling
call).  No threshold gates anything.

    python tools/inorm_bench.py --out profiles/inorm_bench.json

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
MAX_SHIFT = 1024


def host_normalize(tab, ref, ref_lo, ref_hi, first, max_shift):
    """include/brc_inorm.h over a gathered table (every record judged) in numpy -> (npos, shift, per record: the merged record's read
    count, the number of merged records)"""
    pos, lib, ln = (tab[k].astype(np.int64) for k in ("pos", "lib", "len"))
    off, text = tab["allele_off"].astype(np.int64)[:-1], tab["alleles"]
    m = pos.size
    refa = np.frombuffer(ref, np.uint8) if isinstance(ref, (bytes, bytearray)) else np.asarray(ref, np.uint8)
    fold = np.zeros(256, np.uint8)
    for c in b"ACGT":
        fold[c] = fold[c | 32] = c

    def R(p):                                                   # the raw character, 0: none
        ok = (p >= ref_lo) & (p < ref_hi) & (p < refa.size)
        return np.where(ok, refa[np.clip(p, 0, refa.size - 1)], 0).astype(np.uint8)
    L, ins = np.abs(ln), ln > 0
    p, s, ti = pos.copy(), np.zeros(m, np.int64), L - 1
    floor = max(first, ref_lo)
    act = np.arange(m)
    while act.size:
        pa = p[act]
        own = ins[act] | (ti[act] >= 0)
        tc = np.where(own, text[off[act] + 1 + np.maximum(ti[act], 0)], R(pa + L[act]))
        rc = fold[R(pa)]
        ok = (rc != 0) & (rc == fold[tc]) & (s[act] < max_shift) & (pa - 1 >= floor)
        act = act[ok]
        p[act] -= 1; s[act] += 1; ti[act] -= 1
        wrap = act[ins[act] & (ti[act] < 0)]
        ti[wrap] = L[wrap] - 1
    W = int(L.max()) if m else 0
    col = np.arange(W)[None, :]
    inside = col < L[:, None]
    src_ins = off[:, None] + 1 + (col - s[:, None]) % np.maximum(L, 1)[:, None]
    src_del = off[:, None] + 1 + col - s[:, None]
    own = ins[:, None] | (col >= s[:, None])
    chars = np.where(own, text[np.clip(np.where(ins[:, None], src_ins, src_del), 0, max(text.size - 1, 0))], R(p[:, None] + 1 + col)) * inside
    key = np.concatenate([p[:, None], lib[:, None], ln[:, None], chars.astype(np.int64)], axis=1)
    _, group = np.unique(key, axis=0, return_inverse=True)
    group = group.reshape(-1)
    mm = int(group.max()) + 1 if m else 0
    ist = np.zeros((9, mm), np.uint64)
    for c in range(9):
        np.add.at(ist[c], group, tab["istat"][c].astype(np.uint64))
    fst = np.zeros((4, mm), np.float32)
    for c in range(4):
        np.add.at(fst[c], group, tab["fstat"][c])               # (unbuffered: in input order)
    return p, s, (ist[0] & 0xFFFFFFFF)[group], mm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/inorm_bench.json (none with --cpu-builds)")
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies the two regions' lengths (a rehearsal: 0.02)")
    ap.add_argument("--cpu-builds", action="store_true", help="rehearse on the CPU builds of the tests: no measurement")
    a = ap.parse_args()
    import synthgen as gen
    from bam_readcount_amd import capi, tensors
    gen.build()
    gpu = not a.cpu_builds
    if gpu:
        import torch
        lib = capi.load_product()
        indels = capi.Indels(); inorm = capi.INorm()
        out = a.out or os.path.join(ROOT, "profiles", "inorm_bench.json")
    else:
        sims = {}
        for name in ("sim", "sim_indels", "sim_inorm"):
            subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", name)], stderr=subprocess.DEVNULL)
            sims[name] = os.path.join(ROOT, "tests", name, "libbrc_%s.so" % (name if name == "sim" else name[4:] + "_sim"))
        lib = capi.Library(sims["sim"])
        indels = capi.Indels(sims["sim_indels"]); inorm = capi.INorm(sims["sim_inorm"])
        out = a.out
    res = {"box": socket.gethostname(), "device": torch.cuda.get_device_name(0) if gpu else "CPU builds: a rehearsal, no measurement",
           "min_seconds": a.min_seconds, "scale": a.scale, "max_shift": MAX_SHIFT,
           "engine_kernel_object_sha256_16": capi.kernel_object_hash(), "inorm_kernel_object_sha256_16": capi.kernel_object_hash(capi.INORM_LIB),
           "indels_kernel_object_sha256_16": capi.kernel_object_hash(capi.INDELS_LIB),
           "legs": "alternating round by round; device seconds between torch events around the call; peak_bytes = device memory the call allocates",
           "shapes": []}

    def host(x):
        return x.cpu().numpy() if gpu else x

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
        d = eng.device_indels()
        table = tensors.indels(eng, indels)                    # the table: gathered once, where it stays
        m = table["m"]
        assert m > 0, "the table is empty: nothing to normalise"
        keys = ("pos", "lib", "len", "istat", "fstat", "allele_off", "alleles")

        def yardstick():
            return host_normalize({k: host(table[k]) for k in keys}, ref, int(d.ref_lo), int(d.ref_hi), table["first"], MAX_SHIFT)

        def everything():
            return tensors.normalize_indels(eng, inorm, table, max_shift=MAX_SHIFT)

        def src_only():
            return tensors.normalize_indels(eng, inorm, table, max_shift=MAX_SHIFT, want=())

        def gather_and_all():
            return tensors.normalize_indels(eng, inorm, tensors.indels(eng, indels), max_shift=MAX_SHIFT)
        legs = [("table_to_host_then_numpy", yardstick), ("normalize_all", everything), ("normalize_src_only", src_only), ("indels_then_normalize_all", gather_and_all)]

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
            if k != "table_to_host_then_numpy":
                x.update(inorm.last_timing())
            return x, o
        # the two routes, record for record
        _, (wp, ws, wc, wmm) = timed(*legs[0]); _, r = timed(*legs[1])
        gp, gs, gg = (host(r["src"][k]).astype(np.int64) for k in ("npos", "shift", "group"))
        assert np.array_equal(gp, wp) and np.array_equal(gs, ws), "npos or shift differs at %r" % (np.nonzero((gp != wp) | (gs != ws))[0][:4].tolist(),)
        assert r["m"] == wmm and (gg >= 0).all(), (r["m"], wmm)
        assert np.array_equal(host(r["istat"]).astype(np.int64)[0][gg], wc.astype(np.int64)) and np.array_equal(host(r["pos"]).astype(np.int64)[gg], wp), "merged records differ"
        assert np.array_equal(host(r["len"]).astype(np.int64)[gg], host(table["len"]).astype(np.int64))
        flags = host(r["src"]["flags"]).astype(np.int64)
        entry = {"shape": name, "config": config, "positions": int(d.n_pos), "n_lib": int(d.n_lib), "records": m, "merged_records": wmm, "shifted_records": int((ws > 0).sum()),
                 "largest_shift": int(ws.max()), "steps": int(ws.sum()), "records_at_limit": int((flags & capi.INORM_LIMIT != 0).sum()),
                 "records_at_edge": int((flags & capi.INORM_EDGE != 0).sum()), "largest_class": int(host(r["members"]).astype(np.int64).max()),
                 "workspace_bytes": inorm.workspace(table["n"], m)}
        del wp, ws, wc, r, gp, gs, gg
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
            entry[k] = x
        res["shapes"].append(entry)
        print(json.dumps(entry), flush=True)
        eng.close()
        del ref, arrs, table
        if gpu:
            torch.cuda.empty_cache()
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", out)


if __name__ == "__main__":
    main()
