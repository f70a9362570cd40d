"""Device-side BGZF inflate against the host path, on one box in one invocation (results: profiles/inflate_bench.json).

  (a) the members of a synthetic tumour-depth BAM piece (config 3's data: tumor200x reads) through libbrc_inflate_hip.so, at about
      1 MB, 26 MB (what auto_chunk of the command line aims at) and 250 MB of compressed bytes: GB/s of OUTPUT for the kernel alone
      (events around the launch) and for the whole call (chain walk, H2D, kernel, D2H), from pageable and from page-locked memory;
  (b) the same members through the host path as it stands — brcio::Bgzf, libdeflate when present, 16 threads
      (tools/inflate_host_bench.cpp) — interleaved with (a) size by size;
  (c) --e2e: tools/e2e_configs.py's tumour leg (config 5) and site leg (config 4) with the switch off and on, off/on interleaved.

Every figure: one warm-up pass, then passes until at least --min-seconds of timed work.  The 250-MB piece is the 26-MB piece's
members repeated (members are independent of each other: the work per member is the same).

    python tools/inflate_bench.py --out profiles/inflate_bench.json
"""
import argparse
import ctypes as C
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools")); sys.path.insert(0, os.path.join(ROOT, "tools", "fuzz"))


def make_piece(workdir, target_bytes):
    """A BAM of tumor200x reads (synthgen, the generator of bench.py's config 3) of about target_bytes, written with 64-KB blocks."""
    import bamio
    import synthgen as gen
    import inflate_members as im
    raw = b""
    length = 60_000
    while True:
        ref, arrs = gen.generate(length, "tumor200x", seed=7, n_chunks=8)
        path = os.path.join(workdir, "piece.bam")
        bamio.write_bam(path, [("chr1", length)], arrs, np.zeros(len(arrs["pos"]), int), block_bytes=64000)
        raw = open(path, "rb").read()
        if len(raw) >= target_bytes or length >= 2_000_000:
            break
        length = int(length * min(8.0, 1.15 * target_bytes / max(len(raw), 1))) + 1000
    members, _ = im.split_members(raw, decode=False)
    return members


def chain_of(members, target_bytes):
    out, n, k = [], 0, 0
    while n < target_bytes:
        m = members[k % len(members)]; out.append(m); n += len(m); k += 1
    return b"".join(out), k


def timed(fn, min_s):
    fn()
    t0 = time.perf_counter(); reps = 0; acc = []
    while True:
        acc.append(fn()); reps += 1
        s = time.perf_counter() - t0
        if s >= min_s:
            return reps, s, acc


def e2e_legs(a, work):
    """(c): tools/e2e_configs.py's two legs — run once each, validated, files kept — then the leg's own command line timed to /dev/null
    with BRC_CLI_TIMING=1, switch off and on INTERLEAVED (off, on, off, on, ...), so that both sides see the same box in the same minutes.
    Per side: every wall time, their median and best, the CLI's own account of the median run (fetch+decode, the sites line, the
    inflater's account), and — once — that the text of both sides is the same (md5; config 5: the first 0.5 Mbp, its text is gigabytes)."""
    import hashlib
    import re
    cli = os.path.join(ROOT, "bam_readcount_amd", "csrc", "bam-readcount")
    out = []
    for leg, small, cmd, sub in (
            ("tumor", ["--contig-mbp", str(a.e2e_tumor_mbp)], ["-w", "0", "-p", "-i", "-f", "g.fa", "g.bam", "chr2"], ["-w", "0", "-p", "-i", "-f", "g.fa", "g.bam", "chr2:1-500000"]),
            ("sites", ["--contigs", str(a.e2e_sites_contigs)], ["-w", "0", "-q", "20", "-b", "13", "-f", "g.fa", "-l", "sites", "g.bam"], None)):
        d = os.path.join(work, "e2e_" + leg)
        os.makedirs(d, exist_ok=True)
        entry = {"leg": leg, "config": 5 if leg == "tumor" else 4, "command": "bam-readcount " + " ".join(cmd) + " > /dev/null"}
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "e2e_configs.py"), "--leg", leg, "--reps", "1", "--check-lines", "200", "--check-mbp", "0.25", "--keep", d] + small,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        last = p.stdout.decode().strip().split("\n")[-1] if p.stdout else ""
        try:
            j = json.loads(last)
            entry["e2e_configs"] = {k: j.get(k) for k in ("what", "seconds", "events", "printed_lines", "bam_bytes", "validated", "stages")}
        except ValueError:
            entry["e2e_configs"] = {"error": (p.stderr.decode() or last)[-600:]}
        if not os.path.exists(os.path.join(d, "g.bam")):
            out.append(entry); continue
        sides = {"off": [], "on": []}
        env = dict(os.environ, BRC_CLI_TIMING="1"); env.pop("BRC_DEVICE_INFLATE", None)
        def one(side, args, sink):
            t0 = time.perf_counter()
            q = subprocess.run([cli] + (["--brc-device-inflate"] if side == "on" else []) + args, cwd=d, stdout=sink, stderr=subprocess.PIPE, env=env)
            t = time.perf_counter() - t0
            assert q.returncode == 0, q.stderr.decode()[-600:]
            return t, q
        with open(os.devnull, "wb") as dn:
            for side in ("off", "on"):
                one(side, cmd, dn)                                  # warm-up (page cache, the runtime's first start)
            t_all = time.perf_counter()
            # (at least --e2e-reps pairs and min-seconds of timed work per side; a side whose runs take minutes gets three)
            while len(sides["on"]) < (a.e2e_reps if time.perf_counter() - t_all < 60 else 3) or time.perf_counter() - t_all < 2 * a.min_seconds:
                for side in ("off", "on"):
                    t, q = one(side, cmd, dn)
                    err = q.stderr.decode(errors="replace")
                    rec = {"wall_s": round(t, 4), "stages": [l for l in err.splitlines() if l.startswith(("startup:", "timing:", "sites:", "device inflate:"))]}
                    m = re.search(r"timing: fetch\+decode ([0-9.]+) s", err)
                    rec["t_fetch_s"] = float(m.group(1)) if m else None
                    m = re.search(r"waiting for indexed fetch \+ decode ([0-9.]+) s \(the fetches themselves[^:]*: ([0-9.]+) s\)", err)
                    if m:
                        rec["t_site_fetch_wait_s"], rec["t_site_fetch_threads_s"] = float(m.group(1)), float(m.group(2))
                    sides[side].append(rec)
                    print("  %s %s %.3f s" % (leg, side, t), flush=True)
        for side, runs in sides.items():
            ws = sorted(r["wall_s"] for r in runs)
            med = sorted(runs, key=lambda r: r["wall_s"])[len(runs) // 2]
            entry[side] = {"runs": len(runs), "wall_s_all": [r["wall_s"] for r in runs], "wall_s_median": med["wall_s"], "wall_s_best": ws[0], "median_run": med}
        digests = {}
        for side in ("off", "on"):
            q = subprocess.run([cli] + (["--brc-device-inflate"] if side == "on" else []) + (sub or cmd), cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
            digests[side] = (q.returncode, hashlib.md5(q.stdout).hexdigest(), len(q.stdout))
        entry["same_text"] = {"what": "bam-readcount " + " ".join(sub or cmd), "bytes": digests["off"][2], "md5": digests["off"][1], "equal": digests["off"] == digests["on"]}
        assert digests["off"] == digests["on"] and digests["off"][0] == 0, digests
        print(json.dumps({k: entry[k] for k in ("leg", "off", "on", "same_text")})[:3000], flush=True)
        out.append(entry)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inflate_bench.json"))
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--sizes-mb", default="1,26,250")
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--lib", default=None, help="another library exporting include/brc_inflate.h (the CPU build of tests/sim_inflate: a dry run of this tool)")
    ap.add_argument("--e2e", action="store_true", help="also run tools/e2e_configs.py's legs and time their command lines with the switch off and on, interleaved")
    ap.add_argument("--e2e-reps", type=int, default=5)
    ap.add_argument("--e2e-tumor-mbp", type=float, default=6.25, help="config 5's region (BASELINE: 6.25 Mbp per GPU)")
    ap.add_argument("--e2e-sites-contigs", type=int, default=8, help="config 4's contigs of 12.5 Mbp")
    a = ap.parse_args()
    from bam_readcount_amd import capi
    import tempfile
    work = a.workdir or tempfile.mkdtemp(prefix="inflate_bench_")
    os.makedirs(work, exist_ok=True)
    host_exe = os.path.join(work, "inflate_host_bench")
    io = os.path.join(ROOT, "bam_readcount_amd", "csrc", "io")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tools", "inflate_host_bench.cpp"), os.path.join(io, "bamio.cpp"), "-o", host_exe, "-lz", "-ldl", "-pthread"])
    inf = capi.Inflater(a.lib)
    L = inf.lib
    members = make_piece(work, 26e6)
    res = {"box": socket.gethostname(), "device": "MI355X (gfx950)", "inflater": inf.kind(), "host_threads": a.threads,
           "host_path": "brcio::Bgzf (libdeflate when present, zlib otherwise), one handle per thread", "min_seconds": a.min_seconds,
           "kernel_object_sha256_16": capi.kernel_object_hash(capi.INFLATE_LIB), "pieces": []}
    for mb in [float(x) for x in a.sizes_mb.split(",")]:
        chain, n = chain_of(members, mb * 1e6)
        path = os.path.join(work, "chain_%g.bgzf" % mb)
        open(path, "wb").write(chain)
        src = np.frombuffer(chain, np.uint8)
        off = np.zeros(n + 1, np.uint64); st = np.zeros(n, np.uint8); cnt = C.c_size_t(n)
        L.brc_inflate_bgzf(inf.h, src.ctypes.data, len(chain), None, 0, off.ctypes.data, st.ctypes.data, C.byref(cnt))
        out_bytes = int(off[n])
        entry = {"compressed_bytes": len(chain), "members": n, "output_bytes": out_bytes}
        # pageable memory (what the command line hands over) and page-locked memory (brc_inflate_host_alloc)
        dst = np.empty(out_bytes, np.uint8)
        p_src = L.brc_inflate_host_alloc(len(chain)); p_dst = L.brc_inflate_host_alloc(out_bytes)
        C.memmove(p_src, src.ctypes.data, len(chain))

        def call(s, d):
            def f():
                c = C.c_size_t(n)
                rc = L.brc_inflate_bgzf(inf.h, s, len(chain), d, out_bytes, off.ctypes.data, st.ctypes.data, C.byref(c))
                assert rc == 0 and not st.any(), (rc, np.flatnonzero(st)[:8], st[st != 0][:8], L.brc_inflater_last_error(inf.h))
                return inf.last_timing()
            return f
        legs = [("gpu_pageable", call(src.ctypes.data, dst.ctypes.data)), ("host", None), ("gpu_pinned", call(p_src, p_dst))]
        for name, fn in legs:                                  # interleaved: device, host, device
            if fn is None:
                o = subprocess.run([host_exe, path, str(a.threads), str(a.min_seconds)], stdout=subprocess.PIPE, check=True).stdout.split()
                assert int(o[2]) == out_bytes, (o, out_bytes)
                entry["host"] = {"reps": int(o[3]), "seconds": float(o[4]), "GBps_out": out_bytes * int(o[3]) / float(o[4]) / 1e9}
                continue
            reps, s, acc = timed(fn, a.min_seconds)
            ks = sum(t["kernel_s"] for t in acc); cs = sum(t["call_s"] for t in acc)
            entry[name] = {"reps": reps, "seconds": s, "kernel_GBps_out": out_bytes * reps / ks / 1e9, "call_GBps_out": out_bytes * reps / cs / 1e9,
                           "kernel_ms": 1e3 * ks / reps, "call_ms": 1e3 * cs / reps}
        assert bytes(dst[:4096]) == C.string_at(p_dst, 4096)
        L.brc_inflate_host_free(p_src); L.brc_inflate_host_free(p_dst)
        res["pieces"].append(entry)
        print(json.dumps(entry), flush=True)
    if a.e2e:
        res["e2e"] = e2e_legs(a, work)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
