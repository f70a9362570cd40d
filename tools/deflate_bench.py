#!/usr/bin/env python3
"""Device-side BGZF compression (include/brc_deflate.h) measured: members alone, and the command line end to end.

    python tools/deflate_bench.py [--sizes 1,64,512] [--tumor-mbp 6.25] [--wgs-mbp 30] [--out profiles/deflate_bench.json]

The BAMs are tools/e2e_configs.py's: config 5 (tumor200x, -p -i, chr2 of a three-contig file) and config 3 (wgs30x, -q20 -b13, one
contig), written by the same generator calls.  One box, one invocation.

Members alone, on the text the product prints for config 5 (its first bytes, at 1, 64 and 512 MB): per size one warm-up, then calls
for at least a second per figure, the legs taking turns; GB/s are of INPUT bytes.  Legs: the device's kernels alone (events around
them), the whole call from pageable memory, the whole call from page-locked memory (brc_deflate_host_alloc), and the host on 16
threads over the same 0xff00 pieces (tools/deflate_host.cpp: zlib level 1, libdeflate level 1 when the box has one).  Sizes: the
device's, zlib level 1, zlib level 6.

End to end, per config, three runs per leg, the legs interleaved (a, b, c, d, a, b, ...), wall seconds as median and best:
  off_null   switch off > /dev/null              on_null    switch on > /dev/null
  off_pipe   switch off | deflate_host pipe 16 > /dev/null      on_file    switch on > a file
and once per leg, untimed, the md5 of the leg's text after decompression (gzip -dc), which must be the same four times."""
import argparse
import ctypes as C
import hashlib
import json
import os
import re
import socket
import subprocess
import sys
import time
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
CLI = os.path.join(ROOT, "bam_readcount_amd", "csrc", "bam-readcount")
M = 0xff00


def make_bams(work, tumor_mbp, wgs_mbp):
    """{config: (directory, command-line arguments)}: tools/e2e_configs.py leg_tumor's file; a one-contig wgs30x file"""
    import synthgen
    out = {}
    d = os.path.join(work, "config5"); os.makedirs(d, exist_ok=True)
    cfg = synthgen.CONFIGS["tumor200x"]
    contigs = [("chr1", 200_000), ("chr2", int(tumor_mbp * 1e6)), ("chr3", 200_000)]
    w = synthgen.BamWriter(os.path.join(d, "g.bam"), contigs, n_libs=cfg["n_libs"], rgs_per_lib=2); refs = []
    for t, (nm, ln) in enumerate(contigs):
        ref, a = synthgen.generate(ln, "tumor200x", seed=200 + 17 * t); w.add(t, a); refs.append((nm, ref)); del a
    w.close(); synthgen.write_fasta(os.path.join(d, "g.fa"), refs)
    out["config 5"] = (d, ["-w", "0", "-p", "-i", "-f", "g.fa", "g.bam", "chr2"], "tumor200x, chr2 = %.2f Mbp, -p -i" % tumor_mbp)
    d = os.path.join(work, "config3"); os.makedirs(d, exist_ok=True)
    contigs = [("chr1", int(wgs_mbp * 1e6))]
    w = synthgen.BamWriter(os.path.join(d, "g.bam"), contigs, n_libs=1, rgs_per_lib=1)
    ref, a = synthgen.generate(contigs[0][1], "wgs30x", seed=7); w.add(0, a); del a
    w.close(); synthgen.write_fasta(os.path.join(d, "g.fa"), [("chr1", ref)])
    out["config 3"] = (d, ["-w", "0", "-q", "20", "-b", "13", "-f", "g.fa", "g.bam", "chr1"], "wgs30x, chr1 = %.1f Mbp, -q20 -b13" % wgs_mbp)
    return out


def sh(cmd, cwd, env):
    p = subprocess.run(["bash", "-c", "set -o pipefail; " + cmd], cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, (cmd, p.stderr.decode()[-600:])
    return p


def e2e(name, d, args, what, host_exe, runs):
    env = dict(os.environ, BRC_CLI_TIMING="1"); env.pop("BRC_BGZF_OUTPUT", None)
    off = " ".join([CLI] + args); on = " ".join([CLI, "--brc-bgzf-output"] + args)
    legs = {"off_null": off + " > /dev/null", "on_null": on + " > /dev/null", "off_pipe": off + " | %s pipe 16 > /dev/null" % host_exe, "on_file": on + " > out.bgzf"}
    for c in legs.values():
        sh(c, d, env)                                                # warm-up (page cache, the runtime's first start)
    t = {k: [] for k in legs}; acct = None
    for _ in range(runs):
        for k, c in legs.items():
            t0 = time.perf_counter(); p = sh(c, d, env); t[k].append(round(time.perf_counter() - t0, 3))
            if k == "on_null":
                m = re.search(r"device deflate: .*", p.stderr.decode()); acct = m.group(0) if m else None
            print("  %s %s %.3f s" % (name, k, t[k][-1]), flush=True)
    res = {"what": what, "command": "bam-readcount " + " ".join(args), "legs": {}}
    res["bgzf_bytes"] = os.path.getsize(os.path.join(d, "out.bgzf"))
    md5 = {"off_null": off + " | md5sum", "on_null": on + " | gzip -dc | md5sum", "off_pipe": off + " | %s pipe 16 | gzip -dc | md5sum" % host_exe, "on_file": "gzip -dc < out.bgzf | md5sum"}
    for k in legs:
        s = sorted(t[k])
        res["legs"][k] = {"command": legs[k].replace(CLI, "bam-readcount").replace(host_exe, "deflate_host"), "wall_s": t[k], "median_s": s[len(s) // 2], "best_s": s[0],
                          "md5_of_decompressed_text": sh(md5[k], d, env).stdout.split()[0].decode()}
    assert len({v["md5_of_decompressed_text"] for v in res["legs"].values()}) == 1, res
    res["text_bytes"] = int(sh("gzip -dc < out.bgzf | wc -c", d, env).stdout.split()[0])
    res["device_deflate_account_of_last_on_null_run"] = acct
    os.remove(os.path.join(d, "out.bgzf"))
    return res


def members_alone(text_path, sizes, host_exe, seconds, res):
    from bam_readcount_amd import capi
    d = capi.Deflater()
    res["kernel_object_sha256_16"] = capi.kernel_object_hash(capi.DEFLATE_LIB)
    res["engine_kernel_object_sha256_16"] = capi.kernel_object_hash()
    have = os.path.getsize(text_path)
    for mb in sizes:
        n = min(mb << 20, have)
        src = np.fromfile(text_path, np.uint8, n)
        piece = text_path + ".%d" % mb; src.tofile(piece)
        cap = d.bound(n); dstp = np.empty(cap, np.uint8)
        hp = d.lib.brc_deflate_host_alloc(n); hd = d.lib.brc_deflate_host_alloc(cap)
        assert hp and hd
        C.memmove(hp, src.ctypes.data, n)
        got = C.c_size_t(); nm = C.c_size_t()

        def call(s, t):
            assert d.lib.brc_deflate_bgzf(d.h, s, n, t, cap, C.byref(got), C.byref(nm)) == 0
            return d.last_timing()

        def host(level, secs):
            p = subprocess.run([host_exe, "bench", piece, "16", str(secs), str(level)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            if p.returncode == 3:
                return None
            assert p.returncode == 0, p.stderr.decode()
            reps, s, total = p.stdout.split()
            return int(reps), float(s), int(total)
        call(hp, hd); call(src.ctypes.data, dstp.ctypes.data)                                       # warm-up
        acc = {"device_kernels": [0, 0.0], "call_pinned": [0, 0.0], "call_pageable": [0, 0.0], "zlib1_16_threads": [0, 0.0], "libdeflate1_16_threads": [0, 0.0]}
        z1 = ld1 = None; rounds = 0
        while min(acc[k][1] for k in ("device_kernels", "call_pinned", "call_pageable", "zlib1_16_threads")) < seconds:       # the legs take turns
            t = call(hp, hd); acc["call_pinned"][0] += 1; acc["call_pinned"][1] += t["call_s"]; acc["device_kernels"][0] += 1; acc["device_kernels"][1] += t["kernel_s"]
            t = call(src.ctypes.data, dstp.ctypes.data); acc["call_pageable"][0] += 1; acc["call_pageable"][1] += t["call_s"]
            if rounds % 8 == 0:                 # (a process start each: a slice of a quarter of the wanted time, every eighth round)
                r = host(1, seconds / 4); acc["zlib1_16_threads"][0] += r[0]; acc["zlib1_16_threads"][1] += r[1]; z1 = r[2]
                r = host(101, seconds / 4)
                if r:
                    acc["libdeflate1_16_threads"][0] += r[0]; acc["libdeflate1_16_threads"][1] += r[1]; ld1 = r[2]
            rounds += 1
        out_bytes = got.value
        assert C.string_at(hd, out_bytes) == dstp[:out_bytes].tobytes()
        if mb <= 64:                            # what came back is the text
            p = subprocess.run(["gzip", "-dc"], input=C.string_at(hd, out_bytes), stdout=subprocess.PIPE, check=True)
            assert p.stdout == src.tobytes()
        z6 = host(6, 0.01)
        r = {"input_bytes": n, "members": nm.value, "device_bytes": out_bytes, "zlib1_bytes": z1, "zlib6_bytes": z6[2], "libdeflate1_bytes": ld1,
             "ratio_device_to_zlib1": round(out_bytes / z1, 4)}
        for k, (reps, s) in acc.items():
            r[k] = {"reps": reps, "timed_s": round(s, 3), "gbps_of_input": round(n * reps / s / 1e9, 3)} if reps else None
        res["members_alone"]["%d MB" % mb] = r
        print(json.dumps({"%d MB" % mb: r}), flush=True)
        d.lib.brc_deflate_host_free(hp); d.lib.brc_deflate_host_free(hd); os.remove(piece)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,64,512")
    ap.add_argument("--tumor-mbp", type=float, default=6.25)
    ap.add_argument("--wgs-mbp", type=float, default=30.0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deflate_bench.json"))
    a = ap.parse_args()
    work = a.workdir or tempfile.mkdtemp(prefix="deflate_bench_")
    os.makedirs(work, exist_ok=True)
    host_exe = os.path.join(work, "deflate_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tools", "deflate_host.cpp"), "-o", host_exe, "-lz", "-ldl", "-pthread"])
    t0 = time.time(); bams = make_bams(work, a.tumor_mbp, a.wgs_mbp); print("BAMs written in %.0f s" % (time.time() - t0), flush=True)
    res = {"tool": "tools/deflate_bench.py", "box": socket.gethostname(), "device": "MI355X (gfx950)", "host_threads": 16, "members_alone": {}, "end_to_end": {}}
    # the members' text: the first bytes of what config 5 prints
    sizes = [int(x) for x in a.sizes.split(",")]
    d5, args5, _ = bams["config 5"]
    text_path = os.path.join(work, "text5")
    bp = int(max(sizes) * (1 << 20) / 1400 * 1.3) + 20000              # (about 1.4 kB per position with four libraries)
    sh(" ".join([CLI] + args5[:-1] + ["chr2:1-%d" % bp]) + " > " + text_path, d5, dict(os.environ))
    res["members_alone_text"] = "bam-readcount " + " ".join(args5[:-1]) + " chr2:1-%d (config 5), its first bytes" % bp
    members_alone(text_path, sizes, host_exe, a.seconds, res)
    os.remove(text_path)
    for name, (d, args, what) in bams.items():
        res["end_to_end"][name] = e2e(name, d, args, what, host_exe, a.runs)
        print(json.dumps({name: res["end_to_end"][name]}), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1); f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
