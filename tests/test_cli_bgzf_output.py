"""--brc-bgzf-output of the drop-in command line: stdout as BGZF members compressed by the deflater library (include/brc_deflate.h).
[sim]: the simulator's command line with BRC_DEFLATE_LIB pointing at the CPU build of the deflater; [hip] (gpu-marked): the product
binary, which finds libbrc_deflate_hip.so next to itself.  With the switch on, the decompressed stdout, stderr and the exit code are
those of the switch off, and the stream ends with exactly one end-of-file member."""
import os
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_cli import HIP_CLI, RUNS, SIM_CLI, _sites_file, _write_fasta

sys.path.insert(0, os.path.join(ROOT, "tools", "fuzz"))
import inflate_members as im  # noqa: E402

SIM_DEFLATE = os.path.join(ROOT, "tests", "sim_deflate", "libbrc_deflate_sim.so")
SIM_INFLATE = os.path.join(ROOT, "tests", "sim_inflate", "libbrc_inflate_sim.so")
EOF_BLOCK = im.EOF_MEMBER


@pytest.fixture(scope="module", params=["sim", pytest.param("hip", marks=pytest.mark.gpu)])
def cli(request):
    """(executable, environment additions)"""
    if request.param == "hip":
        assert os.path.exists(HIP_CLI), "the product binary is not built"
        return HIP_CLI, {}
    for d in ("sim", "sim_deflate", "sim_inflate"):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", d)])
    return SIM_CLI, {"BRC_DEFLATE_LIB": SIM_DEFLATE, "BRC_INFLATE_LIB": SIM_INFLATE}


def _run(cli, args, cwd, env=None, on=False):
    exe, add = cli
    e = dict(os.environ); e.pop("BRC_BGZF_OUTPUT", None); e.pop("BRC_DEVICE_INFLATE", None); e.update(add); e.update(env or {})
    p = subprocess.run([exe] + (["--brc-bgzf-output"] if on else []) + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)
    return p.returncode, p.stdout, p.stderr


def gunzip(raw):
    """The text of a BGZF stream, member by member; the stream must end with the end-of-file member, which occurs exactly once."""
    members, _ = im.split_members(raw, decode=False)
    assert sum(len(m) for m in members) == len(raw)
    assert members and members[-1] == EOF_BLOCK, "no end-of-file member at the end"
    assert sum(1 for m in members if m == EOF_BLOCK) == 1
    assert all(zlib.decompress(m, 31) for m in members[:-1]), "an empty member inside the stream"
    return b"".join(zlib.decompress(m, 31) for m in members)


def _same(cli, args, cwd, env=None, rc=0, env_on=None):
    off = _run(cli, args, cwd, env, on=False)
    e = dict(env or {}); e.update(env_on or {})
    on = _run(cli, args, cwd, e, on=True)
    assert off[0] == rc, (args, off[0], off[2][-300:])
    assert on[0] == off[0] and on[2] == off[2], (args, on[0], on[2][-300:], off[2][-300:])
    assert gunzip(on[1]) == off[1], args
    return off, on


def test_reference_integration_runs_with_bgzf_output(cli, workdir):
    for exp, bam, extra, how in RUNS:
        args = ["-w", "1"] + extra + ["-f", "ref.fa"] + (["-l", "site_list", bam] if how == "list" else [bam, "21:10402985-10402985", "21:10405200-10405200"])
        (rc, out, err), on = _same(cli, args, workdir)
        assert out == open(os.path.join(GOLDEN, exp), "rb").read(), (exp, bam, extra, how)
        assert gunzip(on[1]) == out and on[1].endswith(EOF_BLOCK)
    # the environment variable is the same switch; the text went THROUGH the deflater: its account is not empty
    args = ["-w", "1", "-f", "ref.fa", "-l", "site_list", "test.bam"]
    rc, out, err = _run(cli, args, workdir, env={"BRC_BGZF_OUTPUT": "1", "BRC_CLI_TIMING": "1"})
    assert rc == 0 and gunzip(out) == open(os.path.join(GOLDEN, "expected_all_lib"), "rb").read()
    assert out == _run(cli, args, workdir, on=True)[1]
    m = re.search(rb"device deflate: (\d+) calls, ([0-9.]+) MB in, ([0-9.]+) MB out, ([0-9.]+) s", err)
    assert m and int(m.group(1)) > 0, err[-400:]


@pytest.fixture(scope="module")
def long_bam(tmp_path_factory):
    """40 kb and 9 kb of reads in 4000-byte blocks, with a BAI; a copy cut at two thirds (the fixture of tests/test_cli_inflate.py, rebuilt)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bamio
    import synth
    d = tmp_path_factory.mktemp("bgzf_cli")
    rng = np.random.default_rng(5)
    refs = [synth.make_ref(rng, 40000), synth.make_ref(rng, 9000)]
    parts = [synth.make_batch(71, refs[0], 2500, style="indel"), synth.make_batch(72, refs[1], 700, style="mixed")]
    arrs = {}
    for k in ("pos", "flag", "mapq", "lib", "l_qseq", "n_cigar", "nm", "sm", "tags"):
        arrs[k] = np.concatenate([p[k] for p in parts])
    for arena, off in (("cigar", "cigar_off"), ("seq4", "seq_off"), ("qual", "qual_off")):
        arrs[arena] = np.concatenate([p[arena] for p in parts])
        arrs[off] = np.concatenate([parts[0][off], parts[1][off] + np.uint64(parts[0][arena].size)])
    tids = np.concatenate([np.zeros(len(parts[0]["pos"]), int), np.ones(len(parts[1]["pos"]), int)])
    bamio.write_bam(str(d / "x.bam"), [("chrA", 40000), ("chrB", 9000)], arrs, tids, block_bytes=4000)
    _write_fasta(d / "r.fa", [("chrA", refs[0]), ("chrB", refs[1])])
    raw = open(d / "x.bam", "rb").read()
    open(d / "cut.bam", "wb").write(raw[:len(raw) * 2 // 3])
    os.link(d / "x.bam.bai", d / "cut.bam.bai")
    rng2 = np.random.default_rng(9)
    sites = [("chrA", int(p), int(p) + 3) for p in sorted(rng2.integers(1, 39000, 60))] + [("chrB", 17, 17), ("chrB", 8000, 9000)]
    _sites_file(d, "s.txt", sites)
    return d


def test_switch_on_decompresses_to_switch_off(cli, long_bam):
    d = long_bam
    base = ["-w", "0", "-f", "r.fa"]
    small = {"BRC_BGZF_BATCH": "300000"}           # several deflate calls per run
    (rc, out, err), on = _same(cli, base + ["--brc-chunk", "500", "x.bam", "chrA:2000-30000"], d, env_on=small)
    assert out.count(b"\n") > 20000 and len(on[1]) < len(out) // 3
    _same(cli, base + ["x.bam", "chrA", "chrB"], d)
    _same(cli, base + ["-l", "s.txt", "x.bam"], d)
    _same(cli, base + ["-l", "s.txt", "--brc-plan", "0", "x.bam"], d)
    _same(cli, base + ["-p", "x.bam", "chrA:1-9000"], d)
    for ranks in ("2", "3"):
        _same(cli, base + ["--brc-ranks", ranks, "x.bam", "chrA"], d, env={"BRC_RANK_CUT": "4096"}, env_on=small)
    # a BAM cut at two thirds: exit code 1, the text written before the cut is all there, and the end-of-file member too
    (rc, out, err), on = _same(cli, base + ["--brc-chunk", "2000", "cut.bam", "chrA"], d, rc=1)
    assert b"read error" in err and out.count(b"\n") > 1000
    _same(cli, base + ["cut.bam", "chrA"], d, rc=1)
    # the same as ranks: the rank that meets the cut has written members; one end-of-file member behind what was written
    off = _run(cli, base + ["--brc-ranks", "2", "--brc-chunk", "2000", "cut.bam", "chrA"], d, env={"BRC_RANK_CUT": "4096"})
    on = _run(cli, base + ["--brc-ranks", "2", "--brc-chunk", "2000", "cut.bam", "chrA"], d, env={"BRC_RANK_CUT": "4096"}, on=True)
    assert off[0] == on[0] == 1 and gunzip(on[1]) == off[1] and off[1].count(b"\n") > 1000


def test_several_engines_on_the_simulator(long_bam):
    for d in ("sim", "sim_deflate"):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", d)])
    cli = (SIM_CLI, {"BRC_DEFLATE_LIB": SIM_DEFLATE})
    _same(cli, ["-w", "0", "-f", "r.fa", "--brc-gpus", "2", "--brc-chunk", "3000", "x.bam", "chrA"], long_bam)
    _same(cli, ["-w", "0", "-f", "r.fa", "--brc-gpus", "2", "-l", "s.txt", "x.bam"], long_bam)


def test_timing_line_and_missing_library(cli, long_bam):
    args = ["-w", "0", "-f", "r.fa", "x.bam", "chrA:1-20000"]
    rc, out, err = _run(cli, args, long_bam, env={"BRC_CLI_TIMING": "1"}, on=True)
    m = re.search(rb"device deflate: (\d+) calls, ([0-9.]+) MB in, ([0-9.]+) MB out, ([0-9.]+) s", err)
    assert rc == 0 and m and int(m.group(1)) > 0 and float(m.group(3)) < float(m.group(2)), err[-400:]
    rc, out, err = _run(cli, args, long_bam, env={"BRC_DEFLATE_LIB": "/nonexistent/libbrc_deflate.so"}, on=True)
    assert rc == 1 and out == b"" and b"cannot load the deflater library" in err
    # ... and as ranks: no rank has a deflater, the coordinator adds nothing
    rc, out, err = _run(cli, ["-w", "0", "-f", "r.fa", "--brc-ranks", "2", "x.bam", "chrA"], long_bam, env={"BRC_DEFLATE_LIB": "/nonexistent/libbrc_deflate.so", "BRC_RANK_CUT": "4096"}, on=True)
    assert rc == 1 and out == b"" and b"cannot load the deflater library" in err


def test_combined_with_device_inflate(cli, long_bam):
    args = ["-w", "0", "-f", "r.fa", "--brc-chunk", "7000", "x.bam", "chrA"]
    off = _run(cli, args, long_bam)
    on = _run(cli, ["--brc-device-inflate"] + args, long_bam, on=True)
    assert off[0] == 0 and on[0] == 0 and gunzip(on[1]) == off[1] and on[2] == off[2]
