"""--brc-device-inflate of the drop-in command line: BGZF blocks inflated by the inflater library (include/brc_inflate.h) instead of
block by block on the fetch threads.  [sim]: the simulator's command line with BRC_INFLATE_LIB pointing at the CPU build of the
inflater; [hip] (gpu-marked): the product binary, which finds libbrc_inflate_hip.so next to itself.  With the switch on, stdout,
stderr and the exit code are those of the switch off — error cases included."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_cli import HIP_CLI, RUNS, SIM_CLI, _sites_file, _write_fasta, run_cli, synthetic_bam  # noqa: F401  (the reference's six runs and the synthetic BAM of the CLI tests)

SIM_INFLATE = os.path.join(ROOT, "tests", "sim_inflate", "libbrc_inflate_sim.so")


@pytest.fixture(scope="module", params=["sim", pytest.param("hip", marks=pytest.mark.gpu)])
def cli(request):
    """(executable, environment additions)"""
    if request.param == "hip":
        assert os.path.exists(HIP_CLI), "the product binary is not built"
        return HIP_CLI, {}
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "sim")])
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "sim_inflate")])
    return SIM_CLI, {"BRC_INFLATE_LIB": SIM_INFLATE}


def _run(cli, args, cwd, env=None, on=False):
    exe, add = cli
    e = dict(os.environ); e.pop("BRC_DEVICE_INFLATE", None); e.update(add); e.update(env or {})
    p = subprocess.run([exe] + (["--brc-device-inflate"] if on else []) + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)
    return p.returncode, p.stdout, p.stderr


def _same(cli, args, cwd, env=None, rc=0):
    off = _run(cli, args, cwd, env, on=False)
    on = _run(cli, args, cwd, env, on=True)
    assert off[0] == rc, (args, off[0], off[2][-300:])
    assert on == off, (args, on[0], on[2][-300:], off[2][-300:])
    return off


def test_reference_integration_runs_with_device_inflate(cli, workdir):
    exe, add = cli
    for exp, bam, extra, how in RUNS:
        args = ["-w", "1"] + extra + ["-f", "ref.fa"] + (["-l", "site_list", bam] if how == "list" else [bam, "21:10402985-10402985", "21:10405200-10405200"])
        rc, out, err = _run(cli, args, workdir, on=True)
        assert rc == 0, err.decode()
        assert out == open(os.path.join(GOLDEN, exp), "rb").read(), (exp, bam, extra, how)
        assert b"Minimum mapping quality is set to 0" in err
    # the environment variable is the same switch
    rc, out, err = _run(cli, ["-w", "1", "-f", "ref.fa", "-l", "site_list", "test.bam"], workdir, env={"BRC_DEVICE_INFLATE": "1", "BRC_CLI_TIMING": "1"})
    assert rc == 0 and out == open(os.path.join(GOLDEN, "expected_all_lib"), "rb").read()
    # the blocks went THROUGH the inflater: calls, bytes in and bytes out of its account are not zero (a quiet return to the host path would leave them so)
    m = re.search(rb"device inflate: (\d+) calls, ([0-9.]+) MB in, ([0-9.]+) MB out", err)
    assert m and int(m.group(1)) > 0 and float(m.group(2)) > 0 and float(m.group(3)) > float(m.group(2)), err[-400:]


@pytest.fixture(scope="module")
def long_bam(tmp_path_factory):
    """40 kb and 9 kb of reads in 4000-byte blocks, with a BAI; a CSI-indexed copy; a copy cut at two thirds; a copy with one CRC byte flipped."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bamio
    import synth
    d = tmp_path_factory.mktemp("inflate_cli")
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
    (d / "csi").mkdir()
    bamio.write_bam(str(d / "csi" / "x.bam"), [("chrA", 40000), ("chrB", 9000)], arrs, tids, block_bytes=4000, csi=(14, 5))
    assert os.path.exists(d / "csi" / "x.bam.csi") and not os.path.exists(d / "csi" / "x.bam.bai")
    _write_fasta(d / "r.fa", [("chrA", refs[0]), ("chrB", refs[1])])
    shutil.copy(d / "r.fa", d / "csi" / "r.fa")
    raw = open(d / "x.bam", "rb").read()
    open(d / "cut.bam", "wb").write(raw[:len(raw) * 2 // 3])
    os.link(d / "x.bam.bai", d / "cut.bam.bai")
    # the CRC32 of a block in the middle of the file: the trailer of the member that holds the file's middle byte
    sys.path.insert(0, os.path.join(ROOT, "tools", "fuzz"))
    import inflate_members as im
    members, _ = im.split_members(raw, decode=False)
    o = 0
    for m in members:
        if o + len(m) > len(raw) // 2:
            break
        o += len(m)
    bad = bytearray(raw); bad[o + len(m) - 7] ^= 0x20
    open(d / "crc.bam", "wb").write(bytes(bad))
    os.link(d / "x.bam.bai", d / "crc.bam.bai")
    rng2 = np.random.default_rng(9)
    sites = [("chrA", int(p), int(p) + 3) for p in sorted(rng2.integers(1, 39000, 60))] + [("chrB", 17, 17), ("chrB", 8000, 9000)]
    _sites_file(d, "s.txt", sites)
    return d


def test_switch_on_equals_switch_off(cli, long_bam):
    d = long_bam
    base = ["-w", "0", "-f", "r.fa"]
    a = _same(cli, base + ["--brc-chunk", "500", "x.bam", "chrA:2000-30000"], d)
    assert a[1].count(b"\n") > 20000
    _same(cli, base + ["x.bam", "chrA", "chrB"], d)
    # a striped fetch: five stripes share the piece's window
    _same(cli, base + ["--brc-chunk", "7000", "x.bam", "chrA"], d, env={"BRC_FETCH_STRIPE_MIN": "100", "BRC_FETCH_THREADS": "5"})
    _same(cli, base + ["--brc-chunk", "3000", "x.bam", "chrA"], d, env={"BRC_FETCH_STRIPE_MIN": "100", "BRC_FETCH_THREADS": "3"})
    _same(cli, base + ["x.bam", "chrA", "chrB:100-8000"], d / "csi")
    _same(cli, base + ["-l", "s.txt", "x.bam"], d)
    _same(cli, base + ["-l", "s.txt", "--brc-plan", "0", "x.bam"], d)
    _same(cli, base + ["--brc-ranks", "2", "x.bam", "chrA"], d, env={"BRC_RANK_CUT": "4096"})
    # a BAM cut at two thirds: exit code 1 and "read error", nothing partial of the piece that met the cut
    c = _same(cli, base + ["cut.bam", "chrA"], d, rc=1)
    assert b"read error" in c[2]
    c = _same(cli, base + ["--brc-chunk", "2000", "cut.bam", "chrA"], d, rc=1)
    assert b"read error" in c[2] and c[1].count(b"\n") > 1000
    # one flipped CRC byte: the same message as the host path
    c = _same(cli, base + ["crc.bam", "chrA"], d, rc=1)
    assert b"read error" in c[2]
    c = _same(cli, base + ["--brc-chunk", "2000", "crc.bam", "chrA"], d, rc=1, env={"BRC_FETCH_STRIPE_MIN": "100", "BRC_FETCH_THREADS": "4"})
    assert b"read error" in c[2]
    # ... and a region in front of the damaged block does not notice it, on either path
    _same(cli, base + ["crc.bam", "chrA:1-3000"], d)


def test_missing_library_is_an_error_and_cram_ignores_the_switch(cli, long_bam, synthetic_bam):  # noqa: F811
    rc, out, err = _run(cli, ["-w", "0", "-f", "r.fa", "x.bam", "chrA:1-2000"], long_bam, env={"BRC_INFLATE_LIB": "/nonexistent/libbrc_inflate.so"}, on=True)
    assert rc == 1 and out == b"" and b"cannot load the inflater library" in err
    off = _run(cli, ["-w", "0", "-f", "syn.fa", "syn.cram", "chrA:100-2000"], synthetic_bam, on=False)
    on = _run(cli, ["-w", "0", "-f", "syn.fa", "syn.cram", "chrA:100-2000"], synthetic_bam, env={"BRC_INFLATE_LIB": "/nonexistent/libbrc_inflate.so"}, on=True)
    assert off[0] == 0 and on[0] == 0 and on[1] == off[1] and off[1].count(b"\n") > 1000
    assert on[2].count(b"--brc-device-inflate is ignored for CRAM input") == 1
    assert on[2].replace(b"bam-readcount: --brc-device-inflate is ignored for CRAM input\n", b"") == off[2]
