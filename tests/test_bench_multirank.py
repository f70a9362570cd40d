"""bench.py's rank arithmetic without GPUs: two ranks under torch.distributed.run with the gloo backend, the C-ABI served by
the CPU lane simulator (`--dry-run-lib`, test infrastructure: the line it prints says "dry_run" and carries no throughput).
In every mode the totals rank 0 reduces must equal the sum of what each rank owns when its share is run on its own
(`--as-rank r --as-world 2`, no launcher), and the partition must be the documented one: weak — every rank its own contig;
strong — the contig cut into world_size intervals; sites — the -l list cut into contiguous slices whose sizes add up.
What is left for the real multi-GPU run is RCCL itself."""
import json
import os
import socket
import subprocess
import sys

import pytest

from conftest import ROOT

SIM = os.path.join(ROOT, "tests", "sim", "libbrc_sim.so")
COMMON = ["--steps", "1", "--warmup", "0", "--cpu-sample-mbp", "0", "--e2e-mbp", "0", "--other-configs", "0", "--dry-run-lib", SIM]
MODES = {"weak": ["--mode", "weak", "--contig-mbp", "0.06"],
         "strong": ["--mode", "strong", "--contig-mbp", "0.02"],
         "sites": ["--mode", "sites", "--contig-mbp", "0.06", "--sites", "301"]}


def line_of(out):
    return json.loads([l for l in out.decode().splitlines() if l.startswith("{")][-1])


@pytest.mark.parametrize("mode,world", [("strong", 4), ("sites", 8)])
def test_more_ranks_describe_themselves(mode, world):
    """world 4 and 8 (the driver's scaling run goes to 8): the line carries every rank's own clock, share and memory, the
    shares add up to the totals, and the partition is the documented one."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "sim")])
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, OMP_NUM_THREADS="1")
    small = {"strong": ["--mode", "strong", "--contig-mbp", "0.016"], "sites": ["--mode", "sites", "--contig-mbp", "0.03", "--sites", "203"]}[mode]
    run = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1", "--master-port", str(port),
                          os.path.join(ROOT, "bench.py"), "--gpus", str(world)] + small + COMMON, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=900)
    assert run.returncode == 0, run.stderr.decode()[-2000:]
    total = line_of(run.stdout)
    pr = total["per_rank"]
    assert total["n_gpus"] == world and [x["rank"] for x in pr] == list(range(world))
    assert sum(x["events"] for x in pr) == total["events_per_step"] > 0 and sum(x["positions"] for x in pr) == total["positions_per_step"]
    if mode == "sites":
        assert total["positions_per_step"] == 203 and sorted(x["positions"] for x in pr) == sorted([203 // world + (1 if r < 203 % world else 0) for r in range(world)])
    else:
        for x in pr:
            assert 3_500 < x["positions"] <= 4_000           # 16 kb cut into 4 intervals


@pytest.mark.parametrize("mode", sorted(MODES))
def test_two_ranks_reduce_what_each_rank_owns(mode):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "sim")])
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, OMP_NUM_THREADS="1")
    two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
                          os.path.join(ROOT, "bench.py"), "--gpus", "2"] + MODES[mode] + COMMON, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=900)
    assert two.returncode == 0, two.stderr.decode()[-2000:]
    total = line_of(two.stdout)
    assert total["dry_run"].startswith("rank arithmetic only") and total["value"] is None and total["n_gpus"] == 2
    own = []
    for r in (0, 1):
        one = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--as-rank", str(r), "--as-world", "2"] + MODES[mode] + COMMON,
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=900)
        assert one.returncode == 0, one.stderr.decode()[-2000:]
        own.append(line_of(one.stdout))
    assert total["events_per_step"] == own[0]["own_events"] + own[1]["own_events"] > 0
    assert total["positions_per_step"] == own[0]["own_positions"] + own[1]["own_positions"] > 0
    assert total["own_events"] == own[0]["own_events"]                       # rank 0 of the pair did rank 0's share
    if mode == "sites":
        assert total["positions_per_step"] == 301 and {own[0]["own_positions"], own[1]["own_positions"]} == {150, 151}
    if mode == "strong":
        # fixed total work: each rank an interval of half the contig (0.02 Mbp -> 10 kb each), about 200x deep
        for o in own:
            assert 9_000 < o["own_positions"] <= 10_000 and 150 * 9_000 < o["own_events"] < 250 * 10_000
    if mode == "weak":
        for o in own:
            assert 59_000 < o["own_positions"] <= 60_000
        assert own[0]["own_events"] != own[1]["own_events"]                  # different contigs (seed per rank)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_every_rank_validates_its_own_share_with_full_only(mode):
    """A plain run checks nothing; with --full every rank holds a prefix of its own interval (its own sites) against the oracle
    and the verdicts are MIN-reduced onto the line."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "sim")])
    env = dict(os.environ, OMP_NUM_THREADS="1")
    lines = {}
    for full in ([], ["--full"]):
        s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
        run = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
                              os.path.join(ROOT, "bench.py"), "--gpus", "2"] + full + MODES[mode] + COMMON, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=900)
        assert run.returncode == 0, run.stderr.decode()[-2000:]
        lines[bool(full)] = line_of(run.stdout)
    assert lines[False]["validated"] is None and all("validated_ok" not in x for x in lines[False]["per_rank"])
    v = lines[True]["validated"]
    assert v["all_ranks_ok"] is True and v["own_error"] is None and v["own"]
    assert all(x["validated_ok"] is True and x["validated_events"] > 0 for x in lines[True]["per_rank"])
    for k in ("events_per_step", "positions_per_step", "own_events", "own_positions"):
        assert lines[False][k] == lines[True][k] > 0


@pytest.mark.parametrize("mode", ["weak", "strong"])
def test_dump_outputs_are_reproducible_and_equal_the_oracle(mode, tmp_path, oracle_lib):
    """--dump-outputs: float32 / float64 arrays, at most 64 MB, the same on every run with the same inputs whatever --steps is,
    and the sampled windows' planes and indel buckets are what the oracle computes for those windows as regions of their own."""
    import numpy as np
    import bench
    import parity
    import synthgen
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "sim")])
    env = dict(os.environ, OMP_NUM_THREADS="1")
    dirs, lines = [], []
    assert COMMON[:2] == ["--steps", "1"]
    for steps in ("1", "3"):
        d = tmp_path / ("steps" + steps)
        run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + MODES[mode] + ["--steps", steps] + COMMON[2:] + ["--dump-outputs", str(d)],
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=900)
        assert run.returncode == 0, run.stderr.decode()[-2000:]
        dirs.append(d); lines.append(line_of(run.stdout))
    names = sorted(os.listdir(dirs[0]))
    assert names == sorted(os.listdir(dirs[1])) and "ncol.npy" in names and "istat.npy" in names
    got = {n[:-4]: np.load(dirs[0] / n) for n in names}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= 64 << 20
    for n in names:
        np.testing.assert_array_equal(got[n[:-4]], np.load(dirs[1] / n), err_msg=n)
    assert list(got["region_counts"]) == [lines[0]["own_events"], lines[0]["own_positions"]]
    assert got["ncol"].sum() == got["window_events"].sum() > 0
    # the first windows of the sample against the oracle, each as a region of its own
    per_lib = mode == "strong"
    contig_len = int(float(MODES[mode][-1]) * 1e6)
    ref, arrs = synthgen.generate(contig_len, "tumor200x" if per_lib else "wgs30x", seed=1)
    names_l = ["lib%d" % i for i in range(synthgen.CONFIGS["tumor200x"]["n_libs"])] if per_lib else ()
    opts = dict(min_mapq=0, min_bq=0, per_lib=True, insertion_centric=True) if per_lib else dict(min_mapq=20, min_bq=13)
    W = bench.DUMP_WINDOW_LEN
    n_ind = 0
    for j, a in enumerate(got["window_start"][:4].astype(int).tolist()):
        _, (r,) = parity.run_engine(oracle_lib, arrs, [(a, a + W)], ref=ref, lib_names=names_l, **opts)
        off = a - r.pos0
        blk = slice(j * W, (j + 1) * W)
        for k in ("ncol", "depth", "istat"):
            np.testing.assert_array_equal(got[k][..., blk], getattr(r, k)[..., off:off + W].astype(np.float64), err_msg=k)
        np.testing.assert_array_equal(got["fstat"][..., blk].view(np.uint32), r.fstat[..., off:off + W].view(np.uint32))
        want = np.array([(x["pos"], x["lib"], x["len"]) for x in r.indels], np.float64).reshape(-1, 3)
        np.testing.assert_array_equal(got["indel_key"][n_ind:n_ind + len(want), :3], want)
        np.testing.assert_array_equal(got["indel_istat"][n_ind:n_ind + len(want)], np.array([x["i"] for x in r.indels], np.float64).reshape(-1, 9))
        n_ind += len(want)
