"""`bench.py` on the GPU, plain and with `--full`: a plain run sets up, warms up, times the steps and prints the line, and every
measurement or check beyond that — validation against the oracle, cpu_baseline, e2e, abi_roundtrip, other_configs — is null on it;
`--full` runs them.  Both lines carry the same headline fields, and the step they time is the same one (events, positions)."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

SHAPE = ["--gpus", "1", "--mode", "weak", "--contig-mbp", "2", "--steps", "3", "--warmup", "1"]
EXTRAS = ("cpu_baseline", "e2e", "e2e_sites", "e2e_tumor", "e2e_sharded", "abi_roundtrip", "validated", "other_configs")


def run_bench(extra):
    run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SHAPE + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert run.returncode == 0, run.stderr.decode()[-3000:]
    out = [l for l in run.stdout.decode().splitlines() if l.strip()]
    return json.loads(out[-1])                           # the result line is the last line of stdout


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_nothing_else_and_full_adds_the_rest():
    plain = run_bench([])
    assert plain["full"] is False and all(plain[k] is None for k in EXTRAS), {k: plain[k] for k in EXTRAS}
    assert plain["metric"] == "pileup base-events/sec" and plain["unit"] == "events/s" and plain["higher_is_better"] is True and plain["dtype"] == "u32+f32"
    assert plain["steps"] == 3 and plain["warmup"] == 1 and plain["ms_per_step"] > 0
    assert plain["value"] == pytest.approx(plain["config"]["events_per_step"] / (plain["ms_per_step"] * 1e-3), rel=1e-3)
    assert plain["roofline"]["kernel_ms"]["k_pileup"] > 0
    # the sizes of the legs are read only with --full: naming one does not bring its leg back
    assert run_bench(["--cpu-sample-mbp", "0.5", "--abi-mbp", "1"])["validated"] is None
    full = run_bench(["--full", "--cpu-sample-mbp", "0.5", "--cpu-ref-mbp", "0", "--e2e-mbp", "1", "--abi-mbp", "1", "--other-configs", "0", "--e2e-configs", "0"])
    v = full["validated"]
    assert full["full"] is True and v["events_equal_sum_of_spans"] and v["planes_bit_exact"] and v["text_byte_exact"] and v["device_text_byte_exact"] and v["full_contig"] is True
    assert full["cpu_baseline"]["value"] > 0 and full["cpu_baseline"]["all_cores"]["value"] > 0
    assert full["e2e"]["value"] > 0 and full["abi_roundtrip"]["value"] > 0
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup"):
        assert full[k] == plain[k]
    assert full["config"] == plain["config"] and full["value"] > 0
