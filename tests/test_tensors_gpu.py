"""bam_readcount_amd.tensors.region on the GPU: CUDA tensors filled by libbrc_dense_hip.so on torch's current stream, equal to the
oracle's dense result; later torch work on that stream sees them without a host synchronisation."""
import numpy as np
import pytest

from bam_readcount_amd import capi
from test_dense import computed, oracle_result, want_planes

pytestmark = pytest.mark.gpu

NAMES = ["libA", "libB", "libC", "libD"]
OPTS = dict(lib_names=NAMES, per_lib=True, insertion_centric=True, min_mapq=20, min_bq=13)


@pytest.fixture(scope="module")
def tumor():
    import synthgen as gen
    return gen.generate(200_000, "tumor200x", seed=7, n_chunks=8)


def _check(r, res, kinds):
    want = want_planes(res, 0, res.n_pos)
    for k in kinds:
        assert r[k].is_cuda and r[k].is_contiguous()
        assert np.array_equal(r[k].cpu().numpy().view(np.uint32).reshape(want[k].shape), want[k]), k


def test_region_returns_cuda_tensors_equal_to_the_oracle(hip_lib, oracle_lib, tumor):
    import torch
    from bam_readcount_amd import tensors
    ref, arrs = tumor
    dense = capi.Dense()
    assert dense.kind() == "hip-gfx950"
    eng = computed(hip_lib, arrs, 1000, 21000, ref, **OPTS)
    res, _ = oracle_result(oracle_lib, arrs, 1000, 21000, ref, **OPTS)
    assert res.n_lib == 4 and res.n_pos >= 20000
    # a reduction queued right behind the call, no synchronisation in between: .item() waits for the reduction only
    r = tensors.region(eng, dense)
    total = r["depth"].to(torch.int64).sum()
    assert int(total.item()) == int(res.depth.astype(np.int64).sum())
    assert (r["pos0"], r["first"], r["n"], r["n_lib"]) == (res.pos0, res.pos0, res.n_pos, 4)
    assert r["istat"].dtype == torch.uint32 and r["metrics"].dtype == torch.float32 and r["istat"].device == torch.device("cuda", 0)
    assert tuple(r["metrics"].shape) == (4, 6, 13, res.n_pos)
    _check(r, res, tensors.DEFAULT_WANT)
    # the same on a stream of the caller's choosing
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        r2 = tensors.region(eng, dense, want=("istat", "unavail"))
        reads = r2["istat"][:, :, 0, :].to(torch.int64).sum()
        assert int(reads.item()) == int(res.istat[:, :, 0, :].astype(np.int64).sum())
        _check(r2, res, ("istat", "unavail"))          # (copies queued on the same stream)
    # a use on the device: allele fractions of A C G T, compared with the same arithmetic on the oracle's planes
    af = r["istat"][:, 1:5, 0, :].to(torch.float32) / r["depth"].to(torch.float32).clamp(min=1)[:, None, :]
    want_af = res.istat[:, 1:5, 0, :].astype(np.float32) / np.maximum(res.depth.astype(np.float32), 1)[:, None, :]
    assert np.array_equal(af.cpu().numpy(), want_af)
    torch.cuda.synchronize()

    # a second region on the same engine gives its own results (everything queued on the first has run: the lifetime rule);
    # the first region's tensors are the caller's and keep their values
    eng.begin_region(0, 30000, 42000, ref)
    idx = capi.fetch_overlapping(arrs, capi.read_ends(arrs), 29999, 42000)
    eng.push_reads(capi.select_reads(arrs, idx)); eng.upload(); eng.compute()
    res_b, _ = oracle_result(oracle_lib, arrs, 30000, 42000, ref, **OPTS)
    rb = tensors.region(eng, dense, want=tensors.KINDS)
    assert rb["pos0"] == res_b.pos0 and rb["n"] == res_b.n_pos
    _check(rb, res_b, tensors.KINDS)
    _check(r, res, tensors.DEFAULT_WANT)
    torch.cuda.synchronize()
    t = dense.last_timing()
    assert t["kernel_s"] > 0 and t["bytes_written"] == 4 * res_b.n_pos * (4 * (2 + 6 * 26) + 1)
    eng.close(); dense.close()


def test_engine_created_before_torch_is_imported(tmp_path):
    """The order of a caller who meets torch late, in a process of its own: engine and dense handle created and a region computed
    BEFORE torch is imported; tensors.region then imports it, and torch finds the GPU the engine is on (one HIP runtime in the
    process: capi._load) and reads what the kernels wrote."""
    import subprocess
    import sys
    from conftest import ROOT
    script = tmp_path / "late_torch.py"
    script.write_text('''
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r + "/tools"); sys.path.insert(0, %r + "/tests")
import numpy as np
import synthgen
from bam_readcount_amd import capi, tensors
from test_dense import computed
ref, arrs = synthgen.generate(50_000, "wgs30x", seed=5, n_chunks=2)
eng = computed(capi.load_product(), arrs, 1000, 9000, ref, min_mapq=20, min_bq=13)
dense = capi.Dense()
want = eng.fetch_result()
assert "torch" not in sys.modules
r = tensors.region(eng, dense)
import torch
assert r["depth"].is_cuda and r["n"] == want.n_pos
assert int(r["depth"].to(torch.int64).sum().item()) == int(want.depth.astype(np.int64).sum()) > 0
assert np.array_equal(r["istat"].cpu().numpy(), want.istat)
assert np.array_equal(r["fstat"].cpu().numpy().view(np.uint32), want.fstat.view(np.uint32))
torch.cuda.synchronize(); eng.close(); dense.close()
print("LATE TORCH OK")
''' % (ROOT, ROOT, ROOT))
    p = subprocess.run([sys.executable, str(script)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0 and b"LATE TORCH OK" in p.stdout, p.stderr.decode()[-3000:]
