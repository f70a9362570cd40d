"""brc_inorm_table on a caller's stream, by test_side_streams' technique (late inputs behind a bounded hold): brc_indels_gather with
sizes already known, brc_inorm_table over the table where the gather leaves it, and brc_ivet_records over the normalised table are
queued back to back on a non-default stream, behind a hold and the late copy of the real inputs over a decoy.  The call must return
while the hold runs; after ONE synchronisation every destination must hold, byte for byte and sentinels included, what the CPU builds
of the three libraries give for the real contents.  A launch, a memset (the status clear, the counters' clear) or a timing event that
strayed to the default stream would meet the decoy, or be covered by the sentinel fill.  The sizes of the normalised table come from a
first, untimed call that asks for the counts alone.

In the CPU suite the chain runs on the CPU builds and its parts are compared with test_inorm's plain-Python reference and test_ivet's
numpy predicate."""
import numpy as np
import pytest

from bam_readcount_amd import capi
from route import Route
import test_indels as ti
import test_inorm as tn
import test_ivet as tiv
import test_side_streams as tss
import test_vet as tv

ROLE = [tiv.CASE, tiv.CTL]
THR = tiv.T_(min_depth=2, min_var_count=2, freq_num=1, freq_den=10, ctl_max_count=0, ctl_min_depth=1)
TABLE = ("pos", "lib", "len", "rep_read", "rep_qpos", "istat", "fstat", "allele_off", "alleles")
NTAB = ("pos", "lib", "len", "istat", "fstat", "allele_off", "alleles")
PER_OUT = {"pos": 1, "lib": 1, "len": 1, "rep_read": 1, "rep_qpos": 1, "members": 1, "istat": 9, "fstat": 4, "metrics": 13}
PAD = tss.PAD
SEED = 21


LIBS = tss.LIBS + ("ivet", "inorm")


def source_of(route, buf, cap, acap):
    return capi.INormSource(cap, cap, *[route.ptr(buf[k]) for k in TABLE], acap)


def counted(route, sc, gat, cap, acap):
    """the first, untimed call: the gather and brc_inorm_table for its two counts alone, on the default stream; the host reads them"""
    buf = {k: route.sentinel_bytes(max(n, 8)) for k, n in gat.sizes(route).items()}
    buf["n.counts"], buf["n.ws"] = route.sentinel_bytes(8), route.sentinel_bytes(max(route.inorm.workspace(tss.P, cap), 8))
    assert gat.enqueue(route, buf, None) == 0
    route.inorm.table(sc.d, capi.INormParams(1024), source_of(route, buf, cap, acap), 0, tss.P, workspace=route.ptr(buf["n.ws"]),
                      workspace_bytes=route.inorm.workspace(tss.P, cap), counts=route.ptr(buf["n.counts"]))
    return [int(x) for x in route.host(buf["n.counts"])[:8].view(np.uint32)]


def chain_job(sc, expect):
    """indels.gather (exact capacities) -> inorm over the gathered table (exact capacities) -> ivet over the normalised table"""
    gat = tss.indels_job(sc)
    real = ti.table_of(ti.window_of(sc.real.res, 0, tss.P))
    cap, acap = real["pos"].shape[1], int(real["alleles"].size)
    mm, nb = counted(sc.route, sc, gat, cap, acap)
    ds = mm + PAD

    def sizes(route):
        s = dict(gat.sizes(route))
        s.update({"n." + k: 4 * (pl * mm + PAD) for k, pl in PER_OUT.items()})
        s.update({"n." + k: 4 * (cap + PAD) for k in tn.PER_IN})
        s.update({"n.allele_off": 4 * (mm + 1 + PAD), "n.alleles": nb + PAD, "n.counts": 8, "n.status": 4, "n.ws": route.inorm.workspace(tss.P, cap)})
        s.update({"v.fail": 4 * ds, "v.vals": 4 * tiv.NVAL * ds, "v.ctl_count": 4 * ds, "v.status": 4, "v.ws": route.ivet.workspace(sc.v, mm)})
        return s

    def enqueue(route, buf, stream):
        rc = gat.enqueue(route, buf, stream)
        if rc:
            return rc
        rc = route.inorm.table_raw(sc.d, capi.INormParams(1024), source_of(route, buf, cap, acap), 0, tss.P, workspace=route.ptr(buf["n.ws"]),
                                   workspace_bytes=route.inorm.workspace(tss.P, cap), cap=mm, alleles_cap=nb, stream=stream,
                                   **{k: route.ptr(buf["n." + k]) for k in tn.EVERY})
        if rc:
            return rc
        par, keepalive = capi.ivet_params(ROLE, tiv.ALL_TESTS, tiv.INS | tiv.DEL, **THR)
        tab = capi.IVetTable(mm, mm, *[route.ptr(buf["n." + k]) for k in NTAB], nb)
        rc = route.ivet.records_raw(sc.v, sc.d, par, tab, None, None, 0, ds, fail=route.ptr(buf["v.fail"]), vals=route.ptr(buf["v.vals"]),
                                    ctl_count=route.ptr(buf["v.ctl_count"]), status=route.ptr(buf["v.status"]), workspace=route.ptr(buf["v.ws"]), stream=stream)
        del keepalive
        return rc
    job = tss.Job("indels -> inorm -> ivet", "inorm", sizes, enqueue, expect)
    job.cap, job.acap, job.mm, job.nb, job.ds = cap, acap, mm, nb, ds
    return job


def cpu_bytes(sim_route, seed):
    """the chain on the CPU builds over the scene of that seed: {buffer: bytes} of everything but the scratch"""
    sc = tss.Scene(sim_route, seed)
    job = chain_job(sc, None)
    rc, got, _ = tss.run_plain(sim_route, job)
    assert rc == 0, sim_route.inorm._call("_last_error")(sim_route.inorm.h)
    return sc, job, {k: np.array(b) for k, b in got.items() if not k.endswith("ws")}


@pytest.fixture(scope="module")
def sim_route():
    return Route("sim", LIBS)


def test_the_chain_on_the_cpu_builds_is_the_reference(sim_route):
    sc, job, got = cpu_bytes(sim_route, SEED)
    res = sc.real.res
    T = tiv.Tab.of_oracle(res.indels)
    assert T.m == job.cap > 5
    V = tn.View.of_engine(sc.d, b"N" * (tss.POS0 + tss.REF_SLICE[0]) + bytes(np.asarray(sim_route.host(sc.keep["ref"])).view(np.uint8)))
    W = tn.norm_reference(V, T)
    tn.props(V, T, W, 1024)
    e = tn.expected(W, T, job.mm, job.nb)
    assert (job.mm, job.nb) == (len(W["merged"]), sum(len(g["text"]) for g in W["merged"]))
    for k in tn.EVERY:
        g = got["n." + k]
        w = e[k][:g.size // e[k].itemsize] if k != "alleles" else e[k][:g.size]
        assert np.array_equal(g.view(w.dtype)[:w.size], w), k
    # the scene is worth the run: a record that moved, and the filter judged the normalised table
    assert any(W["shift"]) and W["status"] == 0
    wf, wv, wc, wk, wst = tiv.reference(tv.Dense.of(res), tn.merged_tab(W), None, None, ROLE, **THR)
    assert np.array_equal(got["v.fail"].view(np.uint32)[:job.mm], wf) and (got["v.fail"].view(np.uint32)[job.mm:job.ds] == tiv.SENT).all()
    assert np.array_equal(got["v.vals"].view(np.uint32).reshape(tiv.NVAL, job.ds)[:, :job.mm], wv.view(np.uint32))
    assert np.array_equal(got["v.ctl_count"].view(np.uint32)[:job.mm], wc) and got["v.status"].view(np.uint32)[0] == wst
    # ... and with the decoy in place the outputs come out otherwise
    sc.to_decoy()
    rc, decoy, _ = tss.run_plain(sim_route, job)
    assert rc == 0
    for k in ("n.counts", "n.npos", "v.fail"):
        assert not np.array_equal(decoy[k][:got[k].size], got[k]), k
    sc.to_real()


@pytest.fixture(scope="module")
def gpu(sim_route):
    """The hip route, one scene, the chain run once on the default stream (code objects loaded, the values checked there too, its warm
    host time taken), and the hold sized against it."""
    g = tss.Gpu()
    g.route = route = Route("hip", LIBS)
    g.torch = torch = route.torch
    _, sim_job, want = cpu_bytes(sim_route, SEED)
    g.scene = sc = tss.Scene(route, SEED)
    g.job = job = chain_job(sc, lambda w: want)
    assert (job.mm, job.nb) == (sim_job.mm, sim_job.nb)
    rc, got, dt = tss.run_plain(route, job)
    assert rc == 0, route.inorm._call("_last_error")(route.inorm.h)
    tss.compare(got, want, "chain [default stream]")
    torch.cuda.synchronize()
    _, _, dt = tss.run_plain(route, job)
    torch.cuda.synchronize()
    g.hold = tss.Hold(torch, dt)
    g.streams = tss.streams_beside_the_default(torch, g.hold)
    assert len(g.streams) >= 1, "INCONCLUSIVE: no stream runs beside the default stream on this machine"
    print("\nhold: %d ticks = %.4f s; warm host-side time of the three calls: %.1f us" % (g.hold.ticks, g.hold.seconds, 1e6 * dt))
    return g


@pytest.mark.gpu
def test_gather_inorm_and_ivet_back_to_back_on_a_held_stream(gpu):
    wall, = tss.held(gpu, [(gpu.scene, gpu.job, 1.0)])
    t = gpu.route.inorm.last_timing()
    print("inorm: kernel_s %.6f, call to synchronised %.6f, hold %.6f" % (t["kernel_s"], wall, gpu.hold.seconds))
    assert 0 < t["kernel_s"] < wall and t["kernel_s"] < gpu.hold.seconds, (t, wall, gpu.hold.seconds)
