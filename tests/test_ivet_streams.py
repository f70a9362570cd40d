"""brc_ivet_records on a caller's stream, by test_side_streams' technique (late inputs behind a bounded hold): brc_indels_gather with
sizes already known, brc_ivet_records over the table where the gather leaves it, and brc_panel_gather are queued back to back on a
non-default stream, behind a hold and the late copy of the real inputs over a decoy.  The call must return while the hold runs; after
ONE synchronisation every destination must hold, byte for byte and sentinels included, what the CPU builds of the three libraries give
for the real contents.  A launch, a memset (the status clear, the keep clear, the heads' fill) or a timing event that strayed to the
default stream would meet the decoy, or be covered by the sentinel fill.

In the CPU suite the chain runs on the CPU builds and the filter's part of it is compared with test_ivet's numpy predicate."""
import numpy as np
import pytest

from bam_readcount_amd import capi
from route import Route
import test_indels as ti
import test_ivet as tiv
import test_side_streams as tss
import test_vet as tv

ROLE = [tiv.CASE, tiv.CTL]
THR = tiv.T_(min_depth=2, min_var_count=2, freq_num=1, freq_den=10, ctl_max_count=0, ctl_min_depth=1)
TABLE = ("pos", "lib", "len", "istat", "fstat", "allele_off", "alleles")
PAD = tss.PAD
# the filter's list: positions with indel records (one of them twice), positions without, the last one out of range
LIST = np.array([2, 63, 64, 64, 100, 255, 256, 300, 599, tss.P], np.int32)


LIBS = tss.LIBS + ("ivet",)


def chain_job(sc, expect):
    """indels.gather (exact capacities) -> ivet over the gathered table and LIST -> panel over the scene's list"""
    gat = tss.indels_job(sc)
    real = ti.table_of(ti.window_of(sc.real.res, 0, tss.P))
    cap, acap = real["pos"].shape[1], int(real["alleles"].size)
    n, pn = LIST.size, tss.N_IDX
    ds, pds = cap + PAD, pn + PAD
    lst = sc.route.put(LIST)

    def sizes(route):
        s = dict(gat.sizes(route), **tss.plane_sizes(pds, "p."))
        s.update({"p.status": 4, "v.fail": 4 * ds, "v.vals": 4 * tiv.NVAL * ds, "v.ctl_count": 4 * ds, "v.keep": 4 * (n + PAD), "v.status": 4,
                  "v.ws": route.ivet.workspace(sc.v, cap)})
        return s

    def enqueue(route, buf, stream):
        rc = gat.enqueue(route, buf, stream)
        if rc:
            return rc
        par, keepalive = capi.ivet_params(ROLE, tiv.ALL_TESTS, tiv.INS | tiv.DEL, **THR)
        tab = capi.IVetTable(cap, cap, *[route.ptr(buf[k]) for k in TABLE], acap)
        rc = route.ivet.records_raw(sc.v, sc.d, par, tab, route.ptr(lst), None, n, ds, fail=route.ptr(buf["v.fail"]), vals=route.ptr(buf["v.vals"]),
                                    ctl_count=route.ptr(buf["v.ctl_count"]), keep=route.ptr(buf["v.keep"]), status=route.ptr(buf["v.status"]),
                                    workspace=route.ptr(buf["v.ws"]), stream=stream)
        del keepalive
        return rc or route.panel.gather_raw(sc.v, route.ptr(sc.keep["idx"]), pn, pds, status=route.ptr(buf["p.status"]), stream=stream,
                                            **{k: route.ptr(buf["p." + k]) for k in tss.td.KINDS})
    job = tss.Job("indels -> ivet -> panel", "ivet", sizes, enqueue, expect)
    job.cap, job.ds, job.lst = cap, ds, lst
    return job


def cpu_bytes(sim_route, seed):
    """the chain on the CPU builds over the scene of that seed: {buffer: bytes} of everything but the scratch"""
    sc = tss.Scene(sim_route, seed)
    job = chain_job(sc, None)
    rc, got, _ = tss.run_plain(sim_route, job)
    assert rc == 0, sim_route.ivet._call("_last_error")(sim_route.ivet.h)
    return sc, job, {k: np.array(b) for k, b in got.items() if not k.endswith("ws")}


@pytest.fixture(scope="module")
def sim_route():
    return Route("sim", LIBS)


def test_the_chain_on_the_cpu_builds_is_the_predicate(sim_route):
    sc, job, got = cpu_bytes(sim_route, 21)
    res = sc.real.res
    D = tv.Dense.of(res)
    T = tiv.Tab.of_oracle(res.indels)
    assert T.m == job.cap > 5
    wf, wv, wc, wk, wst = tiv.reference(D, T, LIST, None, ROLE, **THR)
    m, n = T.m, LIST.size
    assert np.array_equal(got["v.fail"].view(np.uint32)[:m], wf) and (got["v.fail"].view(np.uint32)[m:job.ds] == tiv.SENT).all()
    assert np.array_equal(got["v.vals"].view(np.uint32).reshape(tiv.NVAL, job.ds)[:, :m], wv.view(np.uint32))
    assert np.array_equal(got["v.ctl_count"].view(np.uint32)[:m], wc) and np.array_equal(got["v.keep"].view(np.uint32)[:n], wk)
    assert got["v.status"].view(np.uint32)[0] == wst == capi.IVET_LIST_OUT_OF_RANGE
    # the scene is worth the run: judged and unjudged records, a control veto, kept and unkept elements
    assert (wf == 0).any() and (wf & tiv.BIT["CTL_ALLELE"]).any() and (wf == tiv.NOT_ASKED).any() and wk.any() and not wk.all()
    # ... and with the decoy in place the filter's outputs come out otherwise
    sc.to_decoy()
    rc, decoy, _ = tss.run_plain(sim_route, job)
    assert rc == 0
    for k in ("v.fail", "v.vals", "v.keep", "p.depth"):
        assert not np.array_equal(decoy[k][:got[k].size], got[k]), k
    sc.to_real()


@pytest.fixture(scope="module")
def gpu(sim_route):
    """The hip route, one scene, the chain run once on the default stream (code objects loaded, the values checked there too, its warm
    host time taken), and the hold sized against it."""
    g = tss.Gpu()
    g.route = route = Route("hip", LIBS)
    g.torch = torch = route.torch
    _, _, want = cpu_bytes(sim_route, 21)
    g.scene = sc = tss.Scene(route, 21)
    g.job = job = chain_job(sc, lambda w: want)
    rc, got, dt = tss.run_plain(route, job)
    assert rc == 0, route.ivet._call("_last_error")(route.ivet.h)
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
def test_gather_ivet_and_panel_back_to_back_on_a_held_stream(gpu):
    wall, = tss.held(gpu, [(gpu.scene, gpu.job, 1.0)])
    t = gpu.route.ivet.last_timing()
    print("ivet: kernel_s %.6f, call to synchronised %.6f, hold %.6f" % (t["kernel_s"], wall, gpu.hold.seconds))
    assert 0 < t["kernel_s"] < wall and t["kernel_s"] < gpu.hold.seconds, (t, wall, gpu.hold.seconds)
