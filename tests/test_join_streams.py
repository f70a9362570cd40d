"""brc_join_views on a caller's stream, by test_side_streams' technique (late inputs behind a bounded hold): the join of two sources
over a window wider than both, brc_dense_expand over the joined view and brc_select_sites over the joined views are queued back to
back on a non-default stream, behind a hold and the late copy of the real inputs over a decoy.  The calls must return while the hold
runs; after ONE synchronisation every destination must hold, byte for byte and sentinels included, what the CPU builds of the three
libraries give for the real contents.  A launch, a memset (the status clear, the counts' clear) or a timing event that strayed to the
default stream would meet the decoy, or be covered by the sentinel fill.  The bytes of the synthetic reads and the selection's
capacity come from a first, untimed call.

The two sources are the scene's views, twice: libraries 0, 1 and again as 2, 3 — sources may share memory, destinations may not.

In the CPU suite the chain runs on the CPU builds and its parts are compared with test_dense's and test_select's references of the
scene, placed at the sources' offset."""
import numpy as np
import pytest

from bam_readcount_amd import capi
from route import Route
import test_dense as td
import test_join as tj
import test_side_streams as tss

PAD = tss.PAD
SEED = 21
LEAD, TAIL = 7, 9                               # the joined window starts 7 positions before the sources and ends 9 behind them
POS0, N = tss.POS0 - LEAD, tss.P + LEAD + TAIL
L = 2 * tss.L
ROLE, SEL_P = [1, 2, 1, 2], tss.SEL_P
KINDS = ("istat", "fstat", "depth", "ncol", "unavail")


LIBS = tss.LIBS + ("join",)


def sources_of(sc):
    return capi.join_sources([(sc.v, sc.d), (sc.v, sc.d)])


def counted(route, sc):
    """the first, untimed call: the join for its two counts alone, on the default stream; the host reads them"""
    src = sources_of(sc)
    z = route.join.sizes(src, POS0, N, N)
    ws, c = route.sentinel_bytes(max(int(z.workspace_bytes), 8)), route.sentinel_bytes(8)
    route.join.views(src, POS0, N, N, counts=route.ptr(c), workspace=route.ptr(ws), workspace_bytes=int(z.workspace_bytes))
    return z, [int(x) for x in route.host(c)[:8].view(np.uint32)]


def chain_job(sc, expect):
    """join (exact seq_cap) -> dense.expand over the joined view -> select over the joined views"""
    route = sc.route
    z, (kept, nbytes) = counted(route, sc)
    cap = len(sc.real.h.want(ROLE[:2], SEL_P, 0, tss.P)[0])
    ds = N + PAD
    shape = capi.DeviceView(route.mem, 0, L, POS0, N, N, n_xagg=int(z.n_xagg)), capi.DeviceIndels(route.mem, 0, L, POS0, N, None, int(z.n_slots))
    select_ws = route.select.workspace(shape[0], shape[1], N)             # (a function of the joined views' sizes, which the host knows)

    def sizes(route):
        s = {"j." + k: int(getattr(z, k + "_bytes")) + 4 * PAD for k in capi.JOIN_DESTS if k != "seq4"}
        s.update({"j.seq4": nbytes + 4 * PAD, "j.counts": 8, "j.status": 4, "j.ws": int(z.workspace_bytes)})
        s.update({"d." + k: 4 * td.planes_of(k, L) * ds for k in KINDS})
        s.update({"s.counts": 4, "s.idx": 4 * (cap + PAD), "s.why": 4 * (cap + PAD), "s.ws": select_ws})
        return s

    def enqueue(route, buf, stream):
        v, d = capi.DeviceView(), capi.DeviceIndels()
        dest = capi.JoinDest(**{k: route.ptr(buf["j." + k]) for k in capi.JOIN_DESTS})
        rc = route.join.views_raw(sources_of(sc), POS0, N, N, dest=dest, out_view=v, out_indels=d, counts=route.ptr(buf["j.counts"]), seq_cap=nbytes,
                                  status=route.ptr(buf["j.status"]), workspace=route.ptr(buf["j.ws"]), workspace_bytes=int(z.workspace_bytes), stream=stream)
        if rc:
            return rc
        rc = route.dense.expand_raw(v, 0, N, ds, stream=stream, **{k: route.ptr(buf["d." + k]) for k in KINDS})
        if rc:
            return rc
        if route.select.workspace(v, d, N) != select_ws:
            return -99
        par, keep = capi.select_params(ROLE, SEL_P["flags"], SEL_P["min_depth"], SEL_P["min_alt"], SEL_P["frac"], SEL_P["ctl_min_depth"], SEL_P["ctl_max_alt"], SEL_P["ctl_frac"])
        rc = route.select.sites_raw(v, d, par, 0, N, cap=cap, idx=route.ptr(buf["s.idx"]), why=route.ptr(buf["s.why"]), counts=route.ptr(buf["s.counts"]),
                                    workspace=route.ptr(buf["s.ws"]), stream=stream)
        del keep
        return rc
    job = tss.Job("join -> dense -> select", "join", sizes, enqueue, expect)
    job.z, job.kept, job.nbytes, job.cap, job.ds = z, kept, nbytes, cap, ds
    return job


def cpu_bytes(sim_route, seed):
    """the chain on the CPU builds over the scene of that seed: {buffer: bytes} of everything but the scratch"""
    sc = tss.Scene(sim_route, seed)
    job = chain_job(sc, None)
    rc, got, _ = tss.run_plain(sim_route, job)
    assert rc == 0, sim_route.join._call("_last_error")(sim_route.join.h)
    return sc, job, {k: np.array(b) for k, b in got.items() if not k.endswith("ws")}


@pytest.fixture(scope="module")
def sim_route():
    return Route("sim", LIBS)


def test_the_chain_on_the_cpu_builds_is_the_reference(sim_route):
    sc, job, got = cpu_bytes(sim_route, SEED)
    res = sc.real.res
    assert job.kept == 2 * len(tss.INDELS) and job.z.n_xagg == 2 * sc.v.n_xagg > 6 and job.z.n_lib == L
    assert (job.z.ref_lo, job.z.ref_hi) == (tss.POS0 + tss.REF_SLICE[0], tss.POS0 + tss.REF_SLICE[1]) and got["j.status"].view(np.uint32)[0] == 0
    # the dense expansion: the scene's own planes at the sources' offset, twice, and empty positions around them
    want = td.want_planes(res, 0, tss.P)
    for k in KINDS:
        rows = td.planes_of(k, tss.L)
        g = got["d." + k].view(np.uint32).reshape(-1, job.ds)
        assert (g[:, N:] == tj.SENT).all(), k
        if k == "unavail":
            assert (g[:, :N] == tj.NONE32).all()
            continue
        for half in (0, 1):
            h = g[half * rows:(half + 1) * rows]
            assert np.array_equal(h[:, LEAD:LEAD + tss.P], want[k].reshape(rows, tss.P)), (k, half)
            assert not h[:, :LEAD].any() and not h[:, LEAD + tss.P:N].any(), (k, half)
    # the selection: libraries 2, 3 repeat 0, 1 — what the scene's own reference selects, LEAD positions further on
    widx, wwhy = sc.real.h.want(ROLE[:2], SEL_P, 0, tss.P)
    assert got["s.counts"].view(np.uint32)[0] == len(widx) == job.cap > 10
    assert np.array_equal(got["s.idx"].view(np.int32)[:job.cap], np.asarray(widx) + LEAD) and np.array_equal(got["s.why"].view(np.uint32)[:job.cap], np.asarray(wwhy, np.uint32))
    # ... and with the decoy in place the outputs come out otherwise
    sc.to_decoy()
    rc, decoy, _ = tss.run_plain(sim_route, job)
    assert rc == 0
    for k in ("j.depth", "j.slots", "j.ref", "d.istat", "s.counts"):
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
    assert (job.kept, job.nbytes, job.cap) == (sim_job.kept, sim_job.nbytes, sim_job.cap)
    rc, got, dt = tss.run_plain(route, job)
    assert rc == 0, route.join._call("_last_error")(route.join.h)
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
def test_join_dense_and_select_back_to_back_on_a_held_stream(gpu):
    wall, = tss.held(gpu, [(gpu.scene, gpu.job, 1.0)])
    t = gpu.route.join.last_timing()
    print("join: kernel_s %.6f, call to synchronised %.6f, hold %.6f" % (t["kernel_s"], wall, gpu.hold.seconds))
    assert 0 < t["kernel_s"] < wall and t["kernel_s"] < gpu.hold.seconds, (t, wall, gpu.hold.seconds)
    assert t["bytes_written"] >= 116 * N * L
