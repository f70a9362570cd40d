"""brc_cons_call on a caller's stream, by test_side_streams' technique (late inputs behind a bounded hold): brc_indels_gather with sizes
already known, brc_inorm_table over the table where the gather leaves it, brc_cons_call over the normalised table and brc_dense_expand
over the same window are queued back to back on a non-default stream, behind a hold and the late copy of the real inputs over a decoy.
The calls must return while the hold runs; after ONE synchronisation every destination must hold, byte for byte and sentinels
included, what the CPU builds of the four libraries give for the real contents.  A launch, a memset (the status clear, the difference
array's and the run words' presets) or a timing event that strayed to the default stream would meet the decoy, or be covered by the
sentinel fill.  The sizes — the normalised table's and the sequence's — come from a first, untimed call that asks for the counts alone.

In the CPU suite the chain runs on the CPU builds and the consensus is compared with test_cons' plain-Python reference over
test_inorm's reference of the normalised table."""
import numpy as np
import pytest

from bam_readcount_amd import capi
from bam_readcount_amd import consensus as cc
from route import Route
import test_cons as tc
import test_dense as td
import test_indels as ti
import test_inorm as tn
import test_inorm_streams as tis
import test_ivet as tiv
import test_side_streams as tss

PAD = tss.PAD
SEED = 21
K0, N = tss.K0, tss.N
P = dict(min_depth=2, min_count=1, num=1, den=4, ins_min_count=1, ins_num=1, ins_den=10)
KINDS = ("istat", "depth")
LIBS = tss.LIBS + ("inorm",)
CDEST = ("call", "cnt", "ins_rec", "off", "seq")


def route_of(name):
    r = Route(name, LIBS)
    r.cons = tc.cons_handle(r)
    return r


def params():
    return cc.cons_params(None, 0, P["min_depth"], P["min_count"], (P["num"], P["den"]), P["ins_min_count"], (P["ins_num"], P["ins_den"]))


def cons_table(route, buf, mm, nb):
    """the normalised table where brc_inorm_table leaves it: count is row BRC_I_N of its istat planes"""
    return cc.ConsTable(mm, mm, route.ptr(buf["n.pos"]), route.ptr(buf["n.lib"]), route.ptr(buf["n.len"]), route.ptr(buf["n.istat"]), route.ptr(buf["n.allele_off"]),
                        route.ptr(buf["n.alleles"]), nb)


def chain_job(sc, expect):
    """indels.gather (exact capacities) -> inorm (exact capacities) -> cons (exact seq_cap) -> dense.expand"""
    gat = tss.indels_job(sc)
    real = ti.table_of(ti.window_of(sc.real.res, 0, tss.P))
    cap, acap = real["pos"].shape[1], int(real["alleles"].size)
    route = sc.route
    mm, nb = tis.counted(route, sc, gat, cap, acap)
    ds = N + PAD
    wsb = route.cons.workspace(sc.v, N, mm)

    def sizes(route, total=0):
        s = dict(gat.sizes(route))
        s.update({"n." + k: 4 * (pl * mm + PAD) for k, pl in tis.PER_OUT.items()})
        s.update({"n." + k: 4 * (cap + PAD) for k in tn.PER_IN})
        s.update({"n.allele_off": 4 * (mm + 1 + PAD), "n.alleles": nb + PAD, "n.counts": 8, "n.status": 4, "n.ws": route.inorm.workspace(tss.P, cap)})
        s.update({"c.counts": 4, "c.status": 4, "c.call": N + PAD, "c.cnt": 4 * 6 * ds, "c.ins_rec": 4 * (N + PAD), "c.off": 4 * (N + 1 + PAD), "c.seq": total + PAD,
                  "c.ws": wsb})
        s.update({"d." + k: 4 * td.planes_of(k, tss.L) * ds for k in KINDS})
        return s

    def enqueue(route, buf, stream, seq_cap=None):
        rc = gat.enqueue(route, buf, stream)
        if rc:
            return rc
        rc = route.inorm.table_raw(sc.d, capi.INormParams(1024), tis.source_of(route, buf, cap, acap), 0, tss.P, workspace=route.ptr(buf["n.ws"]),
                                   workspace_bytes=route.inorm.workspace(tss.P, cap), cap=mm, alleles_cap=nb, stream=stream,
                                   **{k: route.ptr(buf["n." + k]) for k in tn.EVERY})
        if rc:
            return rc
        par, keepalive = params()
        dests = {k: route.ptr(buf["c." + k]) for k in CDEST} if seq_cap is None else {}
        rc = route.cons.call_raw(sc.v, sc.d, par, cons_table(route, buf, mm, nb), K0, N, ds, seq_cap=job.total if seq_cap is None else seq_cap,
                                 counts=route.ptr(buf["c.counts"]), status=route.ptr(buf["c.status"]), workspace=route.ptr(buf["c.ws"]), stream=stream, **dests)
        del keepalive
        if rc or seq_cap is not None:
            return rc
        return route.dense.expand_raw(sc.v, K0, N, ds, stream=stream, **{k: route.ptr(buf["d." + k]) for k in KINDS})
    job = tss.Job("indels -> inorm -> cons -> dense", "cons", sizes, enqueue, expect)
    job.cap, job.acap, job.mm, job.nb, job.ds = cap, acap, mm, nb, ds
    # the first, untimed call: the chain up to the consensus for its count alone, on the default stream; the host reads it
    buf = {k: route.sentinel_bytes(max(n, 8)) for k, n in sizes(route).items()}
    assert enqueue(route, buf, None, seq_cap=0) == 0, route.cons._call("_last_error")(route.cons.h)
    job.total = int(route.host(buf["c.counts"])[:4].view(np.uint32)[0])
    job.sizes = lambda route: sizes(route, job.total)
    return job


def cpu_bytes(sim_route, seed):
    """the chain on the CPU builds over the scene of that seed: {buffer: bytes} of everything but the scratch"""
    sc = tss.Scene(sim_route, seed)
    job = chain_job(sc, None)
    rc, got, _ = tss.run_plain(sim_route, job)
    assert rc == 0, sim_route.cons._call("_last_error")(sim_route.cons.h)
    return sc, job, {k: np.array(b) for k, b in got.items() if not k.endswith("ws")}


@pytest.fixture(scope="module")
def sim_route():
    return route_of("sim")


def test_the_chain_on_the_cpu_builds_is_the_reference(sim_route):
    sc, job, got = cpu_bytes(sim_route, SEED)
    res = sc.real.res
    T = tiv.Tab.of_oracle(res.indels)
    V = tn.View.of_engine(sc.d, b"N" * (tss.POS0 + tss.REF_SLICE[0]) + bytes(np.asarray(sim_route.host(sc.keep["ref"])).view(np.uint8)))
    W = tn.norm_reference(V, T)
    assert (job.mm, job.nb) == (len(W["merged"]), sum(len(g["text"]) for g in W["merged"])) and any(W["shift"])
    w = tc.reference(res.istat[:, 1:5, 0, :], res.refbase, tss.POS0, tn.merged_tab(W), K0, N, **P)
    assert w["counts"] == job.total == got["c.counts"].view(np.uint32)[0] and got["c.status"].view(np.uint32)[0] == w["status"] == 0
    assert np.array_equal(got["c.call"][:N], w["call"]) and (got["c.call"][N:] == tc.SENT8).all()
    assert np.array_equal(got["c.cnt"].view(np.uint32).reshape(6, job.ds)[:, :N], w["cnt"]) and (got["c.cnt"].view(np.uint32).reshape(6, job.ds)[:, N:] == tc.SENT).all()
    assert np.array_equal(got["c.ins_rec"].view(np.uint32)[:N], w["ins_rec"]) and np.array_equal(got["c.off"].view(np.uint32)[:N + 1], w["off"])
    assert np.array_equal(got["c.seq"][:job.total], w["seq"]) and (got["c.seq"][job.total:] == tc.SENT8).all()
    # the scene is worth the run: positions under deletions, accepted insertions and two-base codes
    assert (w["cnt"][4] != 0).sum() >= 4 and (w["ins_rec"] != tc.NO_INS).sum() >= 2 and job.total != N and set(bytes(w["call"])) & set(b"MRWSYK")
    want = td.want_planes(res, K0, N)
    for k in KINDS:
        g = got["d." + k].view(np.uint32).reshape(-1, job.ds)
        assert np.array_equal(g[:, :N], want[k].reshape(-1, N)) and (g[:, N:] == tc.SENT).all(), k
    # ... and with the decoy in place the outputs come out otherwise
    sc.to_decoy()
    rc, decoy, _ = tss.run_plain(sim_route, job)
    assert rc == 0
    for k in ("n.counts", "c.call", "c.cnt", "c.off", "c.seq", "d.depth"):
        assert not np.array_equal(decoy[k][:got[k].size], got[k]), k
    sc.to_real()


@pytest.fixture(scope="module")
def gpu(sim_route):
    """The hip route, one scene, the chain run once on the default stream (code objects loaded, the values checked there too, its warm
    host time taken), and the hold sized against it."""
    g = tss.Gpu()
    g.route = route = route_of("hip")
    g.torch = torch = route.torch
    _, sim_job, want = cpu_bytes(sim_route, SEED)
    g.scene = sc = tss.Scene(route, SEED)
    g.job = job = chain_job(sc, lambda w: want)
    assert (job.mm, job.nb, job.total) == (sim_job.mm, sim_job.nb, sim_job.total)
    rc, got, dt = tss.run_plain(route, job)
    assert rc == 0, route.cons._call("_last_error")(route.cons.h)
    tss.compare(got, want, "chain [default stream]")
    torch.cuda.synchronize()
    _, _, dt = tss.run_plain(route, job)
    torch.cuda.synchronize()
    g.hold = tss.Hold(torch, dt)
    g.streams = tss.streams_beside_the_default(torch, g.hold)
    assert len(g.streams) >= 1, "INCONCLUSIVE: no stream runs beside the default stream on this machine"
    print("\nhold: %d ticks = %.4f s; warm host-side time of the four calls: %.1f us" % (g.hold.ticks, g.hold.seconds, 1e6 * dt))
    return g


@pytest.mark.gpu
def test_gather_inorm_cons_and_dense_back_to_back_on_a_held_stream(gpu):
    wall, = tss.held(gpu, [(gpu.scene, gpu.job, 1.0)])
    t = gpu.route.cons.last_timing()
    print("cons: kernel_s %.6f, call to synchronised %.6f, hold %.6f" % (t["kernel_s"], wall, gpu.hold.seconds))
    assert 0 < t["kernel_s"] < wall and t["kernel_s"] < gpu.hold.seconds, (t, wall, gpu.hold.seconds)
    assert t["bytes_read"] >= 12 * N * tss.L
