"""brc_vet_sites on a caller's stream, in the chain it was built for: brc_select_sites (the list already sized), brc_vet_sites over the
list and the reason words where they lie, and brc_panel_gather over the same list, queued back to back on a non-default torch stream
behind a bounded hold and LATE INPUTS (tests/test_side_streams.py has the technique and its reasons: the views' contents are a decoy
until the copies queued behind the hold have run), with no host wait between the three calls.  Right behind the last call's return the
inputs' event must still be pending; after ONE synchronisation every destination must hold, byte for byte and sentinels included,
what the CPU builds of the three libraries give for the same views and the same calls."""
import numpy as np
import pytest

from bam_readcount_amd import capi
from route import Route
import test_dense as td
import test_side_streams as ss
import test_vet as tv

PAD = ss.PAD
T = tv.T_(min_depth=4, min_var_count=2, freq_num=1, freq_den=8)


def chain(sc, cap):
    """(sizes(route), enqueue(route, buf, stream)) of select -> vet -> panel over `cap` elements"""
    sel = ss.select_job(sc)
    ds = cap + PAD
    L = ss.L

    def sizes(route):
        s = dict(sel.sizes(route), **ss.plane_sizes(ds, "p."))
        s.update({"p.status": 4, "v.fail": 4 * L * 4 * ds, "v.keep": 4 * ds, "v.vals": 4 * L * 4 * capi.VET_NVAL * ds, "v.status": 4,
                  "v.ws": route.vet.workspace(sc.v, cap)})
        return s

    def enqueue(route, buf, stream):
        rc = sel.enqueue(route, buf, stream)
        par, keepalive = capi.vet_params(None, capi.VET_ALL_TESTS, **T)
        at = lambda k: route.ptr(buf[k])
        rc = rc or route.vet.sites_raw(sc.v, sc.d, par, at("idx"), at("why"), cap, ds, fail=at("v.fail"), keep=at("v.keep"), vals=at("v.vals"),
                                       status=at("v.status"), workspace=at("v.ws"), stream=stream)
        del keepalive
        return rc or route.panel.gather_raw(sc.v, at("idx"), cap, ds, status=at("p.status"), stream=stream, **{k: at("p." + k) for k in td.KINDS})
    return sizes, enqueue


@pytest.mark.gpu
def test_select_vet_panel_back_to_back_on_a_held_stream():
    sim, hip = Route("sim", ss.LIBS), Route("hip", ss.LIBS)
    torch = hip.torch
    # the CPU route: the same views (the scene is seeded), the same calls
    sc = ss.Scene(sim, 21)
    cap = ss.select_job(sc).cap
    sizes, enqueue = chain(sc, cap)
    want_sizes = sizes(sim)
    buf = {k: sim.sentinel_bytes(max(n, 8)) for k, n in want_sizes.items()}
    assert enqueue(sim, buf, None) == 0
    want = {k: sim.host(b)[:want_sizes[k]].copy() for k, b in buf.items() if not k.endswith("ws")}
    keep = want["v.keep"].view(np.uint32)[:cap]
    assert cap >= 3 and (keep != 0).any() and (keep == 0).any() and sc.v.n_xagg > 0
    # the GPU route: once on the default stream (code objects loaded), then held
    g = ss.Scene(hip, 21)
    gsizes, genqueue = chain(g, cap)
    gs = gsizes(hip)
    assert {k: n for k, n in gs.items() if not k.endswith("ws")} == {k: n for k, n in want_sizes.items() if not k.endswith("ws")}
    rc, got, _ = ss.run_plain(hip, ss.Job("select -> vet -> panel", "vet", gsizes, genqueue, None))
    assert rc == 0, hip.vet.lib.brc_vet_last_error(hip.vet.h)
    ss.compare(got, want, "default stream")
    torch.cuda.synchronize()
    hold = ss.Hold(torch, 0.001)
    streams = ss.streams_beside_the_default(torch, hold, want=1)
    assert streams, "INCONCLUSIVE: no stream runs beside the default stream on this machine"
    s = streams[0]
    g.to_decoy()
    bufs = {k: torch.zeros(max(n, 8), dtype=torch.uint8, device="cuda") for k, n in gs.items()}
    outs = {k: torch.zeros_like(b) for k, b in bufs.items()}
    e = torch.cuda.Event()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        hold.queue()
        g.restore()
        for b in bufs.values():
            b.fill_(ss.SENT8)
        e.record(s)
        rc = genqueue(hip, bufs, s.cuda_stream)
        for k in bufs:
            outs[k].copy_(bufs[k], non_blocking=True)
    pending = not e.query()
    s.synchronize()                                         # the one wait
    assert rc == 0, hip.vet.lib.brc_vet_last_error(hip.vet.h)
    assert pending, "INCONCLUSIVE: when the calls returned, the inputs' event had fired: a call waited, or the hold of %.1f ms was too short" % (1e3 * hold.seconds)
    ss.compare({k: b.cpu().numpy()[:gs[k]] for k, b in outs.items()}, want, "held stream")
    g.to_real()
