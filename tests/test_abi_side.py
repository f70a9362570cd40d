"""The lifecycle every side library shares (brc_side_hip.h for the gfx950 builds, tests/sim_side.h for the CPU builds), library by
library over the table of tests/abi_side.py; what is a library's own is in tests/test_abi_<library>.py."""
import ctypes as C
import os
import re

import pytest

import abi_side as side


def test_the_table_is_every_side_library():
    """The table's rows, the SIDE list of the build rule, the CPU builds under tests/ and the binding's LIB / EXPORTS pairs name the
    same ten libraries: one that is built, simulated or bound without a row would escape every sibling check."""
    from bam_readcount_amd import capi
    mk = open(os.path.join(side.CSRC, "Makefile")).read()
    words = lambda var: set(re.search(r"^%s = (.*)$" % var, mk, flags=re.M).group(1).split())
    codecs = words("CODEC")                                    # (the inflater and the deflater: tests/test_abi_{inflate,deflate}.py)
    tests = os.path.join(side.ROOT, "tests")
    sims = {d[4:] for d in os.listdir(tests) if d.startswith("sim_") and os.path.exists(os.path.join(tests, d, "brc_%s_sim.cpp" % d[4:]))}
    bound = {n[:-4].lower() for n in dir(capi) if n.endswith("_LIB") and hasattr(capi, n[:-4] + "_EXPORTS")}
    rows = [r["name"] for r in side.ROWS]
    assert len(rows) == 10 and set(rows) == set(side.SIDE) == words("SIDE") == sims - codecs == bound - codecs
    assert codecs == {"inflate", "deflate"} and codecs <= sims and codecs <= bound
    for r in side.ROWS:
        assert set(r.get("uses", ())) <= set(rows) - {r["name"]}, r["name"]


@pytest.mark.parametrize("row", side.ROWS, ids=list(side.SIDE))
@pytest.mark.parametrize("build", ["sim", pytest.param("hip", marks=pytest.mark.gpu)])
def test_handle_lifecycle(row, build):
    """The shared lifecycle (brc_side_hip.h / sim_side.h) behind every library's five common calls; no view, no data."""
    from bam_readcount_amd import capi
    name = row["name"]
    o = getattr(capi, row["cls"])(side.sim_lib(row) if build == "sim" else None)
    L = o.lib
    call = lambda suffix: getattr(L, "brc_%s_%s" % (name, suffix))
    zeros = dict(kernel_s=0.0, bytes_read=0, bytes_written=0)
    assert o.kind() == ("sim" if build == "sim" else "hip-gfx950")
    assert o.last_timing() == zeros and call("last_error")(o.h) == b""
    assert row["null_call"](o) == capi.E_ARG
    assert call("last_error")(o.h) != b""
    assert o.last_timing() == zeros
    # NULL handles are harmless
    call("destroy")(None)
    assert call("last_error")(None) == b""
    k = C.c_double(7.0); r = C.c_uint64(7); w = C.c_uint64(7)
    call("last_timing")(None, C.byref(k), C.byref(r), C.byref(w))
    assert (k.value, r.value, w.value) == (7.0, 7, 7)
    call("last_timing")(o.h, None, None, None)
    # devices that do not exist
    h = C.c_void_p()
    assert call("create")(-1, C.byref(h)) == (capi.E_ARG if build == "sim" else capi.E_NODEVICE) and not h
    assert call("create")(0, None) == capi.E_ARG
    if build == "hip":
        import torch
        h = C.c_void_p()
        assert call("create")(torch.cuda.device_count(), C.byref(h)) == capi.E_NODEVICE and not h
    # create and destroy over and over: the shared destroy gives back everything the shared create took
    for _ in range(20):
        h = C.c_void_p()
        assert call("create")(0, C.byref(h)) == 0 and h
        call("destroy")(h)
    o.close()
    assert o.h is None
