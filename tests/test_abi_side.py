"""The lifecycle every side library shares (brc_side_hip.h for the gfx950 builds, tests/sim_side.h for the CPU builds), library by
library over the table of tests/abi_side.py; what is a library's own is in tests/test_abi_<library>.py."""
import ctypes as C

import pytest

import abi_side as side


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
