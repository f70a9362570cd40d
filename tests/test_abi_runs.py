"""The depth-class interval library is a library of its own: it exports exactly what its header declares and the binding lists, its
parameter struct has the header's layout, it carries a kernel object of its own, leaves the engine's kernel object what it was, and the
product library neither links nor loads it."""
import ctypes as C

import abi_side as side
from abi_side import define

ROW = side.SIDE["runs"]


def test_runs_exports_equal_the_header_and_the_binding():
    side.check_exports(ROW)


def test_runs_params_layout_and_constants_are_the_headers(tmp_path):
    from bam_readcount_amd import capi
    h = side._header("brc_runs.h")
    P = capi.RunsParams
    side.check_struct(tmp_path, "brc_runs.h", "brc_runs_params", P, array_len=capi.RUNS_MAX_CUT)
    assert C.sizeof(P) == 88 and (P.role.offset, P.combine.offset, P.n_cut.offset, P.cut.offset, P.keep.offset, P.flags.offset) == (0, 8, 12, 16, 76, 80)
    assert (define(h, "BRC_RUNS_MAX_LIB"), define(h, "BRC_RUNS_MAX_CUT")) == (capi.RUNS_MAX_LIB, capi.RUNS_MAX_CUT) == (254, 15)
    assert (define(h, "BRC_RUNS_MIN"), define(h, "BRC_RUNS_MAX"), define(h, "BRC_RUNS_SUM")) == (capi.RUNS_MIN, capi.RUNS_MAX, capi.RUNS_SUM) == (0, 1, 2)
    assert define(h, "BRC_RUNS_REF_N") == capi.RUNS_REF_N == 1
    from bam_readcount_amd import tensors
    assert tensors.RUNS_COMBINE == {"min": 0, "max": 1, "sum": 2}


def test_runs_library_has_a_kernel_object_of_its_own():
    side.check_kernel_object(ROW)


def test_engine_kernel_object_still_equals_the_committed_stamps():
    side.check_engine_stamps()


def test_product_library_neither_links_nor_loads_the_runs_library():
    side.check_neither_links_nor_loads(ROW)


def test_the_runs_sources_use_no_inline_assembly_and_the_siblings_flags():
    side.check_sources_and_flags(ROW)


def test_package_and_runs_import_without_torch():
    side.check_import_without_torch(ROW)


def test_runs_library_refuses_to_exist_without_a_device_or_a_build():
    side.check_refuses_to_exist(ROW)
