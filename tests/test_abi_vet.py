"""The candidate filter is a library of its own: it exports exactly what its header declares and the binding lists, its parameter struct
has the header's layout, it carries a kernel object of its own, leaves the engine's kernel object what it was, and the product library
neither links nor loads it."""
import ctypes as C

import abi_side as side
from abi_side import define

ROW = side.SIDE["vet"]


def test_vet_exports_equal_the_header_and_the_binding():
    side.check_exports(ROW)


def test_vet_params_layout_and_constants_are_the_headers(tmp_path):
    from bam_readcount_amd import capi
    h = side._header("brc_vet.h")
    P = capi.VetParams
    side.check_struct(tmp_path, "brc_vet.h", "brc_vet_params", P)          # (names, types, and what a C compiler makes of the header)
    assert [n for n, _ in P._fields_] == ["lib_on", "tests"] + list(capi.VET_UINTS) + list(capi.VET_FLOATS)
    assert C.sizeof(P) == 104 and (P.lib_on.offset, P.tests.offset, P.min_depth.offset, P.min_var_readpos.offset, P.max_rl_diff.offset) == (0, 8, 12, 44, 96)
    assert (define(h, "BRC_VET_MAX_LIB"), define(h, "BRC_VET_NVAL")) == (capi.VET_MAX_LIB, capi.VET_NVAL) == (254, 20)
    assert [define(h, "BRC_VET_" + n) for n in capi.VET_TESTS] == [capi.VET_BIT[n] for n in capi.VET_TESTS] == [1 << i for i in range(18)]
    assert define(h, "BRC_VET_ALL_TESTS") == capi.VET_ALL_TESTS == (1 << 18) - 1
    assert (define(h, "BRC_VET_NOT_ASKED"), define(h, "BRC_VET_NO_SITE")) == (capi.VET_NOT_ASKED, capi.VET_NO_SITE) == (1 << 30, 1 << 31)
    panel = side._header("brc_panel.h")
    twins = (define(panel, "BRC_PANEL_OUT_OF_RANGE"), define(panel, "BRC_PANEL_NOT_ASCENDING"))
    assert (define(h, "BRC_VET_OUT_OF_RANGE"), define(h, "BRC_VET_NOT_ASCENDING")) == (capi.VET_OUT_OF_RANGE, capi.VET_NOT_ASCENDING) == twins
    cols = ["CV", "CR", "D", "FREQ", "STRAND", "MMQS_DIFF", "MAPQ_DIFF", "RL_DIFF", "VAR", "REF"]
    assert [define(h, "BRC_VET_V_" + n) for n in cols] == [0, 1, 2, 3, 4, 5, 6, 7, 8, 14] and len(capi.VET_V_NAMES) == capi.VET_NVAL
    assert [n.upper() for n in capi.VET_V_NAMES[:8]] == cols[:8]


def test_vet_library_has_a_kernel_object_of_its_own():
    side.check_kernel_object(ROW)


def test_engine_kernel_object_still_equals_the_committed_stamps():
    side.check_engine_stamps()


def test_product_library_neither_links_nor_loads_the_vet_library():
    side.check_neither_links_nor_loads(ROW)


def test_the_vet_sources_use_no_inline_assembly_and_the_siblings_flags():
    side.check_sources_and_flags(ROW)


def test_package_and_vet_import_without_torch():
    side.check_import_without_torch(ROW)


def test_vet_library_refuses_to_exist_without_a_device_or_a_build():
    side.check_refuses_to_exist(ROW)
