"""The indel candidate filter is a library of its own: it exports exactly what its header declares and the binding lists, its parameter
and table structs have the header's layout, its shared test bits are brc_vet.h's, it carries a kernel object of its own, leaves the
engine's kernel object what it was, and the product library neither links nor loads it.  Its row of the table declares that it is built
from the candidate filter's header and core (uses)."""
import ctypes as C
import os
import re

import abi_side as side
from abi_side import define

ROW = side.SIDE["ivet"]


def test_ivet_exports_equal_the_header_and_the_binding():
    side.check_exports(ROW)


def test_ivet_structs_and_constants_are_the_headers(tmp_path):
    from bam_readcount_amd import capi
    h = side._header("brc_ivet.h")
    P = capi.IVetParams
    side.check_struct(tmp_path, "brc_ivet.h", "brc_ivet_params", P)
    assert [n for n, _ in P._fields_] == ["role", "tests", "kinds"] + list(capi.IVET_UINTS) + list(capi.IVET_FLOATS)
    assert C.sizeof(P) == 120 and (P.role.offset, P.tests.offset, P.kinds.offset, P.min_depth.offset, P.ctl_min_depth.offset, P.min_var_readpos.offset,
                                   P.max_rl_diff.offset) == (0, 8, 12, 16, 48, 64, 112)
    # the thresholds are brc_vet_params' without min_var_bq, then the control test
    assert list(capi.IVET_UINTS[:8]) == list(capi.VET_UINTS) and list(capi.IVET_FLOATS) == [k for k in capi.VET_FLOATS if k != "min_var_bq"]
    T = capi.IVetTable
    side.check_struct(tmp_path, "brc_ivet.h", "brc_ivet_table", T)
    assert [n for n, _ in T._fields_] == ["m", "stride", "pos", "lib", "len", "istat", "fstat", "allele_off", "alleles", "alleles_len"]
    assert C.sizeof(T) == 80
    assert (define(h, "BRC_IVET_MAX_LIB"), define(h, "BRC_IVET_NVAL")) == (capi.IVET_MAX_LIB, capi.IVET_NVAL) == (254, 20)
    # the new bits, and the shared ones: brc_vet.h's values
    assert (define(h, "BRC_IVET_CTL_DEPTH"), define(h, "BRC_IVET_CTL_ALLELE")) == (capi.IVET_BIT["CTL_DEPTH"], capi.IVET_BIT["CTL_ALLELE"]) == (1 << 18, 1 << 19)
    vet = side._header("brc_vet.h")
    for n in capi.IVET_TESTS[:-2]:
        assert capi.IVET_BIT[n] == capi.VET_BIT[n] == define(vet, "BRC_VET_" + n), n
    assert "VAR_BQ" not in capi.IVET_BIT and len(capi.IVET_TESTS) == 19
    assert define(h, "BRC_IVET_ALL_TESTS") == capi.IVET_ALL_TESTS == ((define(vet, "BRC_VET_ALL_TESTS") & ~define(vet, "BRC_VET_VAR_BQ")) | 3 << 18)
    assert (define(h, "BRC_IVET_NOT_ASKED"), define(h, "BRC_IVET_NO_SITE")) == (capi.IVET_NOT_ASKED, capi.IVET_NO_SITE) == \
        (define(vet, "BRC_VET_NOT_ASKED"), define(vet, "BRC_VET_NO_SITE"))
    assert define(vet, "BRC_VET_NVAL") == define(h, "BRC_IVET_NVAL")
    status = ("LIST_OUT_OF_RANGE", "LIST_NOT_ASCENDING", "TABLE_OUT_OF_RANGE", "TABLE_NOT_ASCENDING")
    assert [define(h, "BRC_IVET_" + n) for n in status] == [getattr(capi, "IVET_" + n) for n in status] == [1, 2, 4, 8]
    assert (capi.IVET_LIST_OUT_OF_RANGE, capi.IVET_LIST_NOT_ASCENDING) == (capi.VET_OUT_OF_RANGE, capi.VET_NOT_ASCENDING)
    # the header includes brc_vet.h: roles and reason bits are brc_select.h's
    assert re.search(r'#include\s+"brc_vet.h"', h)


def test_ivet_runs_the_snv_filters_tests_not_a_copy():
    """the fp32 tests and the bucket lookup are brc_vet_core.h's functions"""
    core = open(os.path.join(side.CSRC, "brc_ivet_core.h")).read()
    assert '#include "brc_vet_core.h"' in core
    for fn in ("brcvet::judge(", "brcvet::bucket_side(", "brcvet::ref_bucket(", "brcvet::side_of(", "brcvet::check_job("):
        assert fn in core, fn
    assert "metrics13" not in core and "BRC_VET_VAR_READPOS" not in core


def test_ivet_library_has_a_kernel_object_of_its_own():
    side.check_kernel_object(ROW)


def test_engine_kernel_object_still_equals_the_committed_stamps():
    side.check_engine_stamps()


def test_product_library_neither_links_nor_loads_the_ivet_library():
    side.check_neither_links_nor_loads(ROW)


def test_the_ivet_sources_use_no_inline_assembly_and_the_siblings_flags():
    side.check_sources_and_flags(ROW)


def test_package_and_ivet_import_without_torch():
    side.check_import_without_torch(ROW)


def test_ivet_library_refuses_to_exist_without_a_device_or_a_build():
    side.check_refuses_to_exist(ROW)
