"""The indel normalisation is a library of its own: it exports exactly what its header declares and the binding lists, its parameter
and source structs have the header's layout, its flag and status bits are the header's, it carries a kernel object of its own, leaves
the engine's kernel object and those of the indel table, the candidate filter and the indel candidate filter what they were, and the
product library neither links nor loads it."""
import ctypes as C
import os

import abi_side as side
from abi_side import define

ROW = side.SIDE["inorm"]


def test_inorm_exports_equal_the_header_and_the_binding():
    side.check_exports(ROW)


def test_inorm_structs_and_constants_are_the_headers(tmp_path):
    from bam_readcount_amd import capi
    h = side._header("brc_inorm.h")
    P, S = capi.INormParams, capi.INormSource
    side.check_struct(tmp_path, "brc_inorm.h", "brc_inorm_params", P, array_len=3)
    assert [n for n, _ in P._fields_] == ["max_shift", "reserved"] and [C.sizeof(P), P.max_shift.offset, P.reserved.offset] == [16, 0, 4]
    side.check_struct(tmp_path, "brc_inorm.h", "brc_inorm_source", S)
    assert [n for n, _ in S._fields_] == ["m", "stride", "pos", "lib", "len", "rep_read", "rep_qpos", "istat", "fstat", "allele_off", "alleles", "alleles_len"]
    for n, ct in S._fields_:
        assert ct is (C.c_int64 if n in ("m", "stride", "alleles_len") else C.c_void_p), n
    assert C.sizeof(S) == 96
    assert define(h, "BRC_INORM_MAX_SHIFT") == capi.INORM_MAX_SHIFT == 1 << 20
    flags = ("NOT_JUDGED", "LIMIT", "EDGE")
    assert [define(h, "BRC_INORM_" + n) for n in flags] == [getattr(capi, "INORM_" + n) for n in flags] == [1, 2, 4]
    status = ("TABLE_BAD", "ANY_LIMIT", "ANY_EDGE")
    assert [define(h, "BRC_INORM_" + n) for n in status] == [getattr(capi, "INORM_" + n) for n in status] == [1, 2, 4]
    # the new table is the indel table's: the same destinations, and one more
    assert capi.INORM_DESTS == capi.INDEL_DESTS[:5] + ("members",) + capi.INDEL_DESTS[5:]


def test_inorm_runs_the_dense_librarys_columns_not_a_copy():
    """the thirteen columns of a merged record are brc_dense_core.h's metrics13, the function emit_lane calls"""
    core = open(os.path.join(side.CSRC, "brc_inorm_core.h")).read()
    assert "brcdense::metrics13(" in core and "BRC_M_AVG" not in core
    hip = open(os.path.join(side.CSRC, "brc_inorm.hip")).read()
    assert '#include "brc_side_scan.h"' in hip and "__shared__" not in hip and "__shared__" not in core


def test_inorm_library_has_a_kernel_object_of_its_own():
    side.check_kernel_object(ROW)


def test_engine_and_sibling_kernel_objects_are_unchanged():
    """the engine's stamp is the committed one, and so are those of the indel table, the candidate filter and the indel candidate filter:
    none of their sources, nor a header they are built from, was touched"""
    side.check_engine_stamps()
    from bam_readcount_amd import capi
    import json
    j = json.load(open(os.path.join(side.ROOT, "profiles", "ivet_bench.json")))          # (the stamps the parent commit's measurement recorded)
    assert capi.kernel_object_hash(capi.INDELS_LIB) == j["indels_kernel_object_sha256_16"] == "fee860b3aa70b55c"
    assert capi.kernel_object_hash(capi.IVET_LIB) == j["ivet_kernel_object_sha256_16"] == "bcc67358ff5bed76"
    assert capi.kernel_object_hash(capi.VET_LIB) == "8f54c7ace8dd5fad"


def test_product_library_neither_links_nor_loads_the_inorm_library():
    side.check_neither_links_nor_loads(ROW)


def test_the_inorm_sources_use_no_inline_assembly_and_the_siblings_flags():
    side.check_sources_and_flags(ROW)
    src = open(os.path.join(side.CSRC, "brc_side_scan.h")).read()
    assert "asm" not in src and "brc_core.h" not in src and "brc_host.h" not in src


def test_package_and_inorm_import_without_torch():
    side.check_import_without_torch(ROW)


def test_inorm_library_refuses_to_exist_without_a_device_or_a_build():
    side.check_refuses_to_exist(ROW)
