"""The join of computed regions is a library of its own: it exports exactly what its header declares and the binding lists, its source,
destination and size structs have the header's layout, its constants are the header's, it carries a kernel object of its own, leaves
the engine's kernel object and those of the dense planes, the indel table, the site selection, the two candidate filters and the indel
normalisation what they were, and the product library neither links nor loads it."""
import ctypes as C
import json
import os
import re

import abi_side as side
from abi_side import define

ROW = side.SIDE["join"]


def test_join_exports_equal_the_header_and_the_binding():
    side.check_exports(ROW)


def test_join_structs_and_constants_are_the_headers(tmp_path):
    from bam_readcount_amd import capi
    h = side._header("brc_join.h")
    for struct, T, size in (("brc_join_source", capi.JoinSource, 16), ("brc_join_dest", capi.JoinDest, 88), ("brc_join_sizes", capi.JoinSizes, 136)):
        side.check_struct(tmp_path, "brc_join.h", struct, T, types=T is not capi.JoinSource)          # (the source's pointers are typed)
        assert C.sizeof(T) == size, struct
    assert [n for n, _ in capi.JoinDest._fields_] == list(capi.JOIN_DESTS)
    for n, ct in capi.JoinSizes._fields_:
        assert ct is {"n_lib": C.c_int32, "has_ref": C.c_int32, "ref_lo": C.c_int64, "ref_hi": C.c_int64, "ref_len": C.c_int64}.get(n, C.c_uint64), n
    assert define(h, "BRC_JOIN_MAX_SOURCES") == capi.JOIN_MAX_SOURCES == 16
    assert define(h, "BRC_JOIN_MAX_LIB") == capi.JOIN_MAX_LIB == capi.SELECT_MAX_LIB == 254
    assert define(h, "BRC_JOIN_REF_DIFFERS") == capi.JOIN_REF_DIFFERS == 1
    # the record sizes and the empty position the header names are the engine's
    core = open(os.path.join(side.CSRC, "brc_core.h")).read()
    assert "enum { NB_NONE = 7 };" in core and "dead ? (1u | ((uint32_t)NB_NONE << 8))" in core
    mine = open(os.path.join(side.CSRC, "brc_join_core.h")).read()
    assert "EMPTY_SLOT = 1u | (7u << 8)" in mine and "sizeof(Rec) == 64 && sizeof(Slot) == 72" in mine
    assert define(side._header("brc_ivet.h"), "BRC_IVET_MAX_LIB") == capi.JOIN_MAX_LIB


def test_join_uses_the_shared_scan_and_no_memset_of_planes():
    """the planes are written in one pass: the only memsets of the entry point are the status word's and the counts'"""
    hip = open(os.path.join(side.CSRC, "brc_join.hip")).read()
    assert '#include "brc_side_scan.h"' in hip and "__shared__" not in hip
    assert re.findall(r"hipMemsetAsync\((\w+),", hip) == ["status", "counts"]
    assert "hipMalloc" not in hip and "Synchronize" not in hip and "hipMemcpy" not in hip


def test_join_library_has_a_kernel_object_of_its_own():
    side.check_kernel_object(ROW)


def test_engine_and_sibling_kernel_objects_are_unchanged():
    """the engine's stamp is the committed one, and so are those of the dense planes, the indel table, the site selection, the candidate
    filter, the indel candidate filter and the indel normalisation: none of their sources, nor a header they are built from, was touched"""
    side.check_engine_stamps()
    from bam_readcount_amd import capi
    prof = lambda name: json.load(open(os.path.join(side.ROOT, "profiles", name)))          # (the stamps the earlier commits' measurements recorded)
    assert capi.kernel_object_hash(capi.DENSE_LIB) == prof("panel_bench.json")["dense_kernel_object_sha256_16"] == "0728c62aa99b7ee1"
    assert capi.kernel_object_hash(capi.INDELS_LIB) == prof("inorm_bench.json")["indels_kernel_object_sha256_16"] == "fee860b3aa70b55c"
    assert capi.kernel_object_hash(capi.IVET_LIB) == prof("ivet_bench.json")["ivet_kernel_object_sha256_16"] == "bcc67358ff5bed76"
    assert capi.kernel_object_hash(capi.INORM_LIB) == prof("inorm_bench.json")["inorm_kernel_object_sha256_16"] == "303df97f40a75dc6"
    assert capi.kernel_object_hash(capi.SELECT_LIB) == "878f5677d7083f27"
    assert capi.kernel_object_hash(capi.VET_LIB) == "8f54c7ace8dd5fad"


def test_product_library_neither_links_nor_loads_the_join_library():
    side.check_neither_links_nor_loads(ROW)


def test_the_join_sources_use_no_inline_assembly_and_the_siblings_flags():
    side.check_sources_and_flags(ROW)
    core = open(os.path.join(side.CSRC, "brc_join_core.h")).read()
    assert not re.search(r'#\s*include\s+"brc_\w+_core\.h"', core)          # (it includes no sibling's core: the views are plain data)


def test_package_and_join_import_without_torch():
    side.check_import_without_torch(ROW)


def test_join_library_refuses_to_exist_without_a_device_or_a_build():
    side.check_refuses_to_exist(ROW)
