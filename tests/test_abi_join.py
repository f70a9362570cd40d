"""The join of computed regions is a library of its own: it exports exactly what its header declares and the binding lists, its source,
destination and size structs have the header's layout, its constants are the header's, it carries a kernel object of its own, leaves
the engine's kernel object and those of the dense planes, the indel table, the site selection, the two candidate filters and the indel
normalisation what they were, and the product library neither links nor loads it.  Its row of the side libraries' table is defined
here and handed to the checks of tests/abi_side.py, which take any row; "the others" of this row are the engine, the inflater, the
deflater and every row of that table."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest

import abi_side as side
import test_abi_side

ROW = dict(name="join", cls="Join", tensors="join",
           kernels=("k_join_planes", "k_join_xagg", "k_join_slots", "k_join_reads", "k_join_ref", "k_side_scan_reduce", "k_side_scan_parts", "k_side_scan_apply"),
           strict=True, null_call=lambda o: o.views_raw(None, 0, 1, 1, K=1))
LATER = ("RUNS", "VET", "IVET", "INORM")          # (the libraries that came after abi_side's table)


def test_join_exports_equal_the_header_and_the_binding():
    side.check_exports(ROW)
    from bam_readcount_amd import capi
    for other in LATER:
        assert not set(capi.JOIN_EXPORTS) & set(getattr(capi, other + "_EXPORTS"))


def _c_layout(tmp_path, struct, names):
    src = '#include <stddef.h>\n#include <stdio.h>\n#include "brc_join.h"\nint main(void) { printf("%%zu", sizeof(%s));\n' % struct
    src += "".join('printf(" %%zu", offsetof(%s, %s));\n' % (struct, n) for n in names) + "return 0; }\n"
    exe = str(tmp_path / (struct + "_layout_check"))
    subprocess.run(["gcc", "-x", "c", "-std=c99", "-I", os.path.join(side.ROOT, "include"), "-", "-o", exe], input=src.encode(), check=True)
    return [int(x) for x in subprocess.run([exe], stdout=subprocess.PIPE, check=True).stdout.split()]


def _members(h, struct):
    """the member names of a struct of the header, in order"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), h, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [n.strip().lstrip("*").split("[")[0] for n in re.sub(r"^(const\s+)?\w+\s*\*?", "", decl, count=1).split(",")]
    return names


def test_join_structs_and_constants_are_the_headers(tmp_path):
    from bam_readcount_amd import capi
    h = side._header("brc_join.h")
    for struct, T, size in (("brc_join_source", capi.JoinSource, 16), ("brc_join_dest", capi.JoinDest, 88), ("brc_join_sizes", capi.JoinSizes, 136)):
        names = [n for n, _ in T._fields_]
        assert _members(h, struct) == names, struct
        assert _c_layout(tmp_path, struct, names) == [C.sizeof(T)] + [getattr(T, n).offset for n in names] and C.sizeof(T) == size, struct
    assert [n for n, _ in capi.JoinDest._fields_] == list(capi.JOIN_DESTS)
    for n, ct in capi.JoinSizes._fields_:
        assert ct is {"n_lib": C.c_int32, "has_ref": C.c_int32, "ref_lo": C.c_int64, "ref_hi": C.c_int64, "ref_len": C.c_int64}.get(n, C.c_uint64), n

    def define(name):
        return int(re.search(r"#define\s+%s\s+(\d+)u?\b" % name, h).group(1))
    assert define("BRC_JOIN_MAX_SOURCES") == capi.JOIN_MAX_SOURCES == 16
    assert define("BRC_JOIN_MAX_LIB") == capi.JOIN_MAX_LIB == capi.SELECT_MAX_LIB == 254
    assert define("BRC_JOIN_REF_DIFFERS") == capi.JOIN_REF_DIFFERS == 1
    # the record sizes and the empty position the header names are the engine's
    core = open(os.path.join(side.CSRC, "brc_core.h")).read()
    assert "enum { NB_NONE = 7 };" in core and "dead ? (1u | ((uint32_t)NB_NONE << 8))" in core
    mine = open(os.path.join(side.CSRC, "brc_join_core.h")).read()
    assert "EMPTY_SLOT = 1u | (7u << 8)" in mine and "sizeof(Rec) == 64 && sizeof(Slot) == 72" in mine
    ivet = side._header("brc_ivet.h")
    assert int(re.search(r"#define\s+BRC_IVET_MAX_LIB\s+(\d+)", ivet).group(1)) == capi.JOIN_MAX_LIB


def test_join_uses_the_shared_scan_and_no_memset_of_planes():
    """the planes are written in one pass: the only memsets of the entry point are the status word's and the counts'"""
    hip = open(os.path.join(side.CSRC, "brc_join.hip")).read()
    assert '#include "brc_side_scan.h"' in hip and "__shared__" not in hip
    assert re.findall(r"hipMemsetAsync\((\w+),", hip) == ["status", "counts"]
    assert "hipMalloc" not in hip and "Synchronize" not in hip and "hipMemcpy" not in hip


def test_join_library_has_a_kernel_object_of_its_own():
    side.check_kernel_object(ROW)
    from bam_readcount_amd import capi
    mine = capi.kernel_object_hash(capi.JOIN_LIB)
    assert mine not in [capi.kernel_object_hash(getattr(capi, n + "_LIB")) for n in LATER]


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
    from bam_readcount_amd import capi
    for n in LATER:
        assert b"brc_join" not in open(getattr(capi, n + "_LIB"), "rb").read(), n


def test_the_join_sources_use_no_inline_assembly_and_the_siblings_flags():
    side.check_sources_and_flags(ROW)
    core = open(os.path.join(side.CSRC, "brc_join_core.h")).read()
    assert not re.search(r'#\s*include\s+"brc_\w+_core\.h"', core)          # (it includes no sibling's core: the views are plain data)


def test_package_and_join_import_without_torch():
    side.check_import_without_torch(ROW)


def test_join_library_refuses_to_exist_without_a_device_or_a_build():
    side.check_refuses_to_exist(ROW)


@pytest.mark.parametrize("build", ["sim", pytest.param("hip", marks=pytest.mark.gpu)])
def test_join_handle_lifecycle(build):
    test_abi_side.test_handle_lifecycle(ROW, build)
