"""The indel candidate filter is a library of its own: it exports exactly what its header declares and the binding lists, its parameter
and table structs have the header's layout, its shared test bits are brc_vet.h's, it carries a kernel object of its own, leaves the
engine's kernel object what it was, and the product library neither links nor loads it.  Its row of the side libraries' table is
defined here and handed to the checks of tests/abi_side.py, which take any row; "the others" of this row are the engine, the inflater,
the deflater and every row of that table."""
import ctypes as C
import os
import re
import subprocess

import pytest

import abi_side as side
import test_abi_side

ROW = dict(name="ivet", cls="IVet", tensors="vet_indels", kernels=("k_ivet_link", "k_ivet_records"), strict=True,
           null_call=lambda o: o.records_raw(None, None, None, None, None, None, 1, 1))


def test_ivet_exports_equal_the_header_and_the_binding():
    side.check_exports(ROW)


def _fields(h, struct, types):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), h, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, names = re.match(r"(%s)\s*(.*)" % "|".join(re.escape(t) for t in types), decl, flags=re.S).groups()
        fields += [(n.strip().lstrip("*"), typ if not n.strip().startswith("*") else typ + "*") for n in names.split(",")]
    return fields


def _c_layout(tmp_path, struct, names):
    src = '#include <stddef.h>\n#include <stdio.h>\n#include "brc_ivet.h"\nint main(void) { printf("%%zu", sizeof(%s));\n' % struct
    src += "".join('printf(" %%zu", offsetof(%s, %s));\n' % (struct, n) for n in names) + "return 0; }\n"
    exe = str(tmp_path / (struct + "_layout_check"))
    subprocess.run(["gcc", "-x", "c", "-std=c99", "-I", os.path.join(side.ROOT, "include"), "-", "-o", exe], input=src.encode(), check=True)
    return [int(x) for x in subprocess.run([exe], stdout=subprocess.PIPE, check=True).stdout.split()]


def test_ivet_structs_and_constants_are_the_headers(tmp_path):
    from bam_readcount_amd import capi
    h = side._header("brc_ivet.h")
    fields = _fields(h, "brc_ivet_params", ("const uint8_t*", "uint32_t", "float"))
    P = capi.IVetParams
    assert [n for n, _ in fields] == [n for n, _ in P._fields_] == ["role", "tests", "kinds"] + list(capi.IVET_UINTS) + list(capi.IVET_FLOATS)
    ctype = {"const uint8_t*": C.c_void_p, "uint32_t": C.c_uint32, "float": C.c_float}
    for (n, typ), (_, ct) in zip(fields, P._fields_):
        assert ct is ctype[typ], n
    assert C.sizeof(P) == 120 and (P.role.offset, P.tests.offset, P.kinds.offset, P.min_depth.offset, P.ctl_min_depth.offset, P.min_var_readpos.offset,
                                   P.max_rl_diff.offset) == (0, 8, 12, 16, 48, 64, 112)
    assert _c_layout(tmp_path, "brc_ivet_params", [n for n, _ in P._fields_]) == [C.sizeof(P)] + [getattr(P, n).offset for n, _ in P._fields_]
    # the thresholds are brc_vet_params' without min_var_bq, then the control test
    assert list(capi.IVET_UINTS[:8]) == list(capi.VET_UINTS) and list(capi.IVET_FLOATS) == [k for k in capi.VET_FLOATS if k != "min_var_bq"]
    fields = _fields(h, "brc_ivet_table", ("int64_t", "const int32_t", "const uint32_t*", "const float*", "const uint8_t*"))
    T = capi.IVetTable
    assert [n for n, _ in fields] == [n for n, _ in T._fields_] == ["m", "stride", "pos", "lib", "len", "istat", "fstat", "allele_off", "alleles", "alleles_len"]
    for (n, typ), (_, ct) in zip(fields, T._fields_):
        assert ct is (C.c_void_p if typ.endswith("*") else C.c_int64), n
    assert _c_layout(tmp_path, "brc_ivet_table", [n for n, _ in T._fields_]) == [C.sizeof(T)] + [getattr(T, n).offset for n, _ in T._fields_]
    assert C.sizeof(T) == 80

    def define(name, text=h):
        return int(re.search(r"#define\s+%s\s+(\d+)u?\b" % name, text).group(1))
    assert (define("BRC_IVET_MAX_LIB"), define("BRC_IVET_NVAL")) == (capi.IVET_MAX_LIB, capi.IVET_NVAL) == (254, 20)
    # the new bits, and the shared ones: brc_vet.h's values
    assert (define("BRC_IVET_CTL_DEPTH"), define("BRC_IVET_CTL_ALLELE")) == (capi.IVET_BIT["CTL_DEPTH"], capi.IVET_BIT["CTL_ALLELE"]) == (1 << 18, 1 << 19)
    vet = side._header("brc_vet.h")
    for n in capi.IVET_TESTS[:-2]:
        assert capi.IVET_BIT[n] == capi.VET_BIT[n] == define("BRC_VET_" + n, vet), n
    assert "VAR_BQ" not in capi.IVET_BIT and len(capi.IVET_TESTS) == 19
    assert define("BRC_IVET_ALL_TESTS") == capi.IVET_ALL_TESTS == ((define("BRC_VET_ALL_TESTS", vet) & ~define("BRC_VET_VAR_BQ", vet)) | 3 << 18)
    assert (define("BRC_IVET_NOT_ASKED"), define("BRC_IVET_NO_SITE")) == (capi.IVET_NOT_ASKED, capi.IVET_NO_SITE) == \
        (define("BRC_VET_NOT_ASKED", vet), define("BRC_VET_NO_SITE", vet))
    assert define("BRC_VET_NVAL", vet) == define("BRC_IVET_NVAL")
    status = ("LIST_OUT_OF_RANGE", "LIST_NOT_ASCENDING", "TABLE_OUT_OF_RANGE", "TABLE_NOT_ASCENDING")
    assert [define("BRC_IVET_" + n) for n in status] == [getattr(capi, "IVET_" + n) for n in status] == [1, 2, 4, 8]
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
    from bam_readcount_amd import capi
    assert capi.kernel_object_hash(capi.IVET_LIB) != capi.kernel_object_hash(capi.VET_LIB)


def test_engine_kernel_object_still_equals_the_committed_stamps():
    side.check_engine_stamps()


def test_product_library_neither_links_nor_loads_the_ivet_library():
    side.check_neither_links_nor_loads(ROW)
    from bam_readcount_amd import capi
    blob = open(capi.VET_LIB, "rb").read()
    assert b"brc_ivet" not in blob


def test_the_ivet_sources_use_no_inline_assembly_and_the_siblings_flags():
    side.check_sources_and_flags(ROW)


def test_package_and_ivet_import_without_torch():
    side.check_import_without_torch(ROW)


def test_ivet_library_refuses_to_exist_without_a_device_or_a_build():
    side.check_refuses_to_exist(ROW)


@pytest.mark.parametrize("build", ["sim", pytest.param("hip", marks=pytest.mark.gpu)])
def test_ivet_handle_lifecycle(build):
    test_abi_side.test_handle_lifecycle(ROW, build)
