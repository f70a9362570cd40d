"""The candidate filter is a library of its own: it exports exactly what its header declares and the binding lists, its parameter struct
has the header's layout, it carries a kernel object of its own, leaves the engine's kernel object what it was, and the product library
neither links nor loads it.  Its row of the side libraries' table is defined here and handed to the checks of tests/abi_side.py, which
take any row; "the others" of this row are the engine, the inflater, the deflater and every row of that table."""
import ctypes as C
import os
import re
import subprocess

import pytest

import abi_side as side
import test_abi_side

ROW = dict(name="vet", cls="Vet", tensors="vet", kernels=("k_vet_link", "k_vet_sites"), strict=True,
           null_call=lambda o: o.sites_raw(None, None, None, None, None, 1, 1))


def test_vet_exports_equal_the_header_and_the_binding():
    side.check_exports(ROW)


def test_vet_params_layout_and_constants_are_the_headers(tmp_path):
    from bam_readcount_amd import capi
    h = side._header("brc_vet.h")
    body = re.search(r"typedef struct brc_vet_params \{(.*?)\} brc_vet_params;", h, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, names = re.match(r"(const uint8_t\*|uint32_t|float)\s+(.*)", decl, flags=re.S).groups()
        fields += [(n.strip(), typ) for n in names.split(",")]
    P = capi.VetParams
    assert [n for n, _ in fields] == [n for n, _ in P._fields_] == ["lib_on", "tests"] + list(capi.VET_UINTS) + list(capi.VET_FLOATS)
    ctype = {"const uint8_t*": C.c_void_p, "uint32_t": C.c_uint32, "float": C.c_float}
    for (n, typ), (_, ct) in zip(fields, P._fields_):
        assert ct is ctype[typ], n
    assert C.sizeof(P) == 104 and (P.lib_on.offset, P.tests.offset, P.min_depth.offset, P.min_var_readpos.offset, P.max_rl_diff.offset) == (0, 8, 12, 44, 96)
    # ... and what a C compiler makes of the header
    src = '#include <stddef.h>\n#include <stdio.h>\n#include "brc_vet.h"\nint main(void) { printf("%zu", sizeof(brc_vet_params));\n'
    src += "".join('printf(" %%zu", offsetof(brc_vet_params, %s));\n' % n for n, _ in P._fields_) + "return 0; }\n"
    exe = str(tmp_path / "vet_layout_check")
    subprocess.run(["gcc", "-x", "c", "-std=c99", "-I", os.path.join(side.ROOT, "include"), "-", "-o", exe], input=src.encode(), check=True)
    got = [int(x) for x in subprocess.run([exe], stdout=subprocess.PIPE, check=True).stdout.split()]
    assert got == [C.sizeof(P)] + [getattr(P, n).offset for n, _ in P._fields_]

    def define(name):
        return int(re.search(r"#define\s+%s\s+(\d+)u?\b" % name, h).group(1))
    assert (define("BRC_VET_MAX_LIB"), define("BRC_VET_NVAL")) == (capi.VET_MAX_LIB, capi.VET_NVAL) == (254, 20)
    assert [define("BRC_VET_" + n) for n in capi.VET_TESTS] == [capi.VET_BIT[n] for n in capi.VET_TESTS] == [1 << i for i in range(18)]
    assert define("BRC_VET_ALL_TESTS") == capi.VET_ALL_TESTS == (1 << 18) - 1
    assert (define("BRC_VET_NOT_ASKED"), define("BRC_VET_NO_SITE")) == (capi.VET_NOT_ASKED, capi.VET_NO_SITE) == (1 << 30, 1 << 31)
    panel = side._header("brc_panel.h")
    twins = tuple(int(re.search(r"#define\s+%s\s+(\d+)u" % n, panel).group(1)) for n in ("BRC_PANEL_OUT_OF_RANGE", "BRC_PANEL_NOT_ASCENDING"))
    assert (define("BRC_VET_OUT_OF_RANGE"), define("BRC_VET_NOT_ASCENDING")) == (capi.VET_OUT_OF_RANGE, capi.VET_NOT_ASCENDING) == twins
    cols = ["CV", "CR", "D", "FREQ", "STRAND", "MMQS_DIFF", "MAPQ_DIFF", "RL_DIFF", "VAR", "REF"]
    assert [define("BRC_VET_V_" + n) for n in cols] == [0, 1, 2, 3, 4, 5, 6, 7, 8, 14] and len(capi.VET_V_NAMES) == capi.VET_NVAL
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


@pytest.mark.parametrize("build", ["sim", pytest.param("hip", marks=pytest.mark.gpu)])
def test_vet_handle_lifecycle(build):
    test_abi_side.test_handle_lifecycle(ROW, build)
