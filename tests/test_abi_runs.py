"""The depth-class interval library is a library of its own: it exports exactly what its header declares and the binding lists, its
parameter struct has the header's layout, it carries a kernel object of its own, leaves the engine's kernel object what it was, and the
product library neither links nor loads it.  Its row of the side libraries' table is defined here and handed to the checks of
tests/abi_side.py, which take any row; "the others" of this row are the engine, the inflater, the deflater and every row of that table."""
import ctypes as C
import os
import re
import subprocess

import pytest

import abi_side as side
import test_abi_side

ROW = dict(name="runs", cls="Runs", tensors="runs", kernels=("k_runs_class", "k_runs_parts", "k_runs_emit"), strict=True,
           null_call=lambda o: o.find_raw(None, None, None, 0, 1))


def test_runs_exports_equal_the_header_and_the_binding():
    side.check_exports(ROW)


def test_runs_params_layout_and_constants_are_the_headers(tmp_path):
    from bam_readcount_amd import capi
    h = side._header("brc_runs.h")
    body = re.search(r"typedef struct brc_runs_params \{(.*?)\} brc_runs_params;", h, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, name = re.match(r"(const uint8_t\*|uint32_t)\s+(\w+(?:\[\w+\])?)$", decl).groups()
        fields.append((name.split("[")[0], typ, "[" in name))
    assert [n for n, _, _ in fields] == [n for n, _ in capi.RunsParams._fields_]
    ctype = {"const uint8_t*": C.c_void_p, "uint32_t": C.c_uint32}
    for (n, typ, arr), (_, ct) in zip(fields, capi.RunsParams._fields_):
        assert ct is ctype[typ] if not arr else (ct._type_ is ctype[typ] and ct._length_ == capi.RUNS_MAX_CUT), n
    P = capi.RunsParams
    assert C.sizeof(P) == 88 and (P.role.offset, P.combine.offset, P.n_cut.offset, P.cut.offset, P.keep.offset, P.flags.offset) == (0, 8, 12, 16, 76, 80)
    # ... and what a C compiler makes of the header
    src = '#include <stddef.h>\n#include <stdio.h>\n#include "brc_runs.h"\nint main(void) { printf("%zu", sizeof(brc_runs_params));\n'
    src += "".join('printf(" %%zu", offsetof(brc_runs_params, %s));\n' % n for n, _ in P._fields_) + "return 0; }\n"
    exe = str(tmp_path / "runs_layout_check")
    subprocess.run(["gcc", "-x", "c", "-std=c99", "-I", os.path.join(side.ROOT, "include"), "-", "-o", exe], input=src.encode(), check=True)
    got = [int(x) for x in subprocess.run([exe], stdout=subprocess.PIPE, check=True).stdout.split()]
    assert got == [C.sizeof(P)] + [getattr(P, n).offset for n, _ in P._fields_]

    def define(name):
        return int(re.search(r"#define\s+%s\s+(\d+)u?\b" % name, h).group(1))
    assert (define("BRC_RUNS_MAX_LIB"), define("BRC_RUNS_MAX_CUT")) == (capi.RUNS_MAX_LIB, capi.RUNS_MAX_CUT) == (254, 15)
    assert (define("BRC_RUNS_MIN"), define("BRC_RUNS_MAX"), define("BRC_RUNS_SUM")) == (capi.RUNS_MIN, capi.RUNS_MAX, capi.RUNS_SUM) == (0, 1, 2)
    assert define("BRC_RUNS_REF_N") == capi.RUNS_REF_N == 1
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


@pytest.mark.parametrize("build", ["sim", pytest.param("hip", marks=pytest.mark.gpu)])
def test_runs_handle_lifecycle(build):
    test_abi_side.test_handle_lifecycle(ROW, build)
