"""The site-selection library is a library of its own: it exports exactly what its header declares and the binding lists, its parameter
struct has the header's layout, it carries a kernel object of its own, leaves the engine's kernel object what it was, and the product
library neither links nor loads it."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

from conftest import ROOT

CSRC = os.path.join(ROOT, "bam_readcount_amd", "csrc")
SIM_DIR = os.path.join(ROOT, "tests", "sim_select")


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_select_exports_equal_the_header_and_the_binding():
    from bam_readcount_amd import capi
    declared = set(re.findall(r"\b(brc_select_\w+)\s*\(", _header("brc_select.h")))
    assert declared == set(capi.SELECT_EXPORTS)
    others = (set(capi.EXPORTS) | set(capi.INFLATE_EXPORTS) | set(capi.DEFLATE_EXPORTS) | set(capi.DENSE_EXPORTS) | set(capi.INDELS_EXPORTS) |
              set(capi.PANEL_EXPORTS))
    assert not set(capi.SELECT_EXPORTS) & others
    assert os.path.exists(capi.SELECT_LIB), "libbrc_select_hip.so is not built (make -C bam_readcount_amd/csrc)"
    subprocess.check_call(["make", "-s", "-C", SIM_DIR])
    for lib in (capi.SELECT_LIB, os.path.join(SIM_DIR, "libbrc_select_sim.so")):
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, check=True).stdout.decode()
        exported = {l.split()[-1] for l in syms.splitlines() if l.split()[-1].startswith("brc_")}
        assert exported == set(capi.SELECT_EXPORTS), lib
    for h in ("brc.h", "brc_inflate.h", "brc_deflate.h", "brc_dense.h", "brc_indels.h", "brc_panel.h"):
        assert not re.search(r"\bbrc_select_\w+\s*\(", _header(h)), h


def test_select_params_layout_and_constants_are_the_headers():
    from bam_readcount_amd import capi
    h = _header("brc_select.h")
    body = re.search(r"typedef struct brc_select_params \{(.*?)\} brc_select_params;", h, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, names = re.match(r"(const uint8_t\*|uint32_t)\s+(.*)", decl).groups()
        fields += [(n.strip(), typ) for n in names.split(",")]
    assert [n for n, _ in fields] == [n for n, _ in capi.SelectParams._fields_]
    for (n, typ), (_, ct) in zip(fields, capi.SelectParams._fields_):
        assert ct is (C.c_void_p if typ.endswith("*") else C.c_uint32), n
    assert C.sizeof(capi.SelectParams) == 48 and capi.SelectParams.flags.offset == 8 and capi.SelectParams.ctl_frac_den.offset == 40

    def define(name):
        return int(re.search(r"#define\s+%s\s+(\d+)u?\b" % name, h).group(1))
    assert (define("BRC_SELECT_SNV"), define("BRC_SELECT_INDEL")) == (capi.SELECT_SNV, capi.SELECT_INDEL) == (1, 2)
    assert (define("BRC_ROLE_IGNORE"), define("BRC_ROLE_CASE"), define("BRC_ROLE_CONTROL")) == (capi.ROLE_IGNORE, capi.ROLE_CASE, capi.ROLE_CONTROL) == (0, 1, 2)
    assert define("BRC_SELECT_MAX_LIB") == capi.SELECT_MAX_LIB == 254
    bits = tuple(define("BRC_WHY_" + n) for n in ("A", "C", "G", "T", "INS", "DEL"))
    assert bits == (capi.WHY_A, capi.WHY_C, capi.WHY_G, capi.WHY_T, capi.WHY_INS, capi.WHY_DEL) == (1, 2, 4, 8, 16, 32)
    assert "not compared" in open(os.path.join(ROOT, "include", "brc_select.h")).read().lower()      # the allele-blind veto is stated


def test_select_library_has_a_kernel_object_of_its_own():
    from bam_readcount_amd import capi
    h = capi.kernel_object_hash(capi.SELECT_LIB)
    assert h is not None and re.fullmatch(r"[0-9a-f]{16}", h)
    assert h not in (capi.kernel_object_hash(), capi.kernel_object_hash(capi.INFLATE_LIB), capi.kernel_object_hash(capi.DEFLATE_LIB),
                     capi.kernel_object_hash(capi.DENSE_LIB), capi.kernel_object_hash(capi.INDELS_LIB), capi.kernel_object_hash(capi.PANEL_LIB))
    assert capi.kernel_object_hash(os.path.join(SIM_DIR, "libbrc_select_sim.so")) is None
    blob = open(capi.SELECT_LIB, "rb").read()
    for k in (b"k_select_link", b"k_select_flag", b"k_select_why", b"k_select_parts", b"k_select_emit"):
        assert k in blob, k


def test_engine_kernel_object_still_equals_the_committed_stamps():
    from bam_readcount_amd import capi
    j = json.load(open(os.path.join(ROOT, "profiles", "r06_traffic.json")))
    for cfg in ("wgs30x", "tumor200x"):
        stamp = j[cfg]["kernel_object_sha256_16"]
        assert capi.kernel_object_hash() == stamp == "b699f7e6f23ebb67"
        assert capi.kernel_object_hash(os.path.join(CSRC, "libbrc_hip_testknobs.so")) == stamp


def test_product_library_neither_links_nor_loads_the_select_library():
    from bam_readcount_amd import capi
    for lib in (capi.PRODUCT_LIB, os.path.join(CSRC, "libbrc_hip_testknobs.so"), os.path.join(CSRC, "bam-readcount"), capi.DENSE_LIB, capi.INDELS_LIB,
                capi.PANEL_LIB):
        needed = subprocess.run(["readelf", "-d", lib], stdout=subprocess.PIPE, check=True).stdout.decode()
        assert "brc_select" not in needed, lib
        blob = open(lib, "rb").read()
        assert b"brc_select" not in blob and b"libbrc_select" not in blob, lib        # (no dlopen by name, no symbol looked up)
    # ... and the select library links nothing of the engine, nor of its siblings: the views are plain data
    needed = subprocess.run(["readelf", "-d", capi.SELECT_LIB], stdout=subprocess.PIPE, check=True).stdout.decode()
    assert "libbrc_" not in needed.replace("libbrc_select_hip.so", "")
    undefined = subprocess.run(["nm", "-D", "--undefined-only", capi.SELECT_LIB], stdout=subprocess.PIPE, check=True).stdout.decode()
    assert not [l for l in undefined.splitlines() if l.split()[-1].startswith("brc_")]


def test_the_select_sources_use_no_inline_assembly_and_the_siblings_flags():
    for f in ("brc_select.hip", "brc_select_core.h"):
        src = open(os.path.join(CSRC, f)).read()
        assert "asm" not in src and "brc_core.h" not in src and "brc_host.h" not in src, f
    mk = open(os.path.join(CSRC, "Makefile")).read()
    rule = mk[mk.index("brc_select.o:"):mk.index("libbrc_select_hip.so:")]
    assert "-ffp-contract=off" in rule and "-O3" in rule and "-std=c++17" in rule and "fast-math" not in rule and "-Ofast" not in rule
    assert "libbrc_select_hip.so" in mk[mk.index("all:"):mk.index("\n", mk.index("all:"))] and "libbrc_select_hip.so" in mk[mk.index("clean:"):]


def test_package_and_select_import_without_torch():
    """Importing the package, its tensors module and the select binding must not import torch; the CPU route of tensors.select needs
    numpy alone."""
    subprocess.check_call(["make", "-s", "-C", SIM_DIR])
    code = ("import sys; sys.path.insert(0, %r); import bam_readcount_amd; from bam_readcount_amd import capi, tensors; "
            "s = capi.Select(%r); assert s.kind() == 'sim' and callable(tensors.select); assert 'torch' not in sys.modules"
            % (ROOT, os.path.join(SIM_DIR, "libbrc_select_sim.so")))
    subprocess.check_call([sys.executable, "-c", code])


def test_select_library_refuses_to_exist_without_a_device_or_a_build():
    """capi.Select never substitutes: a missing library raises, and so does the hip library on a machine without a GPU."""
    import pytest
    from bam_readcount_amd import capi
    with pytest.raises(capi.BrcError):
        capi.Select(os.path.join(CSRC, "no_such_library.so"))
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(capi.BrcError) as ei:
            capi.Select()
        assert ei.value.rc == capi.E_NODEVICE
