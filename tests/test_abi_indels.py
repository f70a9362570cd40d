"""The indel-table library is a library of its own: it exports exactly what its header declares and the binding lists, carries a kernel
object of its own, leaves the engine's kernel object what it was, and the product library neither links nor loads it."""
import json
import os
import re
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "bam_readcount_amd", "csrc")
SIM_DIR = os.path.join(ROOT, "tests", "sim_indels")


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_indels_exports_equal_the_header_and_the_binding():
    from bam_readcount_amd import capi
    declared = set(re.findall(r"\b(brc_indels_\w+)\s*\(", _header("brc_indels.h")))
    assert declared == set(capi.INDELS_EXPORTS)
    others = set(capi.EXPORTS) | set(capi.INFLATE_EXPORTS) | set(capi.DEFLATE_EXPORTS) | set(capi.DENSE_EXPORTS)
    assert not set(capi.INDELS_EXPORTS) & others
    assert os.path.exists(capi.INDELS_LIB), "libbrc_indels_hip.so is not built (make -C bam_readcount_amd/csrc)"
    subprocess.check_call(["make", "-s", "-C", SIM_DIR], stderr=subprocess.DEVNULL)
    for lib in (capi.INDELS_LIB, os.path.join(SIM_DIR, "libbrc_indels_sim.so")):
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, check=True).stdout.decode()
        exported = {l.split()[-1] for l in syms.splitlines() if l.split()[-1].startswith("brc_")}
        assert exported == set(capi.INDELS_EXPORTS), lib
    # the engine's side of the seam is one call of its own header; the other headers do not know the library
    assert "brc_device_indels_get" in capi.EXPORTS and re.search(r"\bbrc_device_indels_get\s*\(", _header("brc.h"))
    for h in ("brc.h", "brc_inflate.h", "brc_deflate.h", "brc_dense.h"):
        assert not re.search(r"\bbrc_indels_\w+\s*\(", _header(h)), h
    # ... and the engine libraries export it
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "sim")])
    for lib in (capi.PRODUCT_LIB, os.path.join(CSRC, "libbrc_hip_testknobs.so"), os.path.join(ROOT, "tests", "sim", "libbrc_sim.so")):
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, check=True).stdout.decode()
        assert "brc_device_indels_get" in {l.split()[-1] for l in syms.splitlines()}, lib


def test_indels_struct_of_the_binding_has_the_header_layout():
    """capi.DeviceIndels against the C struct, field by field (offsets from a compile of the header)."""
    import ctypes as C
    from bam_readcount_amd import capi
    fields = [f for f, _ in capi.DeviceIndels._fields_]
    src = '#include <stddef.h>\n#include <stdio.h>\n#include "brc.h"\nint main(void) { printf("%zu", sizeof(brc_device_indels));\n'
    src += "".join('printf(" %%zu", offsetof(brc_device_indels, %s));\n' % f for f in fields) + "return 0; }\n"
    exe = os.path.join(SIM_DIR, "indels_layout_check")
    try:
        subprocess.run(["gcc", "-x", "c", "-std=c99", "-I", os.path.join(ROOT, "include"), "-", "-o", exe], input=src.encode(), check=True)
        got = [int(x) for x in subprocess.run([exe], stdout=subprocess.PIPE, check=True).stdout.split()]
    finally:
        if os.path.exists(exe):
            os.remove(exe)
    assert got == [C.sizeof(capi.DeviceIndels)] + [getattr(capi.DeviceIndels, f).offset for f in fields]
    # every member of the C struct is in the binding: a struct of the listed fields, packed as C packs them, has the C size
    members = re.search(r"typedef struct brc_device_indels \{(.*?)\} brc_device_indels;", _header("brc.h"), re.S).group(1)
    names = [n.strip(" *") for decl in members.split(";") if decl.strip() for n in decl.split(",")]
    assert [n.split()[-1].lstrip("*") for n in names] == fields
    # the record layout the header documents is the engine's
    core = open(os.path.join(CSRC, "brc_core.h")).read()
    assert "struct IndelOut { int32_t pos, lib, len; uint32_t rep_read; int32_t rep_qpos; uint32_t i[NI]; float f[NF]; };" in core


def test_indels_library_has_a_kernel_object_of_its_own():
    from bam_readcount_amd import capi
    h = capi.kernel_object_hash(capi.INDELS_LIB)
    assert h is not None and re.fullmatch(r"[0-9a-f]{16}", h)
    assert h not in (capi.kernel_object_hash(), capi.kernel_object_hash(capi.INFLATE_LIB), capi.kernel_object_hash(capi.DEFLATE_LIB),
                     capi.kernel_object_hash(capi.DENSE_LIB))
    assert capi.kernel_object_hash(os.path.join(SIM_DIR, "libbrc_indels_sim.so")) is None


def test_engine_kernel_object_still_equals_the_committed_stamps():
    from bam_readcount_amd import capi
    j = json.load(open(os.path.join(ROOT, "profiles", "r06_traffic.json")))
    for cfg in ("wgs30x", "tumor200x"):
        stamp = j[cfg]["kernel_object_sha256_16"]
        assert capi.kernel_object_hash() == stamp
        assert capi.kernel_object_hash(os.path.join(CSRC, "libbrc_hip_testknobs.so")) == stamp


def test_product_library_neither_links_nor_loads_the_indels_library():
    from bam_readcount_amd import capi
    for lib in (capi.PRODUCT_LIB, os.path.join(CSRC, "libbrc_hip_testknobs.so"), os.path.join(CSRC, "bam-readcount"), capi.DENSE_LIB):
        needed = subprocess.run(["readelf", "-d", lib], stdout=subprocess.PIPE, check=True).stdout.decode()
        assert "brc_indels" not in needed, lib
        blob = open(lib, "rb").read()
        assert b"brc_indels" not in blob and b"libbrc_indels" not in blob, lib        # (no dlopen by name, no symbol looked up)
    # ... and the indels library links nothing of the engine: the view is plain data
    needed = subprocess.run(["readelf", "-d", capi.INDELS_LIB], stdout=subprocess.PIPE, check=True).stdout.decode()
    assert "libbrc_" not in needed.replace("libbrc_indels_hip.so", "")
    undefined = subprocess.run(["nm", "-D", "--undefined-only", capi.INDELS_LIB], stdout=subprocess.PIPE, check=True).stdout.decode()
    assert not [l for l in undefined.splitlines() if l.split()[-1].startswith("brc_")]


def test_the_indels_sources_use_no_inline_assembly_and_no_fast_math():
    for f in ("brc_indels.hip", "brc_indels_core.h"):
        assert "asm" not in open(os.path.join(CSRC, f)).read()
    mk = open(os.path.join(CSRC, "Makefile")).read()
    rule = mk[mk.index("brc_indels.o:"):mk.index("libbrc_indels_hip.so:")]
    assert "-ffp-contract=off" in rule and "fast-math" not in rule and "-Ofast" not in rule
    assert "libbrc_indels_hip.so" in mk[mk.index("all:"):mk.index("\n", mk.index("all:"))] and "libbrc_indels_hip.so" in mk[mk.index("clean:"):]


def test_indels_library_refuses_to_exist_without_a_device_or_a_build():
    """capi.Indels never substitutes: a missing library raises, and so does the hip library on a machine without a GPU."""
    import pytest
    from bam_readcount_amd import capi
    with pytest.raises(capi.BrcError):
        capi.Indels(os.path.join(CSRC, "no_such_library.so"))
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(capi.BrcError) as ei:
            capi.Indels()
        assert ei.value.rc == capi.E_NODEVICE
