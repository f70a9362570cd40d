"""The site-panel library is a library of its own: it exports exactly what its header declares and the binding lists, carries a kernel
object of its own, leaves the engine's kernel object what it was, and the product library neither links nor loads it."""
import json
import os
import re
import subprocess
import sys

from conftest import ROOT

CSRC = os.path.join(ROOT, "bam_readcount_amd", "csrc")
SIM_DIR = os.path.join(ROOT, "tests", "sim_panel")


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_panel_exports_equal_the_header_and_the_binding():
    from bam_readcount_amd import capi
    declared = set(re.findall(r"\b(brc_panel_\w+)\s*\(", _header("brc_panel.h")))
    assert declared == set(capi.PANEL_EXPORTS)
    others = set(capi.EXPORTS) | set(capi.INFLATE_EXPORTS) | set(capi.DEFLATE_EXPORTS) | set(capi.DENSE_EXPORTS) | set(capi.INDELS_EXPORTS)
    assert not set(capi.PANEL_EXPORTS) & others
    assert os.path.exists(capi.PANEL_LIB), "libbrc_panel_hip.so is not built (make -C bam_readcount_amd/csrc)"
    subprocess.check_call(["make", "-s", "-C", SIM_DIR])
    for lib in (capi.PANEL_LIB, os.path.join(SIM_DIR, "libbrc_panel_sim.so")):
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, check=True).stdout.decode()
        exported = {l.split()[-1] for l in syms.splitlines() if l.split()[-1].startswith("brc_")}
        assert exported == set(capi.PANEL_EXPORTS), lib
    # the other headers do not know the library; the bits of the status word are the header's
    for h in ("brc.h", "brc_inflate.h", "brc_deflate.h", "brc_dense.h", "brc_indels.h"):
        assert not re.search(r"\bbrc_panel_\w+\s*\(", _header(h)), h
    bits = tuple(int(re.search(r"#define\s+%s\s+(\d+)u" % n, _header("brc_panel.h")).group(1)) for n in ("BRC_PANEL_OUT_OF_RANGE", "BRC_PANEL_NOT_ASCENDING"))
    assert bits == (capi.PANEL_OUT_OF_RANGE, capi.PANEL_NOT_ASCENDING) == (1, 2)


def test_panel_library_has_a_kernel_object_of_its_own():
    from bam_readcount_amd import capi
    h = capi.kernel_object_hash(capi.PANEL_LIB)
    assert h is not None and re.fullmatch(r"[0-9a-f]{16}", h)
    assert h not in (capi.kernel_object_hash(), capi.kernel_object_hash(capi.INFLATE_LIB), capi.kernel_object_hash(capi.DEFLATE_LIB),
                     capi.kernel_object_hash(capi.DENSE_LIB), capi.kernel_object_hash(capi.INDELS_LIB))
    assert capi.kernel_object_hash(os.path.join(SIM_DIR, "libbrc_panel_sim.so")) is None
    blob = open(capi.PANEL_LIB, "rb").read()
    assert b"k_panel_planes" in blob and b"k_panel_overlay" in blob


def test_engine_kernel_object_still_equals_the_committed_stamps():
    from bam_readcount_amd import capi
    j = json.load(open(os.path.join(ROOT, "profiles", "r06_traffic.json")))
    for cfg in ("wgs30x", "tumor200x"):
        stamp = j[cfg]["kernel_object_sha256_16"]
        assert capi.kernel_object_hash() == stamp
        assert capi.kernel_object_hash(os.path.join(CSRC, "libbrc_hip_testknobs.so")) == stamp


def test_product_library_neither_links_nor_loads_the_panel_library():
    from bam_readcount_amd import capi
    for lib in (capi.PRODUCT_LIB, os.path.join(CSRC, "libbrc_hip_testknobs.so"), os.path.join(CSRC, "bam-readcount"), capi.DENSE_LIB, capi.INDELS_LIB):
        needed = subprocess.run(["readelf", "-d", lib], stdout=subprocess.PIPE, check=True).stdout.decode()
        assert "brc_panel" not in needed, lib
        blob = open(lib, "rb").read()
        assert b"brc_panel" not in blob and b"libbrc_panel" not in blob, lib        # (no dlopen by name, no symbol looked up)
    # ... and the panel library links nothing of the engine: the view is plain data
    needed = subprocess.run(["readelf", "-d", capi.PANEL_LIB], stdout=subprocess.PIPE, check=True).stdout.decode()
    assert "libbrc_" not in needed.replace("libbrc_panel_hip.so", "")
    undefined = subprocess.run(["nm", "-D", "--undefined-only", capi.PANEL_LIB], stdout=subprocess.PIPE, check=True).stdout.decode()
    assert not [l for l in undefined.splitlines() if l.split()[-1].startswith("brc_")]


def test_the_panel_sources_use_no_inline_assembly_and_no_fast_math():
    for f in ("brc_panel.hip", "brc_panel_core.h"):
        assert "asm" not in open(os.path.join(CSRC, f)).read()
    mk = open(os.path.join(CSRC, "Makefile")).read()
    rule = mk[mk.index("brc_panel.o:"):mk.index("libbrc_panel_hip.so:")]
    assert "-ffp-contract=off" in rule and "fast-math" not in rule and "-Ofast" not in rule
    assert "libbrc_panel_hip.so" in mk[mk.index("all:"):mk.index("\n", mk.index("all:"))] and "libbrc_panel_hip.so" in mk[mk.index("clean:"):]


def test_package_and_sites_import_without_torch():
    """Importing the package, its tensors module and the panel binding must not import torch; the CPU route of tensors.sites needs
    numpy alone."""
    subprocess.check_call(["make", "-s", "-C", SIM_DIR])
    code = ("import sys; sys.path.insert(0, %r); import bam_readcount_amd; from bam_readcount_amd import capi, tensors; "
            "p = capi.Panel(%r); assert p.kind() == 'sim' and callable(tensors.sites); assert 'torch' not in sys.modules"
            % (ROOT, os.path.join(SIM_DIR, "libbrc_panel_sim.so")))
    subprocess.check_call([sys.executable, "-c", code])


def test_panel_library_refuses_to_exist_without_a_device_or_a_build():
    """capi.Panel never substitutes: a missing library raises, and so does the hip library on a machine without a GPU."""
    import pytest
    from bam_readcount_amd import capi
    with pytest.raises(capi.BrcError):
        capi.Panel(os.path.join(CSRC, "no_such_library.so"))
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(capi.BrcError) as ei:
            capi.Panel()
        assert ei.value.rc == capi.E_NODEVICE
