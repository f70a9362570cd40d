"""The dense-results library is a library of its own: it exports exactly what its header declares and the binding lists, carries a
kernel object of its own, leaves the engine's kernel object what it was, and the product library neither links nor loads it."""
import json
import os
import re
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "bam_readcount_amd", "csrc")
SIM_DIR = os.path.join(ROOT, "tests", "sim_dense")


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_dense_exports_equal_the_header_and_the_binding():
    from bam_readcount_amd import capi
    declared = set(re.findall(r"\b(brc_dense_\w+)\s*\(", _header("brc_dense.h")))
    assert declared == set(capi.DENSE_EXPORTS)
    assert not set(capi.DENSE_EXPORTS) & (set(capi.EXPORTS) | set(capi.INFLATE_EXPORTS) | set(capi.DEFLATE_EXPORTS))
    assert os.path.exists(capi.DENSE_LIB), "libbrc_dense_hip.so is not built (make -C bam_readcount_amd/csrc)"
    subprocess.check_call(["make", "-s", "-C", SIM_DIR])
    for lib in (capi.DENSE_LIB, os.path.join(SIM_DIR, "libbrc_dense_sim.so")):
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, check=True).stdout.decode()
        exported = {l.split()[-1] for l in syms.splitlines() if l.split()[-1].startswith("brc_")}
        assert exported == set(capi.DENSE_EXPORTS), lib
    # the engine's side of the seam is one call of its own header; the other headers do not know the library
    assert "brc_device_view_get" in capi.EXPORTS and re.search(r"\bbrc_device_view_get\s*\(", _header("brc.h"))
    for h in ("brc.h", "brc_inflate.h", "brc_deflate.h"):
        assert not re.search(r"\bbrc_dense_\w+\s*\(", _header(h)), h


def test_view_struct_of_the_binding_has_the_header_layout():
    """capi.DeviceView against the C struct, field by field (offsets from a compile of the header)."""
    import ctypes as C
    from bam_readcount_amd import capi
    fields = [f for f, _ in capi.DeviceView._fields_]
    src = '#include <stddef.h>\n#include <stdio.h>\n#include "brc.h"\nint main(void) { printf("%zu", sizeof(brc_device_view));\n'
    src += "".join('printf(" %%zu", offsetof(brc_device_view, %s));\n' % f for f in fields) + "return 0; }\n"
    exe = os.path.join(SIM_DIR, "view_layout_check")
    try:
        subprocess.run(["gcc", "-x", "c", "-std=c99", "-I", os.path.join(ROOT, "include"), "-", "-o", exe], input=src.encode(), check=True)
        got = [int(x) for x in subprocess.run([exe], stdout=subprocess.PIPE, check=True).stdout.split()]
    finally:
        if os.path.exists(exe):
            os.remove(exe)
    assert got == [C.sizeof(capi.DeviceView)] + [getattr(capi.DeviceView, f).offset for f in fields]
    assert (capi.MEM_DEVICE, capi.MEM_HOST) == tuple(int(re.search(r"#define\s+%s\s+(\d+)" % n, _header("brc.h")).group(1)) for n in ("BRC_MEM_DEVICE", "BRC_MEM_HOST"))


def test_dense_library_has_a_kernel_object_of_its_own():
    from bam_readcount_amd import capi
    h = capi.kernel_object_hash(capi.DENSE_LIB)
    assert h is not None and re.fullmatch(r"[0-9a-f]{16}", h)
    assert h not in (capi.kernel_object_hash(), capi.kernel_object_hash(capi.INFLATE_LIB), capi.kernel_object_hash(capi.DEFLATE_LIB))
    assert capi.kernel_object_hash(os.path.join(SIM_DIR, "libbrc_dense_sim.so")) is None


def test_engine_kernel_object_still_equals_the_committed_stamps():
    from bam_readcount_amd import capi
    j = json.load(open(os.path.join(ROOT, "profiles", "r06_traffic.json")))
    for cfg in ("wgs30x", "tumor200x"):
        stamp = j[cfg]["kernel_object_sha256_16"]
        assert capi.kernel_object_hash() == stamp
        assert capi.kernel_object_hash(os.path.join(CSRC, "libbrc_hip_testknobs.so")) == stamp


def test_product_library_neither_links_nor_loads_the_dense_library():
    from bam_readcount_amd import capi
    for lib in (capi.PRODUCT_LIB, os.path.join(CSRC, "libbrc_hip_testknobs.so"), os.path.join(CSRC, "bam-readcount")):
        needed = subprocess.run(["readelf", "-d", lib], stdout=subprocess.PIPE, check=True).stdout.decode()
        assert "brc_dense" not in needed, lib
        blob = open(lib, "rb").read()
        assert b"brc_dense" not in blob and b"libbrc_dense" not in blob, lib        # (no dlopen by name, no symbol looked up)
    # ... and the dense library links nothing of the engine: the view is plain data
    needed = subprocess.run(["readelf", "-d", capi.DENSE_LIB], stdout=subprocess.PIPE, check=True).stdout.decode()
    assert "libbrc_" not in needed.replace("libbrc_dense_hip.so", "")
    undefined = subprocess.run(["nm", "-D", "--undefined-only", capi.DENSE_LIB], stdout=subprocess.PIPE, check=True).stdout.decode()
    assert not [l for l in undefined.splitlines() if l.split()[-1].startswith("brc_")]


def test_the_dense_sources_use_no_inline_assembly_and_no_fast_math():
    for f in ("brc_dense.hip", "brc_dense_core.h"):
        assert "asm" not in open(os.path.join(CSRC, f)).read()
    mk = open(os.path.join(CSRC, "Makefile")).read()
    rule = mk[mk.index("brc_dense.o:"):mk.index("libbrc_dense_hip.so:")]
    assert "-ffp-contract=off" in rule and "fast-math" not in rule and "-Ofast" not in rule


def test_package_imports_without_torch():
    """Importing the package and its tensors module must not import torch (the CPU route needs numpy alone)."""
    import sys
    code = ("import sys; sys.path.insert(0, %r); import bam_readcount_amd; from bam_readcount_amd import tensors; "
            "assert 'torch' not in sys.modules; assert 'tensors' in bam_readcount_amd.__doc__" % ROOT)
    subprocess.check_call([sys.executable, "-c", code])


def test_engine_loaded_before_torch_shares_one_hip_runtime():
    """A process that loads the HIP libraries first and imports torch afterwards must hold ONE HIP runtime (capi._load): with two, the
    second finds no GPU and a tensor can never meet a view.  (Checked on the process's own map; no GPU needed.  The GPU half:
    tests/test_tensors_gpu.py::test_engine_created_before_torch_is_imported.)"""
    import sys
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from bam_readcount_amd import capi\n"
            "capi.load_product(); capi.Library(%r)\n"
            "try:\n    capi.Dense()\nexcept capi.BrcError as e:\n    assert getattr(e, 'rc', 0) != 0      # (no device here: created nothing, but the library is loaded)\n"
            "assert 'torch' not in sys.modules\n"
            "import torch\n"
            "for name in ('libamdhip64', 'libhsa-runtime64'):\n"
            "    files = sorted({l.split()[-1] for l in open('/proc/self/maps') if name in l})\n"
            "    assert len(files) == 1, files\n" % (ROOT, os.path.join(CSRC, "libbrc_hip_testknobs.so")))
    subprocess.check_call([sys.executable, "-c", code])
