"""The window-summary library is a library of its own: it exports exactly what its header declares and the binding lists, its parameter
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
SIM_DIR = os.path.join(ROOT, "tests", "sim_bins")


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_bins_exports_equal_the_header_and_the_binding():
    from bam_readcount_amd import capi
    declared = set(re.findall(r"\b(brc_bins_\w+)\s*\(", _header("brc_bins.h")))
    assert declared == set(capi.BINS_EXPORTS)
    others = (set(capi.EXPORTS) | set(capi.INFLATE_EXPORTS) | set(capi.DEFLATE_EXPORTS) | set(capi.DENSE_EXPORTS) | set(capi.INDELS_EXPORTS) |
              set(capi.PANEL_EXPORTS) | set(capi.SELECT_EXPORTS))
    assert not set(capi.BINS_EXPORTS) & others
    assert os.path.exists(capi.BINS_LIB), "libbrc_bins_hip.so is not built (make -C bam_readcount_amd/csrc)"
    subprocess.check_call(["make", "-s", "-C", SIM_DIR])
    for lib in (capi.BINS_LIB, os.path.join(SIM_DIR, "libbrc_bins_sim.so")):
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, check=True).stdout.decode()
        exported = {l.split()[-1] for l in syms.splitlines() if l.split()[-1].startswith("brc_")}
        assert exported == set(capi.BINS_EXPORTS), lib
    for h in ("brc.h", "brc_inflate.h", "brc_deflate.h", "brc_dense.h", "brc_indels.h", "brc_panel.h", "brc_select.h"):
        assert not re.search(r"\bbrc_bins_\w+\s*\(", _header(h)), h


def test_bins_params_layout_and_constants_are_the_headers():
    from bam_readcount_amd import capi
    h = _header("brc_bins.h")
    body = re.search(r"typedef struct brc_bins_params \{(.*?)\} brc_bins_params;", h, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, name = re.match(r"(const int32_t\*|int64_t|int32_t|uint32_t)\s+(\w+(?:\[\w+\])?)$", decl).groups()
        fields.append((name.split("[")[0], typ, "[" in name))
    assert [n for n, _, _ in fields] == [n for n, _ in capi.BinsParams._fields_]
    ctype = {"const int32_t*": C.c_void_p, "int64_t": C.c_int64, "int32_t": C.c_int32, "uint32_t": C.c_uint32}
    for (n, typ, arr), (_, ct) in zip(fields, capi.BinsParams._fields_):
        assert ct is ctype[typ] if not arr else (ct._type_ is ctype[typ] and ct._length_ == capi.BINS_MAX_THR), n
    P = capi.BinsParams
    assert C.sizeof(P) == 64 and (P.edges.offset, P.width.offset, P.n_bins.offset, P.n_thr.offset, P.n_hist.offset, P.thr.offset) == (0, 8, 16, 24, 28, 32)

    def define(name):
        return int(re.search(r"#define\s+%s\s+(\d+)u?\b" % name, h).group(1))
    assert (define("BRC_BINS_NSUM"), define("BRC_BINS_MAX_THR"), define("BRC_BINS_MAX_HIST"), define("BRC_BINS_MAX_LIB")) == \
        (capi.BINS_NSUM, capi.BINS_MAX_THR, capi.BINS_MAX_HIST, capi.BINS_MAX_LIB) == (12, 8, 4096, 65535)
    names = ("DEPTH", "NCOL", "BUCKET", "NONREF", "INS", "DEL", "MAXDEPTH")
    assert tuple(define("BRC_BINS_S_" + n) for n in names) == tuple(getattr(capi, "BINS_S_" + n) for n in names) == (0, 1, 2, 8, 9, 10, 11)
    assert (define("BRC_BINS_DESCENDS"), define("BRC_BINS_OUTSIDE")) == (capi.BINS_DESCENDS, capi.BINS_OUTSIDE) == (1, 2)


def test_bins_library_has_a_kernel_object_of_its_own():
    from bam_readcount_amd import capi
    h = capi.kernel_object_hash(capi.BINS_LIB)
    assert h is not None and re.fullmatch(r"[0-9a-f]{16}", h)
    assert h not in (capi.kernel_object_hash(), capi.kernel_object_hash(capi.INFLATE_LIB), capi.kernel_object_hash(capi.DEFLATE_LIB),
                     capi.kernel_object_hash(capi.DENSE_LIB), capi.kernel_object_hash(capi.INDELS_LIB), capi.kernel_object_hash(capi.PANEL_LIB),
                     capi.kernel_object_hash(capi.SELECT_LIB))
    assert capi.kernel_object_hash(os.path.join(SIM_DIR, "libbrc_bins_sim.so")) is None
    blob = open(capi.BINS_LIB, "rb").read()
    for k in (b"k_bins_clear", b"k_bins_edges", b"k_bins_planes", b"k_bins_records", b"k_bins_indels"):
        assert k in blob, k


def test_engine_kernel_object_still_equals_the_committed_stamps():
    from bam_readcount_amd import capi
    j = json.load(open(os.path.join(ROOT, "profiles", "r06_traffic.json")))
    for cfg in ("wgs30x", "tumor200x"):
        stamp = j[cfg]["kernel_object_sha256_16"]
        assert capi.kernel_object_hash() == stamp == "b699f7e6f23ebb67"
        assert capi.kernel_object_hash(os.path.join(CSRC, "libbrc_hip_testknobs.so")) == stamp


def test_product_library_neither_links_nor_loads_the_bins_library():
    from bam_readcount_amd import capi
    for lib in (capi.PRODUCT_LIB, os.path.join(CSRC, "libbrc_hip_testknobs.so"), os.path.join(CSRC, "bam-readcount"), capi.DENSE_LIB, capi.INDELS_LIB,
                capi.PANEL_LIB, capi.SELECT_LIB):
        needed = subprocess.run(["readelf", "-d", lib], stdout=subprocess.PIPE, check=True).stdout.decode()
        assert "brc_bins" not in needed, lib
        blob = open(lib, "rb").read()
        assert b"brc_bins" not in blob and b"libbrc_bins" not in blob, lib        # (no dlopen by name, no symbol looked up)
    # ... and the bins library links nothing of the engine, nor of its siblings: the views are plain data
    needed = subprocess.run(["readelf", "-d", capi.BINS_LIB], stdout=subprocess.PIPE, check=True).stdout.decode()
    assert "libbrc_" not in needed.replace("libbrc_bins_hip.so", "")
    undefined = subprocess.run(["nm", "-D", "--undefined-only", capi.BINS_LIB], stdout=subprocess.PIPE, check=True).stdout.decode()
    assert not [l for l in undefined.splitlines() if l.split()[-1].startswith("brc_")]


def test_the_bins_sources_use_no_inline_assembly_and_the_siblings_flags():
    for f in ("brc_bins.hip", "brc_bins_core.h"):
        src = open(os.path.join(CSRC, f)).read()
        assert "asm" not in src and "brc_core.h" not in src and "brc_host.h" not in src, f
    mk = open(os.path.join(CSRC, "Makefile")).read()
    rule = mk[mk.index("brc_bins.o:"):mk.index("libbrc_bins_hip.so:")]
    assert "-ffp-contract=off" in rule and "-O3" in rule and "-std=c++17" in rule and "fast-math" not in rule and "-Ofast" not in rule
    assert "libbrc_bins_hip.so" in mk[mk.index("all:"):mk.index("\n", mk.index("all:"))] and "libbrc_bins_hip.so" in mk[mk.index("clean:"):]


def test_package_and_bins_import_without_torch():
    """Importing the package, its tensors module and the bins binding must not import torch; the CPU route of tensors.bins needs
    numpy alone."""
    subprocess.check_call(["make", "-s", "-C", SIM_DIR])
    code = ("import sys; sys.path.insert(0, %r); import bam_readcount_amd; from bam_readcount_amd import capi, tensors; "
            "s = capi.Bins(%r); assert s.kind() == 'sim' and callable(tensors.bins); assert 'torch' not in sys.modules"
            % (ROOT, os.path.join(SIM_DIR, "libbrc_bins_sim.so")))
    subprocess.check_call([sys.executable, "-c", code])


def test_bins_library_refuses_to_exist_without_a_device_or_a_build():
    """capi.Bins never substitutes: a missing library raises, and so does the hip library on a machine without a GPU."""
    import pytest
    from bam_readcount_amd import capi
    with pytest.raises(capi.BrcError):
        capi.Bins(os.path.join(CSRC, "no_such_library.so"))
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(capi.BrcError) as ei:
            capi.Bins()
        assert ei.value.rc == capi.E_NODEVICE
