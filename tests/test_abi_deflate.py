"""The deflater is a library of its own: the engine's kernel object is what it was, the new library carries its own, and its exports
are the ones the header declares and the binding lists."""
import json
import os
import re
import subprocess

from conftest import ROOT


def test_deflater_exports_equal_the_header_and_the_binding():
    from bam_readcount_amd import capi
    hdr = open(os.path.join(ROOT, "include", "brc_deflate.h")).read()
    declared = set(re.findall(r"\b(brc_deflat\w+)\s*\(", hdr))
    assert declared == set(capi.DEFLATE_EXPORTS)
    assert not set(capi.DEFLATE_EXPORTS) & (set(capi.EXPORTS) | set(capi.INFLATE_EXPORTS))
    assert os.path.exists(capi.DEFLATE_LIB), "libbrc_deflate_hip.so is not built (make -C bam_readcount_amd/csrc)"
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "sim_deflate")])
    for lib in (capi.DEFLATE_LIB, os.path.join(ROOT, "tests", "sim_deflate", "libbrc_deflate_sim.so")):
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, check=True).stdout.decode()
        exported = {l.split()[-1] for l in syms.splitlines() if l.split()[-1].startswith("brc_")}
        assert exported == set(capi.DEFLATE_EXPORTS), lib
    for h in ("brc.h", "brc_inflate.h"):
        assert "brc_deflat" not in open(os.path.join(ROOT, "include", h)).read()


def test_deflater_library_has_a_kernel_object_of_its_own():
    from bam_readcount_amd import capi
    h = capi.kernel_object_hash(capi.DEFLATE_LIB)
    assert h is not None and re.fullmatch(r"[0-9a-f]{16}", h)
    assert h != capi.kernel_object_hash() and h != capi.kernel_object_hash(capi.INFLATE_LIB)


def test_engine_kernel_object_still_equals_the_committed_stamp():
    from bam_readcount_amd import capi
    j = json.load(open(os.path.join(ROOT, "profiles", "r06_traffic.json")))
    for cfg in ("wgs30x", "tumor200x"):
        assert capi.kernel_object_hash() == j[cfg]["kernel_object_sha256_16"]


def test_the_deflater_sources_use_no_inline_assembly():
    csrc = os.path.join(ROOT, "bam_readcount_amd", "csrc")
    for f in ("brc_deflate.hip", "brc_deflate_core.h", "brc_codec_hip.h"):
        assert "asm" not in open(os.path.join(csrc, f)).read()
