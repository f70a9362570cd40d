"""The inflater is a library of its own: the engine's kernel object is what it was, the new library carries its own, its exports are
the ones the binding lists, and no source file of the tree names an instruction the shared GPU pool forbids."""
import json
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "bam_readcount_amd", "csrc")


def test_engine_kernel_object_is_unchanged():
    """The constraint of the inflater's design, next to its cause: device code added to libbrc_hip.so would change this hash, fail
    tests/test_abi.py and make bench.py drop its traffic fields."""
    from bam_readcount_amd import capi
    j = json.load(open(os.path.join(ROOT, "profiles", "r06_traffic.json")))
    for cfg in ("wgs30x", "tumor200x"):
        stamp = j[cfg]["kernel_object_sha256_16"]
        assert capi.kernel_object_hash() == stamp
        assert capi.kernel_object_hash(os.path.join(CSRC, "libbrc_hip_testknobs.so")) == stamp


def test_inflater_library_has_a_kernel_object_of_its_own():
    from bam_readcount_amd import capi
    assert os.path.exists(capi.INFLATE_LIB), "libbrc_inflate_hip.so is not built (make -C bam_readcount_amd/csrc)"
    h = capi.kernel_object_hash(capi.INFLATE_LIB)
    assert h is not None and re.fullmatch(r"[0-9a-f]{16}", h) and h != capi.kernel_object_hash()


def test_inflater_exports_equal_the_header_and_the_binding():
    from bam_readcount_amd import capi
    hdr = open(os.path.join(ROOT, "include", "brc_inflate.h")).read()
    declared = set(re.findall(r"\b(brc_inflat\w+)\s*\(", hdr))
    assert declared == set(capi.INFLATE_EXPORTS)
    assert not set(capi.INFLATE_EXPORTS) & set(capi.EXPORTS)
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "sim_inflate")])
    for lib in (capi.INFLATE_LIB, os.path.join(ROOT, "tests", "sim_inflate", "libbrc_inflate_sim.so")):
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, check=True).stdout.decode()
        exported = {l.split()[-1] for l in syms.splitlines() if l.split()[-1].startswith("brc_")}
        assert exported == set(capi.INFLATE_EXPORTS), lib
    # the engine's header does not know the inflater
    assert "brc_inflat" not in open(os.path.join(ROOT, "include", "brc.h")).read()


def test_no_forbidden_instruction_is_named_in_the_sources():
    """Scalar stores to memory, scalar atomics and scalar-cache write-backs must not appear in any source file, strings and comments
    included (documents may speak of them)."""
    words = [a + b for a, b in (("s_st", "ore_"), ("s_buffer_st", "ore_"), ("s_scratch_st", "ore_"), ("s_ato", "mic_"), ("s_buffer_ato", "mic_"),
                                ("s_dcache_", "wb"), ("s_dcache_", "discard"))]
    pat = re.compile("|".join(words), re.I)
    hits = []
    files = subprocess.run(["git", "-C", ROOT, "ls-files", "-co", "--exclude-standard"], stdout=subprocess.PIPE).stdout.decode().split("\n")
    if not any(files):
        files = [os.path.relpath(os.path.join(dp, f), ROOT) for dp, _, fs in os.walk(ROOT) for f in fs]
    for f in files:
        if not f or f.endswith((".md", ".rst", ".txt", ".so", ".o", ".bam", ".npz", ".cram", ".bai", ".crai", ".json", ".csv", ".log")):
            continue
        path = os.path.join(ROOT, f)
        if not os.path.isfile(path) or os.path.getsize(path) > (4 << 20):
            continue
        try:
            text = open(path, errors="ignore").read()
        except OSError:
            continue
        if pat.search(text):
            hits.append(f)
    assert not hits, hits
    for f in ("brc_inflate.hip", "brc_inflate_core.h", "brc_inflate_plan.h"):
        assert not pat.search(open(os.path.join(CSRC, f)).read())
        assert "asm" not in open(os.path.join(CSRC, f)).read()
