"""The consensus caller is a library of its own: it exports exactly what its header declares and the binding lists, its parameter and
table structs have the header's layout, its constants are the header's, it carries a kernel object of its own, leaves the engine's
kernel object and the siblings' what they were, and neither the product nor a sibling links or loads it.  It is no row of
tests/abi_side.py's table yet (the table is pinned to ten rows): this module states its own row and runs the table's checks over it
where they take one, and restates the others."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest

import abi_side as side
from abi_side import define
import test_cons as tc

NAME = "cons"
KERNELS = ("k_cons_link", "k_cons_records", "k_cons_sites", "k_cons_emit", "k_side_scan_reduce", "k_side_scan_parts", "k_side_scan_apply")


def _lib():
    from bam_readcount_amd import consensus as cc
    return cc.CONS_LIB


def test_cons_exports_equal_the_header_and_the_binding():
    from bam_readcount_amd import capi, consensus as cc
    declared = set(re.findall(r"\b(brc_cons_\w+)\s*\(", side._header("brc_cons.h")))
    assert declared == set(cc.CONS_EXPORTS) and len(cc.CONS_EXPORTS) == 7
    others = set(capi.EXPORTS) | set(capi.INFLATE_EXPORTS) | set(capi.DEFLATE_EXPORTS)
    for r in side.ROWS:
        others |= set(side._exports(r))
    assert not set(cc.CONS_EXPORTS) & others
    assert os.path.exists(_lib()), "libbrc_cons_hip.so is not built (make -C bam_readcount_amd/csrc)"
    for lib in (_lib(), tc.cons_sim_lib()):
        assert {s for s in side._defined(lib) if s.startswith("brc_")} == set(cc.CONS_EXPORTS), lib
    # no other header knows the library, and capi does not bind it
    for h in ["brc.h", "brc_inflate.h", "brc_deflate.h"] + ["brc_%s.h" % r["name"] for r in side.ROWS]:
        assert not re.search(r"\bbrc_cons_\w+\s*\(", side._header(h)), h
    assert not [n for n in dir(capi) if n.upper().startswith("CONS")]


def test_cons_structs_and_constants_are_the_headers(tmp_path):
    from bam_readcount_amd import consensus as cc
    h = side._header("brc_cons.h")
    side.check_struct(tmp_path, "brc_cons.h", "brc_cons_params", cc.ConsParams)
    side.check_struct(tmp_path, "brc_cons.h", "brc_cons_table", cc.ConsTable)
    assert C.sizeof(cc.ConsParams) == 48 and cc.ConsParams.flags.offset == 8 and cc.ConsParams.gap.offset == 44
    assert C.sizeof(cc.ConsTable) == 72 and cc.ConsTable.count.offset == 40 and cc.ConsTable.alleles_len.offset == 64
    assert (define(h, "BRC_CONS_ALIGNED"), define(h, "BRC_CONS_FILL_REF"), define(h, "BRC_CONS_INS_CENTRIC")) == \
        (cc.CONS_ALIGNED, cc.CONS_FILL_REF, cc.CONS_INS_CENTRIC) == (1, 2, 4)
    assert (define(h, "BRC_CONS_TABLE_NOT_ASCENDING"), define(h, "BRC_CONS_TABLE_OUT_OF_RANGE")) == (cc.CONS_TABLE_NOT_ASCENDING, cc.CONS_TABLE_OUT_OF_RANGE) == (1, 2)
    assert define(h, "BRC_CONS_MAX_LIB") == cc.CONS_MAX_LIB == define(side._header("brc_select.h"), "BRC_SELECT_MAX_LIB") == 254
    assert define(h, "BRC_CONS_NCNT") == cc.CONS_NCNT == len(cc.CONS_C_NAMES) == 6 and define(h, "BRC_CONS_NO_INS") == cc.CONS_NO_INS == 2 ** 32 - 1
    assert tuple(define(h, "BRC_CONS_C_" + n.upper()) for n in cc.CONS_C_NAMES) == tuple(range(6))
    raw = open(os.path.join(side.ROOT, "include", "brc_cons.h")).read()
    assert cc.CONS_IUPAC == "=ACMGRSVTWYHKDBN" and '"%s"[mask]' % cc.CONS_IUPAC in raw             # the table of fifteen codes is stated
    for code, bases in zip("MRWSYKVHDBN", ("AC", "AG", "AT", "CG", "CT", "GT", "ACG", "ACT", "AGT", "CGT", "ACGT")):
        assert "%s: %s" % (bases, code) in raw and cc.CONS_IUPAC[sum(1 << "ACGT".index(b) for b in bases)] == code
    assert "MODULO 2^32" in raw and "in front of the view's first position" in raw                 # d's width and the limit are stated
    # the third-allele record is the dense planes' restatement of the engine's
    mine = open(os.path.join(side.CSRC, "brc_cons_core.h")).read()
    assert '#include "brc_dense_core.h"' in mine and "using brcdense::Rec;" in mine


def test_cons_uses_the_shared_scan_and_allocates_nothing():
    hip = open(os.path.join(side.CSRC, "brc_cons.hip")).read()
    assert '#include "brc_side_scan.h"' in hip and hip.count("brcside::scan(") == 2
    assert "hipMalloc" not in hip and "Synchronize" not in hip and "hipMemcpy" not in hip
    assert re.findall(r"hipMemsetAsync\(([\w.]+),", hip) == ["status", "counts", "off", "J.head", "J.diff", "J.run"]


def test_cons_library_has_a_kernel_object_of_its_own():
    from bam_readcount_amd import capi
    h = capi.kernel_object_hash(_lib())
    assert h is not None and re.fullmatch(r"[0-9a-f]{16}", h)
    assert h not in [capi.kernel_object_hash(p) for p in [None, capi.INFLATE_LIB, capi.DEFLATE_LIB] + [side._lib(r) for r in side.ROWS]]
    assert capi.kernel_object_hash(tc.cons_sim_lib()) is None
    blob = open(_lib(), "rb").read()
    for k in KERNELS:
        assert k.encode() in blob, k


def test_engine_and_sibling_kernel_objects_are_unchanged():
    """the engine's stamp is the committed one, and so are the siblings': none of their sources, nor a header they are built from, was
    touched"""
    side.check_engine_stamps()
    from bam_readcount_amd import capi
    prof = lambda name: json.load(open(os.path.join(side.ROOT, "profiles", name)))
    assert capi.kernel_object_hash(capi.DENSE_LIB) == prof("panel_bench.json")["dense_kernel_object_sha256_16"] == "0728c62aa99b7ee1"
    assert capi.kernel_object_hash(capi.INDELS_LIB) == prof("inorm_bench.json")["indels_kernel_object_sha256_16"] == "fee860b3aa70b55c"
    assert capi.kernel_object_hash(capi.IVET_LIB) == prof("ivet_bench.json")["ivet_kernel_object_sha256_16"] == "bcc67358ff5bed76"
    assert capi.kernel_object_hash(capi.INORM_LIB) == prof("inorm_bench.json")["inorm_kernel_object_sha256_16"] == "303df97f40a75dc6"
    assert capi.kernel_object_hash(capi.SELECT_LIB) == "878f5677d7083f27"
    assert capi.kernel_object_hash(capi.VET_LIB) == "8f54c7ace8dd5fad"
    assert capi.kernel_object_hash(capi.JOIN_LIB) == prof("join_bench.json")["join_kernel_object_sha256_16"] == "313675239df17673"


def test_the_product_and_every_sibling_neither_link_nor_load_the_cons_library():
    from bam_readcount_amd import capi
    others = [capi.PRODUCT_LIB, os.path.join(side.CSRC, "libbrc_hip_testknobs.so"), os.path.join(side.CSRC, "bam-readcount"), capi.INFLATE_LIB, capi.DEFLATE_LIB]
    for lib in others + [side._lib(r) for r in side.ROWS]:
        needed = subprocess.run(["readelf", "-d", lib], stdout=subprocess.PIPE, check=True).stdout.decode()
        assert "brc_cons" not in needed, lib
        assert b"brc_cons" not in open(lib, "rb").read(), lib           # (no dlopen by name, no symbol looked up)
    needed = subprocess.run(["readelf", "-d", _lib()], stdout=subprocess.PIPE, check=True).stdout.decode()
    assert "libbrc_" not in needed.replace("libbrc_cons_hip.so", "")
    assert not [s for s in side._undefined(_lib()) if s.startswith("brc_")]


def test_the_cons_sources_use_no_inline_assembly_and_the_siblings_flags():
    for f in ("brc_cons.hip", "brc_cons_core.h") + side.SHARED + ("brc_side_scan.h",):
        src = open(os.path.join(side.CSRC, f)).read()
        assert "asm" not in src and "brc_core.h" not in src and "brc_host.h" not in src, f
    core = open(os.path.join(side.CSRC, "brc_cons_core.h")).read()
    assert re.findall(r'#\s*include\s+"(brc_\w+_core\.h)"', core) == ["brc_dense_core.h"]
    cmd = subprocess.run(["make", "-n", "-C", side.CSRC, "-W", "brc_cons.hip", "brc_cons.o"], stdout=subprocess.PIPE, check=True).stdout.decode()
    assert "-c brc_cons.hip" in cmd
    assert "-ffp-contract=off" in cmd and "-O3" in cmd and "-std=c++17" in cmd and "fast-math" not in cmd and "-Ofast" not in cmd
    sib = subprocess.run(["make", "-n", "-C", side.CSRC, "-W", "brc_select.hip", "brc_select.o"], stdout=subprocess.PIPE, check=True).stdout.decode()
    assert cmd.replace("cons", "X") == sib.replace("select", "X")        # the side libraries' compile line, word for word
    mk = open(os.path.join(side.CSRC, "Makefile")).read()
    so = "libbrc_cons_hip.so"
    assert so in mk[mk.index("all:"):mk.index("\n", mk.index("all:"))] and so in mk[mk.index("clean:"):]
    assert re.search(r"^EXTRA_SIDE = cons$", mk, flags=re.M) and "cons" not in re.search(r"^SIDE = (.*)$", mk, flags=re.M).group(1).split()


def test_package_tensors_and_consensus_import_without_torch():
    code = ("import sys; sys.path.insert(0, %r); import bam_readcount_amd; from bam_readcount_amd import capi, tensors, consensus; "
            "o = consensus.Cons(%r); assert o.kind() == 'sim' and callable(tensors.consensus); "
            "assert 'torch' not in sys.modules; assert 'consensus' in bam_readcount_amd.__doc__ and bam_readcount_amd.consensus is consensus"
            % (side.ROOT, tc.cons_sim_lib()))
    subprocess.check_call([sys.executable, "-c", code])


def test_cons_library_refuses_to_exist_without_a_device_or_a_build():
    from bam_readcount_amd import capi, consensus as cc
    with pytest.raises(capi.BrcError):
        cc.Cons(os.path.join(side.CSRC, "no_such_library.so"))
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(capi.BrcError) as ei:
            cc.Cons()
        assert ei.value.rc == capi.E_NODEVICE


@pytest.mark.parametrize("build", ["sim", pytest.param("hip", marks=pytest.mark.gpu)])
def test_handle_lifecycle(build):
    """test_abi_side.test_handle_lifecycle's body over this library: the shared lifecycle behind the five common calls; no view, no data"""
    from bam_readcount_amd import capi, consensus as cc
    o = cc.Cons(tc.cons_sim_lib() if build == "sim" else None)
    call = lambda suffix: getattr(o.lib, "brc_cons_%s" % suffix)
    zeros = dict(kernel_s=0.0, bytes_read=0, bytes_written=0)
    assert o.kind() == ("sim" if build == "sim" else "hip-gfx950")
    assert o.last_timing() == zeros and call("last_error")(o.h) == b""
    assert o.call_raw(None, None, None, None, 0, 1, 1) == capi.E_ARG
    assert call("last_error")(o.h) != b""
    assert o.last_timing() == zeros
    call("destroy")(None)
    assert call("last_error")(None) == b""
    k = C.c_double(7.0); r = C.c_uint64(7); w = C.c_uint64(7)
    call("last_timing")(None, C.byref(k), C.byref(r), C.byref(w))
    assert (k.value, r.value, w.value) == (7.0, 7, 7)
    call("last_timing")(o.h, None, None, None)
    h = C.c_void_p()
    assert call("create")(-1, C.byref(h)) == (capi.E_ARG if build == "sim" else capi.E_NODEVICE) and not h
    assert call("create")(0, None) == capi.E_ARG
    if build == "hip":
        import torch
        h = C.c_void_p()
        assert call("create")(torch.cuda.device_count(), C.byref(h)) == capi.E_NODEVICE and not h
    for _ in range(20):
        h = C.c_void_p()
        assert call("create")(0, C.byref(h)) == 0 and h
        call("destroy")(h)
    o.close()
    assert o.h is None
