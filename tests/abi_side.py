"""What tests/test_abi_<library>.py, tests/test_abi_side.py and tests/route.py share: one table of the side libraries, one row per
library, the checks over a row, and the one reader of a header's structs and constants.  "The others" of a row are the engine, the
inflater, the deflater and every other row, so a new library is a new row and nobody's list of siblings
(test_abi_side.test_the_table_is_every_side_library holds the table to the build rule, the CPU builds and the binding).  Not a test
module."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

from conftest import ROOT

CSRC = os.path.join(ROOT, "bam_readcount_amd", "csrc")
SHARED = ("brc_side_hip.h",)          # the host side the .hip files of the table share

# name: the X of brc_X_*, include/brc_X.h, libbrc_X_hip.so, tests/sim_X/libbrc_X_sim.so, brc_X.hip, brc_X_core.h and capi.X_EXPORTS / X_LIB
# cls / tensors: the binding class and the function of bam_readcount_amd.tensors over it
# kernels: what the code object must hold;  strict: the sources do not even name an engine header
# null_call: the library's one real call with a NULL view, through the binding
# uses: rows whose header and core this library is built from by design (brc_ivet.h includes brc_vet.h): its mangled names spell theirs
ROWS = [
    dict(name="dense", cls="Dense", tensors="region", kernels=("k_dense_planes", "k_dense_overlay"), strict=False,
         null_call=lambda o: o.expand_raw(None, 0, 1, 1)),
    dict(name="indels", cls="Indels", tensors="indels", kernels=("k_count", "k_place", "k_rank", "k_emit", "k_scan_reduce", "k_scan_parts", "k_scan_apply"),
         strict=False, null_call=lambda o: o.gather_raw(None, 0, 1)),
    dict(name="panel", cls="Panel", tensors="sites", kernels=("k_panel_planes", "k_panel_overlay"), strict=False,
         null_call=lambda o: o.gather_raw(None, None, 1, 1)),
    dict(name="select", cls="Select", tensors="select", kernels=("k_select_link", "k_select_flag", "k_select_why", "k_select_parts", "k_select_emit"),
         strict=True, null_call=lambda o: o.sites_raw(None, None, None, 0, 1)),
    dict(name="bins", cls="Bins", tensors="bins", kernels=("k_bins_clear", "k_bins_edges", "k_bins_planes", "k_bins_records", "k_bins_indels"),
         strict=True, null_call=lambda o: o.reduce_raw(None, None, None, 0, 1, 1)),
    dict(name="runs", cls="Runs", tensors="runs", kernels=("k_runs_class", "k_runs_parts", "k_runs_emit"), strict=True,
         null_call=lambda o: o.find_raw(None, None, None, 0, 1)),
    dict(name="vet", cls="Vet", tensors="vet", kernels=("k_vet_link", "k_vet_sites"), strict=True,
         null_call=lambda o: o.sites_raw(None, None, None, None, None, 1, 1)),
    dict(name="ivet", cls="IVet", tensors="vet_indels", kernels=("k_ivet_link", "k_ivet_records"), strict=True, uses=("vet",),
         null_call=lambda o: o.records_raw(None, None, None, None, None, None, 1, 1)),
    dict(name="inorm", cls="INorm", tensors="normalize_indels",
         kernels=("k_inorm_shift", "k_inorm_place", "k_inorm_rank", "k_inorm_heads", "k_inorm_merge", "k_side_scan_reduce", "k_side_scan_parts", "k_side_scan_apply"),
         strict=True, null_call=lambda o: o.table_raw(None, None, None, 0, 1)),
    dict(name="join", cls="Join", tensors="join",
         kernels=("k_join_planes", "k_join_xagg", "k_join_slots", "k_join_reads", "k_join_ref", "k_side_scan_reduce", "k_side_scan_parts", "k_side_scan_apply"),
         strict=True, null_call=lambda o: o.views_raw(None, 0, 1, 1, K=1)),
]
SIDE = {r["name"]: r for r in ROWS}


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def _exports(row):
    from bam_readcount_amd import capi
    return getattr(capi, row["name"].upper() + "_EXPORTS")


def _lib(row):
    from bam_readcount_amd import capi
    return getattr(capi, row["name"].upper() + "_LIB")


def _sim_dir(row):
    return os.path.join(ROOT, "tests", "sim_" + row["name"])


def sim_lib(row):
    """the row's CPU build, built"""
    subprocess.check_call(["make", "-s", "-C", _sim_dir(row)], stderr=subprocess.DEVNULL)
    return os.path.join(_sim_dir(row), "libbrc_%s_sim.so" % row["name"])


def sim_checker(row):
    """the row's stand-alone driver of its CPU build under the host sanitizers (tests/sim_<name>/<name>_check_asan), built"""
    subprocess.check_call(["make", "-s", "-C", _sim_dir(row), "asan"], stderr=subprocess.DEVNULL)
    return os.path.join(_sim_dir(row), "%s_check_asan" % row["name"])


def sim_engine():
    """the engine's CPU build, built"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "sim")])
    return os.path.join(ROOT, "tests", "sim", "libbrc_sim.so")


def _siblings(row):
    return [r for r in ROWS if r is not row]


def _defined(lib, which="--defined-only"):
    syms = subprocess.run(["nm", "-D", which, lib], stdout=subprocess.PIPE, check=True).stdout.decode()
    return {l.split()[-1] for l in syms.splitlines()}


def _undefined(lib):
    return _defined(lib, "--undefined-only")


# ------------------------------------------------------------------------------------------------ a header's structs and constants

_CTYPE = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "uint64_t": C.c_uint64, "int64_t": C.c_int64, "float": C.c_float}


def members(h, struct, types=False):
    """the members of a struct of the header text, in order: their names, or with types (name, the ctypes type a binding gives it —
    c_void_p for every pointer —, whether it is an array)"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), h, flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        if not decl.strip():
            continue
        base, rest = re.match(r"((?:const\s+)?\w+)\s*(.*)", decl.strip(), flags=re.S).groups()
        for n in rest.split(","):
            n = n.strip()
            name = n.lstrip("* ").split("[")[0]
            out.append((name, C.c_void_p if n.startswith("*") else _CTYPE[base.replace("const", "").strip()], "[" in n) if types else name)
    return out


def define(h, name):
    """the value of an integer constant of the header text"""
    return int(re.search(r"#define\s+%s\s+(\d+)u?\b" % name, h).group(1))


def c_layout(tmp_path, header, struct, names):
    """[sizeof, offsetof of every name] from a C compile of the header under include/"""
    src = '#include <stddef.h>\n#include <stdio.h>\n#include "%s"\nint main(void) { printf("%%zu", sizeof(%s));\n' % (header, struct)
    src += "".join('printf(" %%zu", offsetof(%s, %s));\n' % (struct, n) for n in names) + "return 0; }\n"
    exe = str(tmp_path / (struct + "_layout_check"))
    subprocess.run(["gcc", "-x", "c", "-std=c99", "-I", os.path.join(ROOT, "include"), "-", "-o", exe], input=src.encode(), check=True)
    return [int(x) for x in subprocess.run([exe], stdout=subprocess.PIPE, check=True).stdout.split()]


def check_struct(tmp_path, header, struct, T, types=True, array_len=None):
    """the binding's struct T is the header's: the members' names in order, their types, and the layout a C compiler gives them"""
    names = [n for n, _ in T._fields_]
    assert members(_header(header), struct) == names, struct
    if types:
        for (n, ct, arr), (_, bt) in zip(members(_header(header), struct, types=True), T._fields_):
            assert bt is ct if not arr else (bt._type_ is ct and bt._length_ == array_len), (struct, n)
    assert c_layout(tmp_path, header, struct, names) == [C.sizeof(T)] + [getattr(T, n).offset for n in names], struct


def check_exports(row):
    from bam_readcount_amd import capi
    name = row["name"]
    declared = set(re.findall(r"\b(brc_%s_\w+)\s*\(" % name, _header("brc_%s.h" % name)))
    assert declared == set(_exports(row))
    others = set(capi.EXPORTS) | set(capi.INFLATE_EXPORTS) | set(capi.DEFLATE_EXPORTS)
    for r in _siblings(row):
        others |= set(_exports(r))
    assert not set(_exports(row)) & others
    assert os.path.exists(_lib(row)), "libbrc_%s_hip.so is not built (make -C bam_readcount_amd/csrc)" % name
    for lib in (_lib(row), sim_lib(row)):
        assert {s for s in _defined(lib) if s.startswith("brc_")} == set(_exports(row)), lib
    # the other headers do not know the library
    for h in ["brc.h", "brc_inflate.h", "brc_deflate.h"] + ["brc_%s.h" % r["name"] for r in _siblings(row)]:
        assert not re.search(r"\bbrc_%s_\w+\s*\(" % name, _header(h)), h


def check_seam(call, exported_by_the_engines=False):
    """the engine's side of a seam is one call of its own header"""
    from bam_readcount_amd import capi
    assert call in capi.EXPORTS and re.search(r"\b%s\s*\(" % call, _header("brc.h"))
    if exported_by_the_engines:
        for lib in (capi.PRODUCT_LIB, os.path.join(CSRC, "libbrc_hip_testknobs.so"), sim_engine()):
            assert call in _defined(lib), lib


def check_panel_status_bits():
    from bam_readcount_amd import capi
    h = _header("brc_panel.h")
    assert (define(h, "BRC_PANEL_OUT_OF_RANGE"), define(h, "BRC_PANEL_NOT_ASCENDING")) == (capi.PANEL_OUT_OF_RANGE, capi.PANEL_NOT_ASCENDING) == (1, 2)


def check_view_struct(tmp_path):
    """capi.DeviceView against the C struct, field by field (offsets from a compile of the header)."""
    from bam_readcount_amd import capi
    check_struct(tmp_path, "brc.h", "brc_device_view", capi.DeviceView, types=False)
    h = _header("brc.h")
    assert (capi.MEM_DEVICE, capi.MEM_HOST) == (define(h, "BRC_MEM_DEVICE"), define(h, "BRC_MEM_HOST"))


def check_indels_struct(tmp_path):
    """capi.DeviceIndels against the C struct, field by field (offsets from a compile of the header)."""
    from bam_readcount_amd import capi
    check_struct(tmp_path, "brc.h", "brc_device_indels", capi.DeviceIndels, types=False)
    # the record layout the header documents is the engine's
    core = open(os.path.join(CSRC, "brc_core.h")).read()
    assert "struct IndelOut { int32_t pos, lib, len; uint32_t rep_read; int32_t rep_qpos; uint32_t i[NI]; float f[NF]; };" in core


def check_select_params(tmp_path):
    from bam_readcount_amd import capi
    h = _header("brc_select.h")
    check_struct(tmp_path, "brc_select.h", "brc_select_params", capi.SelectParams)
    assert C.sizeof(capi.SelectParams) == 48 and capi.SelectParams.flags.offset == 8 and capi.SelectParams.ctl_frac_den.offset == 40
    assert (define(h, "BRC_SELECT_SNV"), define(h, "BRC_SELECT_INDEL")) == (capi.SELECT_SNV, capi.SELECT_INDEL) == (1, 2)
    assert (define(h, "BRC_ROLE_IGNORE"), define(h, "BRC_ROLE_CASE"), define(h, "BRC_ROLE_CONTROL")) == (capi.ROLE_IGNORE, capi.ROLE_CASE, capi.ROLE_CONTROL) == (0, 1, 2)
    assert define(h, "BRC_SELECT_MAX_LIB") == capi.SELECT_MAX_LIB == 254
    bits = tuple(define(h, "BRC_WHY_" + n) for n in ("A", "C", "G", "T", "INS", "DEL"))
    assert bits == (capi.WHY_A, capi.WHY_C, capi.WHY_G, capi.WHY_T, capi.WHY_INS, capi.WHY_DEL) == (1, 2, 4, 8, 16, 32)
    assert "not compared" in open(os.path.join(ROOT, "include", "brc_select.h")).read().lower()      # the allele-blind veto is stated


def check_bins_params(tmp_path):
    from bam_readcount_amd import capi
    h = _header("brc_bins.h")
    check_struct(tmp_path, "brc_bins.h", "brc_bins_params", capi.BinsParams, array_len=capi.BINS_MAX_THR)
    P = capi.BinsParams
    assert C.sizeof(P) == 64 and (P.edges.offset, P.width.offset, P.n_bins.offset, P.n_thr.offset, P.n_hist.offset, P.thr.offset) == (0, 8, 16, 24, 28, 32)
    assert (define(h, "BRC_BINS_NSUM"), define(h, "BRC_BINS_MAX_THR"), define(h, "BRC_BINS_MAX_HIST"), define(h, "BRC_BINS_MAX_LIB")) == \
        (capi.BINS_NSUM, capi.BINS_MAX_THR, capi.BINS_MAX_HIST, capi.BINS_MAX_LIB) == (12, 8, 4096, 65535)
    names = ("DEPTH", "NCOL", "BUCKET", "NONREF", "INS", "DEL", "MAXDEPTH")
    assert tuple(define(h, "BRC_BINS_S_" + n) for n in names) == tuple(getattr(capi, "BINS_S_" + n) for n in names) == (0, 1, 2, 8, 9, 10, 11)
    assert (define(h, "BRC_BINS_DESCENDS"), define(h, "BRC_BINS_OUTSIDE")) == (capi.BINS_DESCENDS, capi.BINS_OUTSIDE) == (1, 2)


def check_kernel_object(row):
    from bam_readcount_amd import capi
    h = capi.kernel_object_hash(_lib(row))
    assert h is not None and re.fullmatch(r"[0-9a-f]{16}", h)
    assert h not in [capi.kernel_object_hash(p) for p in [None, capi.INFLATE_LIB, capi.DEFLATE_LIB] + [_lib(r) for r in _siblings(row)]]
    assert capi.kernel_object_hash(sim_lib(row)) is None
    blob = open(_lib(row), "rb").read()
    for k in row["kernels"]:
        assert k.encode() in blob, k


def check_engine_stamps():
    from bam_readcount_amd import capi
    j = json.load(open(os.path.join(ROOT, "profiles", "r06_traffic.json")))
    for cfg in ("wgs30x", "tumor200x"):
        stamp = j[cfg]["kernel_object_sha256_16"]
        assert capi.kernel_object_hash() == stamp == "b699f7e6f23ebb67"
        assert capi.kernel_object_hash(os.path.join(CSRC, "libbrc_hip_testknobs.so")) == stamp


def check_neither_links_nor_loads(row):
    from bam_readcount_amd import capi
    name = row["name"]
    others = [(p, ()) for p in (capi.PRODUCT_LIB, os.path.join(CSRC, "libbrc_hip_testknobs.so"), os.path.join(CSRC, "bam-readcount"))]
    for lib, uses in others + [(_lib(r), r.get("uses", ())) for r in _siblings(row)]:
        needed = subprocess.run(["readelf", "-d", lib], stdout=subprocess.PIPE, check=True).stdout.decode()
        assert "brc_" + name not in needed, lib
        blob = open(lib, "rb").read()
        assert b"libbrc_" + name.encode() not in blob, lib                                               # (no dlopen by name)
        if name in uses:
            # built from this library's header and core, so its mangled names spell brc_<name>: it still defines and looks up no call of it
            assert not [s for s in _defined(lib) | _undefined(lib) if s.startswith("brc_%s_" % name)], lib
        else:
            assert b"brc_" + name.encode() not in blob, lib                                              # (no symbol looked up)
    # ... and the library links nothing of the engine, nor of its siblings: the views are plain data
    needed = subprocess.run(["readelf", "-d", _lib(row)], stdout=subprocess.PIPE, check=True).stdout.decode()
    assert "libbrc_" not in needed.replace("libbrc_%s_hip.so" % name, "")
    assert not [s for s in _undefined(_lib(row)) if s.startswith("brc_")]


def check_sources_and_flags(row):
    name = row["name"]
    for f in ("brc_%s.hip" % name, "brc_%s_core.h" % name) + SHARED:
        src = open(os.path.join(CSRC, f)).read()
        assert "asm" not in src and not re.search(r"#\s*include[^\n]*brc_(core|host)\.h", src), f
        if row["strict"] or f in SHARED:
            assert "brc_core.h" not in src and "brc_host.h" not in src, f
    # the command line the object is really compiled with
    cmd = subprocess.run(["make", "-n", "-C", CSRC, "-W", "brc_%s.hip" % name, "brc_%s.o" % name], stdout=subprocess.PIPE, check=True).stdout.decode()
    assert "-c brc_%s.hip" % name in cmd
    assert "-ffp-contract=off" in cmd and "-O3" in cmd and "-std=c++17" in cmd and "fast-math" not in cmd and "-Ofast" not in cmd
    mk = open(os.path.join(CSRC, "Makefile")).read()
    so = "libbrc_%s_hip.so" % name
    assert so in mk[mk.index("all:"):mk.index("\n", mk.index("all:"))] and so in mk[mk.index("clean:"):]


def check_import_without_torch(row):
    """Importing the package, its tensors module and a binding must not import torch; the CPU route of bam_readcount_amd.tensors needs
    numpy alone."""
    code = ("import sys; sys.path.insert(0, %r); import bam_readcount_amd; from bam_readcount_amd import capi, tensors; "
            "o = capi.%s(%r); assert o.kind() == 'sim' and callable(tensors.%s); "
            "assert 'torch' not in sys.modules; assert 'tensors' in bam_readcount_amd.__doc__" % (ROOT, row["cls"], sim_lib(row), row["tensors"]))
    subprocess.check_call([sys.executable, "-c", code])


def check_one_hip_runtime():
    """A process that loads the HIP libraries first and imports torch afterwards must hold ONE HIP runtime (capi._load): with two, the
    second finds no GPU and a tensor can never meet a view.  (Checked on the process's own map; no GPU needed.  The GPU half:
    tests/test_tensors_gpu.py::test_engine_created_before_torch_is_imported.)"""
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


def check_refuses_to_exist(row):
    """A binding never substitutes: a missing library raises, and so does the hip library on a machine without a GPU."""
    from bam_readcount_amd import capi
    cls = getattr(capi, row["cls"])
    import pytest
    with pytest.raises(capi.BrcError):
        cls(os.path.join(CSRC, "no_such_library.so"))
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(capi.BrcError) as ei:
            cls()
        assert ei.value.rc == capi.E_NODEVICE
