#!/usr/bin/env python3
"""side_mutants.py — a mutation pass over the per-lane cores of the six newest side libraries (select, vet, ivet, inorm, runs, bins).

CPU ONLY.  This tool never touches a GPU: an edited core is built with g++ into tests/sim_* of a temporary copy of the tree and
nowhere else, hipcc is never invoked (the children's PATH starts with a directory whose `hipcc` refuses), no product library is
loaded (the test files run with -m "not gpu", which leaves only their [sim] route), and any --route but `sim` is refused before
anything is copied.  A value-only mutation of a GPU kernel once ended in a memory fault on the device (open item):
mutated kernels are not for shared GPUs.

The list (tools/side_mutants.json) holds one edit per entry: id, header (the core), old, new (old must occur exactly once in the
header), test (that library's test file) and equivalent (the argument from the header's contract why no allowed input can tell the
edit from the original, or "").  Its first entries are named edits written by hand; the others (those with a `where`) are
mechanical: one per comparison operator (loop bounds among them), per literal shift, per literal mask and per index with an offset
of one in the lane functions of the
six cores, made by --generate, which keeps the argument of every edit whose text did not change.  Per edit the tool copies the tree
without .git and build products (but with oracle/_ref as built) to a temporary directory, applies the edit there, runs the test file
and reports killed (with the first failing test), crashed (the edited build left its arrays or did not end: noticed) or survived.
At most min(8, CPUs) copies run at once.  A full pass takes a quarter of an hour on eight CPUs, so the tool is no test: pytest does
not collect it.

    python tools/side_mutants.py                         the whole list; exit status 1 if an edit that is not marked equivalent survives
    python tools/side_mutants.py vet.E1 runs.R4          some edits
    python tools/side_mutants.py --out profiles/side_mutants.json
    python tools/side_mutants.py --generate              after a core header changed: the mechanical edits anew
"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIST = os.path.join(ROOT, "tools", "side_mutants.json")
BUILT = shutil.ignore_patterns("*.so", "*.o", "*.a", "*.hsaco", "*.co", "*_check_asan", "__pycache__", "*.pyc", ".pytest_cache")


def skip(directory, names):
    """what a copy leaves out: .git, the recorded results and build products — but oracle/_ref, the reference-compiled checker, goes
    along as it is built (nothing of it is edited, and rebuilding it in every copy was most of an edit's fixed cost)"""
    rel = os.path.relpath(directory, ROOT)
    if rel == os.path.join("oracle", "_ref") or rel.startswith(os.path.join("oracle", "_ref") + os.sep):
        return set()
    out = set(BUILT(directory, names))
    if rel == ".":
        out |= {".git", "profiles", "build"} & set(names)
    if rel == os.path.join("bam_readcount_amd", "csrc"):
        out |= {"bam-readcount"} & set(names)
    if rel == os.path.join("tests", "sim"):
        out |= {"bam-readcount-sim"} & set(names)
    return out


REFUSING_HIPCC = "#!/bin/sh\necho 'side_mutants: hipcc is not to be invoked from a mutated copy' >&2\nexit 97\n"

# ------------------------------------------------------------------------------------------------ the mechanical part of the list

CORES = ("select", "vet", "ivet", "inorm", "runs", "bins")
LANE_FUNCTIONS = r"(\w*_lane|judge|bucket_side|control_vetoes|compare|chr|bin_of|case_ok|ctl_count_ok)"
SWAP = {"<": "<=", "<=": "<", ">": ">=", ">=": ">", "==": "!=", "!=": "=="}
COMPARISON = re.compile(r"(?<![<>=!\-+*/&|^%])(<=|>=|==|!=|<|>)(?![<>=])")
SHIFT = re.compile(r"(<<|>>) (\d+)u?\b")
MASK = re.compile(r"& (0x[0-9a-fA-F]+)u?\b")
INDEX = re.compile(r"\[([^\[\]]*?) ([-+]) 1u?\]")
# a loop over a fixed-size array (for (int f = 0; f < NI; ...)): one more turn is out of bounds by construction, not a value edit
FIXED_LOOP = re.compile(r"\s*<\s*(\(uint32_t\))?(NI|NF|NM|NVAL|NCOL|NB|NADD|4u|2|MAX_CUT|ROLE_WORDS|ON_WORDS|MAX_THR)\b")


def generate():
    """One edit per comparison operator (loop bounds included, but those over fixed-size arrays), per literal shift (one bit further),
    per literal mask (its top bit dropped) and per index of the form [e - 1] / [e + 1] (the offset dropped) in the lane functions of the six cores: id, header, old, new, test, where."""
    out = []
    for lib in CORES:
        header = "bam_readcount_amd/csrc/brc_%s_core.h" % lib
        text = open(os.path.join(ROOT, header)).read()
        lines = text.split("\n")
        i, count = 0, {"m": 0, "s": 0, "x": 0}
        while i < len(lines):
            m = re.match(r"^(BRCD_HD|inline)\s+[\w:<> \*&]+?\b" + LANE_FUNCTIONS + r"\(", lines[i])
            if not m or (lines[i].rstrip().endswith(";") and "{" not in lines[i]):
                i += 1
                continue
            j = i
            if not (lines[i].rstrip().endswith("}") and lines[i].count("{") == lines[i].count("}")):
                while lines[j] != "}":
                    j += 1
            for k in range(i, j + 1):
                ln = lines[k]
                code = ln.split("//")[0]
                if code.lstrip().startswith("#") or "static_assert" in code:
                    continue
                start = (code.index("{") if "{" in code else len(code)) if k == i else 0
                found = []
                for mm in COMPARISON.finditer(code):
                    if re.search(r"for \((int|uint32_t) \w+ = 0u?; \w+ $", code[:mm.start()]) and FIXED_LOOP.match(code[mm.start():]):
                        continue
                    found.append(("m", mm.start(), mm.end(), SWAP[mm.group(1)], "%s -> %s" % (mm.group(1), SWAP[mm.group(1)])))
                for mm in SHIFT.finditer(code):
                    new = "%s %d" % (mm.group(1), int(mm.group(2)) + 1)
                    found.append(("s", mm.start(), mm.start() + len(mm.group(1)) + 1 + len(mm.group(2)), new, "%s %s -> %s" % (mm.group(1), mm.group(2), new)))
                for mm in MASK.finditer(code):
                    new = "& 0x%x" % (int(mm.group(1), 16) >> 1)
                    found.append(("s", mm.start(), mm.start() + 2 + len(mm.group(1)), new, "& %s -> %s" % (mm.group(1), new)))
                for mm in INDEX.finditer(code):
                    found.append(("x", mm.start(), mm.end(), "[%s]" % mm.group(1), "%s -> [%s]" % (mm.group(0), mm.group(1))))
                for kind, a, b, put, what in sorted(found, key=lambda f: f[1]):
                    if a < start:
                        continue
                    old, new, up = ln + "\n", ln[:a] + put + ln[b:] + "\n", k
                    while text.count(old) != 1 and up > 0:
                        up -= 1
                        old, new = lines[up] + "\n" + old, lines[up] + "\n" + new
                    count[kind] += 1
                    out.append(dict(id="%s.%s%03d" % (lib, kind, count[kind]), header=header, old=old, new=new, test="tests/test_%s.py" % lib, equivalent="",
                                    where="%s, line %d, column %d: %s" % (m.group(2), k + 1, a + 1, what)))
            i = j + 1
    return out


def regenerate(path):
    """the list's named edits as they are, its mechanical ones made anew; an argument stays with the edit whose text is unchanged"""
    edits = json.load(open(path))
    kept = {(e["header"], e["old"], e["new"]): e["equivalent"] for e in edits}
    named = [e for e in edits if "where" not in e]
    fresh = generate()
    for e in fresh:
        e["equivalent"] = kept.get((e["header"], e["old"], e["new"]), "")
    with open(path, "w") as f:
        json.dump(named + fresh, f, indent=1)
        f.write("\n")
    print("%d named edits, %d mechanical ones" % (len(named), len(fresh)))


def run_edit(edit, tmp_root, shim, keep, limit):
    d = os.path.join(tmp_root, edit["id"])
    shutil.copytree(ROOT, d, ignore=skip, symlinks=True)
    path = os.path.join(d, edit["header"])
    text = open(path).read()
    res = dict(id=edit["id"], equivalent=bool(edit["equivalent"]), test=None)
    if text.count(edit["old"]) != 1:
        res["verdict"] = "bad-pattern: old text occurs %d times" % text.count(edit["old"])
        return res
    open(path, "w").write(text.replace(edit["old"], edit["new"]))
    env = dict(os.environ, CXX="g++", PATH=shim + os.pathsep + os.environ.get("PATH", ""), PYTHONDONTWRITEBYTECODE="1")
    try:
        p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "not gpu", "-p", "no:cacheprovider", edit["test"]], cwd=d, env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=limit)
    except subprocess.TimeoutExpired:                       # (an edited loop that never ends: noticed, as a crash is)
        res["verdict"] = "crashed: no end after %d s" % limit
        if not keep:
            shutil.rmtree(d, ignore_errors=True)
        return res
    out = p.stdout.decode(errors="replace").splitlines()
    first = next((l.split(" - ")[0].split(None, 1)[1] for l in out if l.startswith(("FAILED ", "ERROR ")) and len(l.split()) > 1), None)
    if p.returncode == 0:
        res["verdict"] = "survived"
    elif p.returncode == 1 and first:
        res["verdict"], res["test"] = "killed", first
    else:
        res["verdict"] = "crashed: pytest ended with status %d" % p.returncode
    if not keep:
        shutil.rmtree(d, ignore_errors=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("ids", nargs="*", help="edits to run (default: the whole list)")
    ap.add_argument("--list", default=LIST)
    ap.add_argument("--route", default="sim", help="only `sim`, the CPU build, is accepted")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--out", help="write the result as JSON: id, verdict, the killing test")
    ap.add_argument("--timeout", type=int, default=300, help="seconds one edit's test file may take (the unedited files take under a minute)")
    ap.add_argument("--generate", action="store_true", help="write the mechanical edits of the list anew from the core headers, and stop")
    ap.add_argument("--keep", action="store_true", help="leave the mutated copies where they are")
    a = ap.parse_args()
    if a.route != "sim":
        sys.exit("side_mutants: route %r refused: mutated cores run on the CPU build only" % a.route)
    if a.generate:
        regenerate(a.list)
        return 0
    edits = json.load(open(a.list))
    ids = [e["id"] for e in edits]
    assert len(set(ids)) == len(ids), "two edits of one id"
    unknown = [i for i in a.ids if i not in ids]
    if unknown:
        sys.exit("side_mutants: no such edit: %s" % " ".join(unknown))
    edits = [e for e in edits if not a.ids or e["id"] in a.ids]
    jobs = max(1, min(8, os.cpu_count() or 1, a.jobs))
    tmp_root = tempfile.mkdtemp(prefix="side_mutants_")
    shim = os.path.join(tmp_root, "_shim")
    os.mkdir(shim)
    with open(os.path.join(shim, "hipcc"), "w") as f:
        f.write(REFUSING_HIPCC)
    os.chmod(os.path.join(shim, "hipcc"), 0o755)
    results = []
    with ThreadPoolExecutor(jobs) as ex:
        for r in ex.map(lambda e: run_edit(e, tmp_root, shim, a.keep, a.timeout), edits):
            print("%-12s %-10s %s%s" % (r["id"], r["verdict"].split(":")[0], r["test"] or "", "  (equivalent)" if r["equivalent"] else ""), flush=True)
            results.append(r)
    if not a.keep:
        shutil.rmtree(tmp_root, ignore_errors=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
    # an edit whose run crashed (the mutated CPU build left its arrays) did not go unnoticed: it is reported, and is no survivor
    # ... and an edit marked equivalent that a test kills has a wrong argument
    bad = [r["id"] for r in results if r["verdict"].startswith("bad-pattern") or (r["verdict"] == "survived") != r["equivalent"]]
    n = dict(killed=sum(r["verdict"] == "killed" for r in results), survived=sum(r["verdict"] == "survived" for r in results),
             crashed=sum(r["verdict"].startswith("crashed") for r in results))
    print("%d edits: %d killed, %d crashed, %d survived (%d of them marked equivalent)" % (len(results), n["killed"], n["crashed"], n["survived"],
                                                                                          sum(r["verdict"] == "survived" and r["equivalent"] for r in results)))
    if bad:
        print("survivors that are not marked equivalent, equivalents that were killed, edits that did not apply: " + " ".join(bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
