#!/usr/bin/env python3
"""Device code of two builds, function by function (host-side, no GPU).

For a change that must not alter what a kernel does by one instruction: build
the parent commit and the new tree with the same `make -C
raytracing-project_amd`, then

    tools/isa_compare.py PARENT/build NEW/build > profiles/<topic>/isa_compare.txt

For every object of the two directories that holds device code it takes the
gfx950 code object out of the .hip_fatbin section (llvm-objcopy,
clang-offload-bundler --unbundle), disassembles it (llvm-objdump -d), strips
addresses and encodings and compares the instruction text per function, by
mangled name; and per kernel the VGPR / SGPR / AGPR counts, the scratch and
LDS sizes and the spill counts of the code-object metadata (llvm-readelf
--notes).

The rule it holds the pair to:

  * functions built WITHOUT op counting (Cnt<false> and CntPlain: every kernel
    whose C template argument is false, every device function specialised on
    those types, and everything that has no such argument): the same set in
    both builds, each identical instruction for instruction with equal
    metadata.  The one line that may differ is the literal of an s_add_u32
    directly after an s_getpc_b64: the address of data that moved.
  * op-counting functions (C = true, Cnt<true>; launched under
    RT_FLAG_COUNT_OPS only): may move; each one that did is listed with its
    instruction count before and after and its metadata.
  * an object that only one build has (objects pair by file name) breaks the
    rule only if it holds device functions; a host-only one is noted.

Exit status 0 if the rule holds, 1 if not.  --strict holds the op-counting
functions to the first rule too.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
META = (("vgpr", ".vgpr_count"), ("sgpr", ".sgpr_count"), ("agpr", ".agpr_count"),
        ("scratch", ".private_segment_fixed_size"), ("lds", ".group_segment_fixed_size"),
        ("vgpr_spill", ".vgpr_spill_count"), ("sgpr_spill", ".sgpr_spill_count"))
# Position of the op-counting argument C in the trace kernels' template
# argument lists (csrc/device/rt_kernels.hpp); no other kernel has one.
COUNT_ARG = {"k_std": 3, "k_std_lean": 0, "k_std_secw": 0, "k_paper_primary": 2, "k_paper_primary_lean": 0}
CNT_TRUE = "3CntILb1EE"   # rtd::Cnt<true> in a device function's mangled name

LABEL = re.compile(r"^[0-9a-f]+ <(.+)>:$")
KERNEL = re.compile(r"_GLOBAL__N_1(\d+)")
TARG = re.compile(r"L([a-z])(n?\d+)E")


def counting(name):
    """Whether the function of this mangled name is an op-counting build."""
    if CNT_TRUE in name:
        return True
    m = KERNEL.search(name)
    if not m:
        return False
    base = name[m.end():m.end() + int(m.group(1))]
    rest = name[m.end() + int(m.group(1)):]
    if base not in COUNT_ARG or not rest.startswith("I"):
        return False
    args, pos = [], 1
    while True:
        a = TARG.match(rest, pos)
        if not a:
            break
        args.append(a.group(2))
        pos = a.end()
    return len(args) > COUNT_ARG[base] and args[COUNT_ARG[base]] == "1"


def run(*cmd):
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True).stdout


def code_object(obj, tmp):
    """The gfx950 code object of a host object's .hip_fatbin, or None."""
    fat = os.path.join(tmp, "fatbin")
    co = os.path.join(tmp, "co")
    for p in (fat, co):
        if os.path.exists(p):
            os.remove(p)
    try:
        run(os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", obj)
    except subprocess.CalledProcessError:
        return None   # no such section: a host-only object
    if not os.path.exists(fat) or os.path.getsize(fat) == 0:
        return None
    bundler = os.path.join(LLVM, "clang-offload-bundler")
    if TARGET not in run(bundler, "--type=o", f"--input={fat}", "--list").split():
        return None
    run(bundler, "--type=o", f"--input={fat}", f"--targets={TARGET}", f"--output={co}", "--unbundle")
    return co if os.path.getsize(co) else None


def functions(co):
    """{mangled name: [instruction text]} with addresses and encodings stripped."""
    out, cur = {}, None
    for line in run(os.path.join(LLVM, "llvm-objdump"), "-d", co).splitlines():
        m = LABEL.match(line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None or not line.startswith("\t"):
            continue
        text = " ".join(line.split("//")[0].split())
        if text:
            cur.append(text)
    return out


def metadata(co):
    """{kernel's mangled name: {figure: value}} from the code-object notes."""
    out, cur = {}, None
    for line in run(os.path.join(LLVM, "llvm-readelf"), "--notes", co).splitlines():
        m = re.match(r"^  (- | {2})(\.\w+):\s*(\S*)", line)
        if not m:
            continue
        if m.group(1) == "- ":
            cur = {}
        if cur is None:
            continue
        if m.group(2) == ".name":
            out[m.group(3)] = cur
        cur[m.group(2)] = m.group(3)
    return {k: {short: v.get(key, "-") for short, key in META} for k, v in out.items()}


def differing(a, b):
    """Lines at which two instruction lists differ, and how many of them the
    rule tolerates (None: the lists differ in length)."""
    if len(a) != len(b):
        return None, 0
    diff = [i for i in range(len(a)) if a[i] != b[i]]
    ok = 0
    for i in diff:
        if (i > 0 and a[i - 1].startswith("s_getpc_b64") and b[i - 1] == a[i - 1]
                and a[i].startswith("s_add_u32 ") and b[i].startswith("s_add_u32 ")
                and a[i].rsplit(",", 1)[0] == b[i].rsplit(",", 1)[0]):
            ok += 1
    return diff, ok


def fmt_meta(m):
    return " ".join(f"{k}={v}" for k, v in m.items()) if m else "(device function: no metadata)"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("parent", help="build directory of the parent commit")
    ap.add_argument("new", help="build directory of the new tree")
    ap.add_argument("--strict", action="store_true", help="hold the op-counting functions to identity too")
    a = ap.parse_args()

    names = sorted(f for f in set(os.listdir(a.parent)) | set(os.listdir(a.new)) if f.endswith(".o"))
    broken, moved = [], []
    tot = {"fn": 0, "same": 0, "tol": 0, "kern": 0, "cnt": 0, "cnt_moved": 0}
    print("Device code, parent build against new build: per object of build/ the gfx950 code object of .hip_fatbin")
    print("(clang-offload-bundler --unbundle), llvm-objdump -d, instruction text per function with addresses and")
    print("encodings stripped, compared by mangled name; per kernel .vgpr_count, .sgpr_count, .agpr_count,")
    print(".private_segment_fixed_size (scratch), .group_segment_fixed_size (LDS), .vgpr_spill_count and")
    print(".sgpr_spill_count of the code-object metadata.  plain: built without op counting; counting: C = true / Cnt<true>.")
    print()
    with tempfile.TemporaryDirectory() as tp, tempfile.TemporaryDirectory() as tn:
        for name in names:
            po, no = os.path.join(a.parent, name), os.path.join(a.new, name)
            if not (os.path.exists(po) and os.path.exists(no)):
                # an object of one build only breaks the rule only if it holds device functions
                side, only, tmp = ("parent", po, tp) if os.path.exists(po) else ("new", no, tn)
                co = code_object(only, tmp)
                n_fn = len(functions(co)) if co else 0
                print(f"{name}: only in the {side} build, " + (f"with {n_fn} device functions" if n_fn else "no device code"))
                if n_fn:
                    broken.append(f"{name}: an object with device functions is missing from one build")
                continue
            pc, nc = code_object(po, tp), code_object(no, tn)
            if pc is None and nc is None:
                print(f"{name}: no device code in either build")
                continue
            if pc is None or nc is None:
                print(f"{name}: device code only in the {'parent' if pc else 'new'} build")
                broken.append(f"{name}: device code in one build only")
                continue
            pf, nf, pm, nm = functions(pc), functions(nc), metadata(pc), metadata(nc)
            only_p, only_n = sorted(set(pf) - set(nf)), sorted(set(nf) - set(pf))
            for n_ in only_p:
                broken.append(f"{name}: {n_} only in the parent build")
            for n_ in only_n:
                broken.append(f"{name}: {n_} only in the new build")
            plain_n = plain_same = cnt_n = cnt_same = tol = meta_eq = 0
            for fn in sorted(set(pf) & set(nf)):
                is_cnt = counting(fn)
                diff, ok = differing(pf[fn], nf[fn])
                same_text = diff is not None and len(diff) == ok
                same_meta = pm.get(fn) == nm.get(fn)
                tol += ok if same_text else 0
                meta_eq += 1 if (fn in pm and same_meta) else 0
                if is_cnt:
                    cnt_n += 1
                    cnt_same += 1 if (same_text and same_meta) else 0
                else:
                    plain_n += 1
                    plain_same += 1 if (same_text and same_meta) else 0
                if same_text and same_meta:
                    continue
                what = (f"{len(pf[fn])} -> {len(nf[fn])} instructions"
                        + ("" if diff is None else f", {len(diff) - ok} lines differ (first at instruction {next(i for i in diff)})")
                        + f"; parent {fmt_meta(pm.get(fn))}; new {fmt_meta(nm.get(fn))}")
                if is_cnt and not a.strict:
                    moved.append(f"{name}: {fn}\n    {what}")
                else:
                    broken.append(f"{name}: {fn}\n    {what}")
            print(f"{name}: {len(pf)} / {len(nf)} functions (parent / new); plain {plain_same} of {plain_n} identical, "
                  f"counting {cnt_same} of {cnt_n} identical; {len(set(pm) & set(nm))} kernels in the metadata, "
                  f"{meta_eq} with equal figures; {tol} pc-relative literals tolerated")
            tot["fn"] += plain_n
            tot["same"] += plain_same
            tot["tol"] += tol
            tot["kern"] += len(set(pm) & set(nm))
            tot["cnt"] += cnt_n
            tot["cnt_moved"] += cnt_n - cnt_same
    print(f"total: plain {tot['same']} of {tot['fn']} functions identical; counting {tot['cnt'] - tot['cnt_moved']} of "
          f"{tot['cnt']} identical; {tot['kern']} kernels compared in the metadata; {tot['tol']} pc-relative literals tolerated")
    print()
    print(f"op-counting functions that moved: {len(moved)}")
    for m in moved:
        print("  " + m)
    print()
    if broken:
        print(f"RULE BROKEN: {len(broken)}")
        for b in broken:
            print("  " + b)
        return 1
    print("RULE HOLDS: the same set of functions in every object; every function built without op counting identical")
    print("instruction for instruction (but for the tolerated literals) with equal register, scratch, LDS and spill figures.")
    return 0


if __name__ == "__main__":
    sys.exit(main())
