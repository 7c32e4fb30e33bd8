#!/usr/bin/env python3
"""SGPR-spill traffic of one kernel's ISA, per asm loop and per spill lane
(host-side, no GPU).

When a kernel needs more SGPRs than it has, the compiler parks the excess in
lanes of a reserved VGPR: `v_writelane_b32 vS, sN, imm` stores, and
`v_readlane_b32 sN, vS, imm` fetches.  Both are VALU issue slots that compute
nothing.  This tool compiles rt_kernels_f64.hip like tools/isa_regions.py
(line tables, the product's flags otherwise), takes the kernel whose mangled
name contains KERNEL and reports

  * per asm loop (the compiler's `Loop Header` / `in Loop: Header=... Depth=...`
    block comments; "-" is code outside every loop): static VALU count, spill
    lane writes and reads, and the device functions the loop's `.loc` lines
    fall in (innermost inlined function, with its line range);
  * per spill lane: every write and read with its loop and source line.

A spill VGPR is one that is the destination of a v_writelane with an immediate
lane; the rdlane_f / wave_max_u32 reads of ordinary values never write lanes.
Static counts: each instruction once, whatever its trip count.

Usage: tools/isa_spill.py [KERNEL] [--asm FILE] [--keep-asm FILE] [--lanes] [extra hipcc flags via ISA_FLAGS]
"""
import argparse
import collections
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_regions import PKG, classify, func_starts, region   # noqa: E402

VALU = ("fp64", "f32", "mov", "cndmask", "cmp", "lane", "int")
WR = re.compile(r"^\s*v_writelane_b32\s+(v\d+),\s*(s\d+|vcc_lo|vcc_hi|exec_lo|exec_hi),\s*(\d+)\b")
RD = re.compile(r"^\s*v_readlane_b32\s+(s\d+|vcc_lo|vcc_hi|exec_lo|exec_hi),\s*(v\d+),\s*(\d+)\b")
BLOCK = re.compile(r"^(?:\.L(BB\d+_\d+):|; %bb\.\d+:)")
IN_LOOP = re.compile(r";\s+in Loop: Header=(BB\d+_\d+) Depth=(\d+)")
THIS_LOOP = re.compile(r";\s*=>\s*This (?:Inner )?Loop Header: Depth=(\d+)")
PARENT = re.compile(r";\s+Parent Loop (BB\d+_\d+) Depth=(\d+)")


def compile_asm(asm):
    cmd = ["/opt/rocm/bin/hipcc", "-std=c++17", "-O3", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off",
           "-fno-fast-math", "-munsafe-fp-atomics", "-mllvm", "--amdgpu-set-wave-priority", "-mllvm",
           "--structurizecfg-skip-uniform-regions", "-gline-tables-only", "-I../include", "-Icsrc/host",
           "-Icsrc/device", "--cuda-device-only", "-S", "csrc/device/rt_kernels_f64.hip", "-o", asm]
    cmd += os.environ.get("ISA_FLAGS", "").split()
    subprocess.run(cmd, cwd=PKG, check=True, stderr=subprocess.DEVNULL)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("kernel", nargs="?", default="k_std_leanILb0ELi1ELb0E")
    ap.add_argument("--asm", default=None, help="existing assembly (skip the compile)")
    ap.add_argument("--keep-asm", default="/tmp/isa_spill.s", help="where the compile writes the assembly")
    ap.add_argument("--lanes", action="store_true", help="list every write and read of every spill lane")
    a = ap.parse_args()
    asm = a.asm or a.keep_asm
    if not a.asm:
        compile_asm(asm)

    files = {}
    pat = re.compile(r"^_Z\S*" + re.escape(a.kernel) + r"\S*:")
    inside = 0            # 0: before the kernel, 1: in its body, 2: in the resource comments after it
    loop = "-"            # innermost loop of the current block
    own = None            # the current block's own label
    fresh = False         # still in the block's leading comment lines
    cur = (None, 0)
    depth = {"-": 0}
    parent = {}
    insts = []            # (loop, (file, line), op, text)
    meta = {}
    with open(asm) as f:
        for raw in f:
            if raw.startswith("\t.file"):
                m = re.match(r'\t\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', raw)
                if m:
                    d, n = m.group(2), m.group(3)
                    path = os.path.join(d, n) if n else d
                    files[int(m.group(1))] = path if os.path.isabs(path) else os.path.join(PKG, path)
                continue
            if inside == 0:
                if pat.match(raw):
                    inside = 1
                continue
            if raw.startswith(".Lfunc_end"):
                inside = 2
                continue
            if inside == 2:
                m = re.match(r"\s*; (ScratchSize|Occupancy|NumVgprs|NumSgprs|TotalNumSgprs|codeLenInByte):\s*(\d+)", raw)
                if m:
                    meta.setdefault(m.group(1), int(m.group(2)))
                if raw.startswith("; LDSByteSize"):
                    break
                continue
            bm = BLOCK.match(raw)
            if bm:
                own, loop, fresh = bm.group(1), "-", True
            if fresh:
                m = THIS_LOOP.search(raw)
                if m and own:
                    loop = own
                    depth[own] = int(m.group(1))
                m = IN_LOOP.search(raw)
                if m:
                    loop = m.group(1)
                    depth[loop] = int(m.group(2))
                m = PARENT.search(raw)
                if m and own:
                    # the deepest parent listed is the direct one
                    if own not in parent or int(m.group(2)) > depth.get(parent[own], 0):
                        parent[own] = m.group(1)
                        depth[m.group(1)] = int(m.group(2))
            if raw.startswith("\t.loc"):
                p = raw.split()
                cur = (int(p[1]), int(p[2]))
                continue
            if not raw.startswith("\t") or raw.startswith("\t."):
                continue
            body = raw.split(";")[0]
            if not body.strip():
                continue
            fresh = False
            insts.append((loop, cur, body.split()[0], body.strip()))
    if not insts:
        print(f"kernel {a.kernel} not found in {asm}", file=sys.stderr)
        return 1

    spill_regs = {m.group(1) for _, _, _, t in insts for m in [WR.match(t)] if m}
    starts_cache = {}

    def where(loc):
        path = files.get(loc[0], "?")
        if path not in starts_cache:
            starts_cache[path] = func_starts(path)
        return f"{region(starts_cache[path], loc[1])}:{loc[1]}"

    per_loop = collections.defaultdict(collections.Counter)
    loop_funcs = collections.defaultdict(dict)
    lanes = collections.defaultdict(lambda: {"w": [], "r": []})
    order = []
    for lp, loc, op, text in insts:
        if lp not in per_loop:
            order.append(lp)
        c = classify(op)
        if c in VALU:
            per_loop[lp]["valu"] += 1
        elif c == "salu":
            per_loop[lp]["salu"] += 1
        if op == "s_nop":
            per_loop[lp]["nop"] += 1
        per_loop[lp]["n"] += 1
        fn, ln = where(loc).rsplit(":", 1)
        lo, hi = loop_funcs[lp].get(fn, (1 << 30, 0))
        loop_funcs[lp][fn] = (min(lo, int(ln)), max(hi, int(ln)))
        m = WR.match(text)
        if m and m.group(1) in spill_regs:
            per_loop[lp]["w"] += 1
            lanes[(m.group(1), int(m.group(3)))]["w"].append((lp, where(loc), m.group(2)))
            continue
        m = RD.match(text)
        if m and m.group(2) in spill_regs:
            per_loop[lp]["r"] += 1
            lanes[(m.group(2), int(m.group(3)))]["r"].append((lp, where(loc), m.group(1)))

    tot = collections.Counter()
    for c in per_loop.values():
        tot.update(c)
    print(f"# {a.kernel}: SGPR spill traffic per asm loop (static)")
    print("# " + "  ".join(f"{k}={v}" for k, v in sorted(meta.items())) + f"  spill VGPRs: {', '.join(sorted(spill_regs)) or 'none'}")
    print(f"{'loop':10s} {'depth':>5s} {'parent':10s} {'insts':>6s} {'valu':>6s} {'salu':>6s} {'s_nop':>6s} {'spill_w':>7s} {'spill_r':>7s}  source (function:first-last line)")
    for lp in order:
        c = per_loop[lp]
        fns = sorted(loop_funcs[lp].items(), key=lambda kv: kv[1][0])
        src = " ".join(f"{fn}:{lo}-{hi}" for fn, (lo, hi) in fns if hi)
        if len(src) > 150:
            src = src[:147] + "..."
        print(f"{lp:10s} {depth.get(lp, 0):5d} {parent.get(lp, '-'):10s} {c['n']:6d} {c['valu']:6d} {c['salu']:6d} {c['nop']:6d} "
              f"{c['w']:7d} {c['r']:7d}  {src}")
    print(f"{'TOTAL':10s} {'':5s} {'':10s} {tot['n']:6d} {tot['valu']:6d} {tot['salu']:6d} {tot['nop']:6d} {tot['w']:7d} {tot['r']:7d}")

    # spill traffic per source function (innermost inlined function of the move's .loc)
    per_fn = collections.defaultdict(collections.Counter)
    for (reg, lane), d in lanes.items():
        for k in ("w", "r"):
            for lp, src, _ in d[k]:
                per_fn[src.rsplit(":", 1)[0]][k] += 1
    print("\n# spill moves per source function")
    for fn, c in sorted(per_fn.items(), key=lambda kv: -(kv[1]["w"] + kv[1]["r"])):
        print(f"{fn:40s} writes {c['w']:4d}  reads {c['r']:4d}")

    print(f"\n# spill lanes: {len(lanes)}")
    print(f"{'lane':10s} {'writes':>6s} {'reads':>6s}  loops written in / read in")
    for (reg, lane), d in sorted(lanes.items(), key=lambda kv: (kv[0][0], kv[0][1])):
        wl = collections.Counter(lp for lp, _, _ in d["w"])
        rl = collections.Counter(lp for lp, _, _ in d["r"])
        print(f"{reg + '[' + str(lane) + ']':10s} {len(d['w']):6d} {len(d['r']):6d}  "
              f"w: {' '.join(f'{k}x{v}' for k, v in wl.items()) or '-'}  |  r: {' '.join(f'{k}x{v}' for k, v in rl.items()) or '-'}")
        if a.lanes:
            for lp, src, sreg in d["w"]:
                print(f"{'':12s}write {sreg:8s} loop {lp:10s} {src}")
            for lp, src, sreg in d["r"]:
                print(f"{'':12s}read  {sreg:8s} loop {lp:10s} {src}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
