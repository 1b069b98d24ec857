"""Census of the hot loop of pg_mm.h (scan()) on the generated ISA, per pg_mm_kernel instance: what ONE super-tile costs.
A step of the loop is found by its fragment wait (the inline-assembly `s_waitcnt vmcnt(4)`): it runs from the start of the
straight-line code in front of that wait (address update, the ring's loads) to the second branch behind it (the test for
candidates, the test for the end of the stretch).  Counted per step: MFMAs, VALU instructions (v_*, MFMAs aside),
lane-spill instructions (v_readlane / v_writelane), scratch accesses, and the chain heads - MFMAs that do not accumulate
onto their own result - with whether their addend is an inline constant (a register there means the compiler keeps a
splat alive: 16 VGPRs refilled in every iteration).
usage: tools/check_scan_loop.py [G ...] [--src DIR] [--json] [--kernel PREFIX]     (compiles DIR/pg_nsq_inst.hip -S per group
count; DIR defaults to prograph_amd/csrc; PREFIX: the kernels whose mangled name starts with it, default _Z12pg_mm_kernel -
_Z20pg_mm_knn_sym_kernel is the symmetric kNN sweep).  Exit status 1 if a step holds spill or scratch code or a head with a register addend."""
import json, os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = "-O3 -std=c++17 --offload-arch=gfx950 -fPIC -Wno-unused-function -Wno-pass-failed -Wno-unused-variable -mllvm -amdgpu-mfma-vgpr-form=1".split()


def instances(path, prefix="_Z12pg_mm_kernel"):
    """{kernel: [(text, in_asm, is_label)]} for every kernel of an assembly file whose name starts with prefix"""
    out, kernel, in_asm = {}, None, False
    for line in open(path):
        t = line.strip()
        if t.startswith(prefix) and ":" in t and not t.endswith('"'):
            kernel, in_asm = t.split(":")[0], False
            out[kernel] = []
            continue
        if not kernel:
            continue
        if t.startswith(";;#ASMSTART"):
            in_asm = True; continue
        if t.startswith(";;#ASMEND"):
            in_asm = False; continue
        if re.match(r"\.LBB\w+:", t):
            out[kernel].append((t, False, True)); continue
        if not t or t.startswith(";") or t.startswith("."):
            continue
        out[kernel].append((t, in_asm, False))
        if t.startswith("s_endpgm"):
            kernel = None
    return out


def is_branch(t):
    return t.startswith("s_cbranch") or t.startswith("s_branch")


def steps(instrs):
    res = []
    for i, (t, in_asm, lab) in enumerate(instrs):
        if not (in_asm and t.startswith("s_waitcnt vmcnt(4)")):
            continue
        a = i
        while a > 0 and not instrs[a - 1][2] and not is_branch(instrs[a - 1][0]):
            a -= 1
        b, nb = i, 0
        while b + 1 < len(instrs) and not instrs[b + 1][2] and nb < 2:
            b += 1
            nb += is_branch(instrs[b][0])
        res.append([x[0] for x in instrs[a:b + 1]])
    return res


def census(step):
    c = {"mfma": 0, "valu": 0, "lane_spill": 0, "scratch": 0, "heads": 0, "heads_inline": 0}
    for t in step:
        op = t.split()[0]
        if op.startswith("v_mfma"):
            c["mfma"] += 1
            ops = [o.strip() for o in t[len(op):].split(",")]
            dst, addend = ops[0], ops[3].split()[0]
            if addend != dst:
                c["heads"] += 1
                c["heads_inline"] += not re.match(r"[vas]\[?\d", addend)
        elif op in ("v_readlane_b32", "v_writelane_b32"):
            c["lane_spill"] += 1
        elif op.startswith("v_"):
            c["valu"] += 1
        elif op.startswith("scratch_") or (op.startswith("buffer_") and "offen" not in t and " off," in t):
            c["scratch"] += 1
    return c


def main():
    args = sys.argv[1:]
    src = os.path.join(ROOT, "prograph_amd", "csrc")
    if "--src" in args:
        src = os.path.abspath(args[args.index("--src") + 1])
        del args[args.index("--src"):args.index("--src") + 2]
    prefix = "_Z12pg_mm_kernel"
    if "--kernel" in args:
        prefix = args[args.index("--kernel") + 1]
        del args[args.index("--kernel"):args.index("--kernel") + 2]
    as_json = "--json" in args
    gs = [int(a) for a in args if a.isdigit()] or list(range(1, 9))
    bad, report = 0, {}
    tmp = tempfile.TemporaryDirectory()
    for g in gs:
        out = os.path.join(tmp.name, f"scan_g{g}.s")
        subprocess.check_call(["/opt/rocm/bin/hipcc"] + FLAGS + [f"-DPG_G={g}", "-S", "--cuda-device-only", "pg_nsq_inst.hip", "-o", out],
                              cwd=src, stderr=subprocess.DEVNULL)
        for name, instrs in instances(out, prefix).items():
            cs = [census(s) for s in steps(instrs)]
            if not cs:
                continue
            worst = {k: max(c[k] for c in cs) for k in cs[0]}
            worst["steps"] = len(cs)
            worst["heads_inline"] = min(c["heads_inline"] - c["heads"] for c in cs) == 0
            report[name] = worst
            ok = worst["lane_spill"] == 0 and worst["scratch"] == 0 and worst["heads_inline"]
            bad += not ok
            if not as_json:
                print(f"G={g} {name}: {len(cs)} steps; per super-tile at most {worst['mfma']} MFMAs ({worst['heads']} heads, addends "
                      f"{'inline' if worst['heads_inline'] else 'IN REGISTERS'}), {worst['valu']} VALU, {worst['lane_spill']} lane-spill, "
                      f"{worst['scratch']} scratch instructions{'' if ok else '   <-- NOT CLEAN'}")
    if as_json:
        print(json.dumps(report))
    else:
        print("instances with spill or scratch code or register addends in the loop:", bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
