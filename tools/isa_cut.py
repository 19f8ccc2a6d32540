"""Where the argmax passes spill: compile cut_argmax.hip to gfx950 assembly once with the given -D
flags, and for each requested instantiation cut_argmax<pass>_kernel<KB> (pass 2 = fp64, 3 = fp32,
4 = integer) count, per loop (a branch back to an earlier label), the MFMAs, LDS reads, scratch
loads / stores, VALU-ish and s_barrier instructions.  CPU only.
Usage: python tools/isa_cut.py [PASS:]KB ... [--table] [--src FILE] [-DFLAG ...]
  isa_cut.py 30            cut_argmax3_kernel<30> (the pass defaults to 3)
  isa_cut.py 2:22 4:30     cut_argmax2_kernel<22> and cut_argmax4_kernel<30>, one compilation
  isa_cut.py --table       one line per instantiation of the three kernels: the compiler's resource
                           usage and the chunk loop's (innermost loop with MFMAs) scratch accesses"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "sqlp_amd", "csrc", "cut_argmax.hip")
KBS = (1, 2, 4, 6, 8, 12, 16, 22, 24, 30, 32)


def compile_asm(src, flags):
    with tempfile.TemporaryDirectory() as d:
        asm = os.path.join(d, "c.s")
        subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.dirname(SRC)] + flags + [src, "-o", asm],
                       check=True, capture_output=True)
        return open(asm).read()


def count(seg):
    c = {"mfma": 0, "ds_read": 0, "scratch_ld": 0, "scratch_st": 0, "v_": 0, "s_": 0, "barrier": 0, "global": 0, "waitcnt": 0}
    for l in seg:
        if l.startswith("v_mfma"): c["mfma"] += 1
        elif l.startswith("ds_read"): c["ds_read"] += 1
        elif l.startswith("scratch_load") or (l.startswith("buffer_load") and "off, s[0:3]" in l): c["scratch_ld"] += 1
        elif l.startswith("scratch_store"): c["scratch_st"] += 1
        elif l.startswith("s_barrier"): c["barrier"] += 1
        elif l.startswith("s_waitcnt"): c["waitcnt"] += 1
        elif l.startswith("global_"): c["global"] += 1
        elif l.startswith("v_"): c["v_"] += 1
        elif l.startswith("s_"): c["s_"] += 1
    return c


def kernel(text, pas, KB):
    """(code lines, the compiler's resource summary) of cut_argmax<pas>_kernel<KB>; loops with MFMAs, smallest first"""
    sym = f"_ZN5twosd18cut_argmax{pas}_kernelILi{KB}EEEvNS_9CutParamsE"
    rest = text[text.index(sym + ":"):]
    end = rest.index(".Lfunc_end")
    lines = [l.strip() for l in rest[:end].splitlines()]
    usage = dict(re.findall(r"^; (Occupancy|ScratchSize|LDSByteSize|NumVgprs): (\d+)", rest[end:end + 4000], re.M))
    labels = {re.match(r"^(\.LBB[^:]+):", l).group(1): i for i, l in enumerate(lines) if re.match(r"^\.LBB[^:]+:", l)}
    loops = []
    for i, l in enumerate(lines):
        m = re.match(r"^s_cbranch_\w+\s+(\.LBB\S+)|^s_branch\s+(\.LBB\S+)", l)
        if m:
            t = m.group(1) or m.group(2)
            if t in labels and labels[t] < i:
                loops.append((labels[t], i))
    loops = [lp for lp in sorted(loops, key=lambda t: t[1] - t[0]) if count(lines[lp[0]:lp[1] + 1])["mfma"] > 0]
    return lines, usage, loops


def main():
    args = sys.argv[1:]
    src = SRC
    if "--src" in args:
        i = args.index("--src")
        src = args[i + 1]
        del args[i:i + 2]
    table = "--table" in args
    flags = [a for a in args if a.startswith("-") and a != "--table"]
    want = [tuple(int(x) for x in (a if ":" in a else "3:" + a).split(":")) for a in args if not a.startswith("-")]
    if table:
        want = [(p, kb) for p in (2, 3, 4) for kb in KBS]
    text = compile_asm(src, flags)
    if table:
        print("flags", flags)
        print("kernel              occupancy  LDS bytes  scratch bytes/lane  VGPRs  chunk loop: scratch loads  stores")
    for pas, KB in want or [(3, 30)]:
        lines, usage, loops = kernel(text, pas, KB)
        if table:
            c = count(lines[loops[0][0]:loops[0][1] + 1])
            print(f"cut_argmax{pas}<{KB:2d}>     {usage['Occupancy']:>9}  {usage['LDSByteSize']:>9}  {usage['ScratchSize']:>18}"
                  f"  {usage['NumVgprs']:>5}  {c['scratch_ld']:>25}  {c['scratch_st']:>6}")
            continue
        print(f"cut_argmax{pas}_kernel<{KB}>", "flags", flags, "whole kernel", count(lines))
        for a, b in loops[:3]:
            print(f"loop lines {a}-{b} ({b - a}):", count(lines[a:b + 1]))


if __name__ == "__main__":
    main()
