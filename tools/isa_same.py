"""Do two source forms of a kernel compile to the same machine code?  Compile one .hip file from
two trees to gfx950 assembly and, for each pair OLD=NEW of kernel instantiations, compare the two
instruction streams and kernel descriptors line by line after normalising what a rename alone
changes: the kernel's own mangled symbol and the function number in local labels.  CPU only; it
compares and does nothing else.
Usage: python tools/isa_same.py --old TREE [--new TREE] [--file PATH] [--map FILE] [-DFLAG ...] [OLD=NEW ...]
  --old / --new   the two checkouts (--new defaults to this one)
  --file          the source, relative to a tree (default sqlp_amd/csrc/boot_kernel.hip)
  OLD=NEW         kernels of namespace twosd as written in the source, template arguments integers
                  or true / false: 'boot_treform_kernel<1, false>=boot_reform_kernel<1, 0, true>';
                  a name alone stands for NAME=NAME
  --map           a file of such pairs, one per line (# starts a comment line)
Per pair one line: `identical` (every instruction, label and descriptor line), or the number of
differing lines with both sides' instruction counts and VGPRs, SGPRs, LDS, scratch and occupancy,
followed by the differing lines themselves (- old, + new)."""
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
USAGE = ("NumVgprs", "TotalNumSgprs", "LDSByteSize", "ScratchSize", "Occupancy")


def compile_asm(tree, rel, flags):
    src = os.path.join(tree, rel)
    with tempfile.TemporaryDirectory() as d:
        asm = os.path.join(d, "k.s")
        subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                        "-I" + os.path.join(tree, "include"), "-I" + os.path.dirname(src)] + flags + [src, "-o", asm],
                       check=True, capture_output=True)
        return open(asm).read()


def mangled_prefix(name):
    """_ZN5twosd<len><name>I<args>EE of twosd::name<args> (the parameter types follow it)"""
    m = re.fullmatch(r"\s*(\w+)\s*(?:<(.*)>)?\s*", name)
    if not m:
        sys.exit(f"cannot read kernel name {name!r}")
    out = f"_ZN5twosd{len(m.group(1))}{m.group(1)}"
    if m.group(2) is None:
        return out + "E"
    out += "I"
    for a in (a.strip() for a in m.group(2).split(",")):
        if a in ("true", "false"):
            out += "Lb%dE" % (a == "true")
        else:
            v = int(a)
            out += "Li%sE" % (f"n{-v}" if v < 0 else v)
    return out + "EE"


def kernel(text, name):
    """(normalised lines of the body and the descriptor, resource usage, instruction count)"""
    pre = mangled_prefix(name)
    syms = sorted(set(re.findall(r"^\s*\.amdhsa_kernel\s+(" + re.escape(pre) + r"\S*)", text, re.M)))
    if len(syms) != 1:
        sys.exit(f"{name}: {len(syms)} kernels with symbol prefix {pre}")
    sym = syms[0]
    body = text[text.index("\n" + sym + ":") + 1:]
    end = body.index(".Lfunc_end")          # the instructions, then the descriptor (.amdhsa_kernel) in .rodata
    tail = body[end:]
    usage = dict(re.findall(r"^; (\w+): (\d+)", tail[:tail.index("; Occupancy") + 40], re.M))
    lines, ninstr = [], 0
    for l in body[:end].splitlines()[1:]:
        l = l.split(";")[0].strip()
        if not l:
            continue
        ninstr += re.match(r"[a-z]\w*(\s|$)", l) is not None
        l = l.replace(sym, "<kernel>").replace(sym[2:], "<kernel>")
        lines.append(re.sub(r"\.L(BB|tmp|func_begin|func_end)\d+", r".L\1", l))
    return lines, {u: usage.get(u, "?") for u in USAGE}, ninstr


def main():
    args = sys.argv[1:]
    opt = {"--old": None, "--new": ROOT, "--map": None, "--file": os.path.join("sqlp_amd", "csrc", "boot_kernel.hip")}
    for o in opt:
        if o in args:
            i = args.index(o)
            opt[o] = args[i + 1]
            del args[i:i + 2]
    if opt["--map"]:
        args += [l.strip() for l in open(opt["--map"]) if l.strip() and not l.startswith("#")]
    flags = [a for a in args if a.startswith("-")]
    pairs = [a.split("=") if "=" in a else [a, a] for a in args if not a.startswith("-")]
    if not opt["--old"] or not pairs:
        sys.exit(__doc__)
    old = compile_asm(os.path.abspath(opt["--old"]), opt["--file"], flags)
    new = compile_asm(os.path.abspath(opt["--new"]), opt["--file"], flags)
    print(f"{opt['--file']}, -O3 --offload-arch=gfx950" + "".join(" " + f for f in flags) + ": old -> new")
    for a, b in pairs:
        la, ua, na = kernel(old, a)
        lb, ub, nb = kernel(new, b)
        head = f"{a.strip()} -> {b.strip()}: "
        res = "  ".join(f"{u} {ua[u]}/{ub[u]}" for u in USAGE)
        if la == lb:
            print(head + f"identical ({na} instructions; {res})")
            continue
        diff = [d for d in difflib.unified_diff(la, lb, n=0, lineterm="") if d[:1] in "+-" and d[:3] not in ("+++", "---")]
        print(head + f"{len(diff)} differing lines; instructions {na}/{nb}  {res}")
        for d in diff:
            print("    " + d)


if __name__ == "__main__":
    main()
