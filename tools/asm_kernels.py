"""Per-kernel comparison of two gfx950 assembly files of one translation unit (hipcc <build.py's FLAGS> --cuda-device-only -S):
instruction count, VGPRs, SGPRs, LDS and scratch bytes before and after, and whether the instruction streams are identical once
comments, labels and directives are stripped.  python tools/asm_kernels.py BEFORE.s AFTER.s"""
import re
import subprocess
import sys

META = {"vgpr": r"\.vgpr_count:\s+(\d+)", "sgpr": r"\.sgpr_count:\s+(\d+)", "lds": r"\.group_segment_fixed_size:\s+(\d+)",
        "scratch": r"\.private_segment_fixed_size:\s+(\d+)"}


def kernels(path):
    text = open(path).read()
    out = {}
    # code: from "<symbol>:" to its .Lfunc_end; every other line that starts with a tab and no dot is an instruction
    for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        body = [re.sub(r"\s*;.*$", "", l).strip() for l in m.group(2).split("\n")]
        body = [re.sub(r"\.LBB\d+_", ".LBB_", l) for l in body if l and not l.startswith(".") and not l.endswith(":")]
        out[m.group(1)] = {"insts": body}
    for m in re.finditer(r"^  - \.agpr_count:.*?^    \.name:\s+(\w+)\n.*?(?=^  - \.agpr_count:|^amdhsa\.target)", text, re.S | re.M):
        if m.group(1) in out:
            for k, pat in META.items():
                out[m.group(1)][k] = int(re.search(pat, m.group(0)).group(1))
    return {k: v for k, v in out.items() if "vgpr" in v}


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    names = sorted(set(a) | set(b))
    dem = subprocess.run(["c++filt"] + names, stdout=subprocess.PIPE, text=True).stdout.split("\n")
    print("%-58s %13s %9s %9s %15s %7s  %s" % ("kernel", "instructions", "VGPR", "SGPR", "LDS", "scratch", "stream"))
    for name, d in zip(names, dem):
        d = re.sub(r"^void |\(anonymous namespace\)::|\(.*$", "", d)
        if name not in a or name not in b:
            print("%-58s only in %s" % (d, "AFTER" if name in b else "BEFORE"))
            continue
        x, y = a[name], b[name]
        pair = lambda k: "%d/%d" % (x[k], y[k])
        print("%-58s %13s %9s %9s %15s %7s  %s" % (d, "%d/%d" % (len(x["insts"]), len(y["insts"])), pair("vgpr"), pair("sgpr"), pair("lds"),
                                                     pair("scratch"), "identical" if x["insts"] == y["insts"] else "differs"))


if __name__ == "__main__":
    main()
