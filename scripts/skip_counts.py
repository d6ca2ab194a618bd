# Developer tool (no GPU): exec-region counts per kernel of a device assembly file (hipcc --cuda-device-only -S
# with build.FLAGS, as isa_same.py): s_cbranch_execz, s_and_saveexec, VALU and all instructions, over the whole
# kernel and over its largest backward-branch loop (the IPM loop of the qp_step kernels), with the registers,
# SGPR spills and scratch of the kernel's metadata.  profiles/skip_branches/static_counts.txt is its output.
#   python3 scripts/skip_counts.py file.s [kernel-name-regex]
import re
import sys

from isa_counts import kernels
from isa_same import kernels as resources

SEL = r"qp_step|sqp_loop|merit_ls"


def ops(lines):
    out = []
    for ln in lines:
        s = ln.split(";", 1)[0].strip()
        if s and not s.startswith(".") and not s.endswith(":"):
            out.append(s.split()[0])
    return out


def counts(lines):
    o = ops(lines)
    return (len(o), sum(x.startswith("v_") for x in o), sum(x == "s_cbranch_execz" for x in o),
            sum(x.startswith("s_and_saveexec") for x in o))


def largest_loop(body):
    labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}
    best = (0, 0)
    for i, l in enumerate(body):
        m = re.search(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
        if m and labels.get(m.group(1), i) < i and i - labels[m.group(1)] > best[1] - best[0]:
            best = (labels[m.group(1)], i + 1)
    return body[best[0]:best[1]]


if __name__ == "__main__":
    path = sys.argv[1]
    sel = sys.argv[2] if len(sys.argv) > 2 else SEL
    res = resources([path])
    print("kernel\tinstructions\tVALU\texecz\tsaveexec\tloop: instructions\tVALU\texecz\tsaveexec\tVGPRs\tSGPR spills\tscratch")
    for name, body in kernels(open(path).read()):
        if name not in res or not re.search(sel, name):
            continue
        r = res[name][1]
        row = counts(body) + counts(largest_loop(body)) + (r["vgpr_count"], r["sgpr_spill_count"], r["private_segment_fixed_size"])
        print(name + "\t" + "\t".join(str(x) for x in row))
