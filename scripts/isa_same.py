# Developer tool (no GPU): are the kernels of two builds the same code?  Compares, per kernel name,
# the opcode sequence in order (operands ignored) and the resource fields of the kernel's metadata
# (VGPR, AGPR and SGPR counts, both spill counts, private segment and LDS size), and the two sets of
# kernel names.  For refactors that must not change the generated code: register numbers may move,
# instructions and resources may not.  Each side takes one or more device assembly files (a kernel
# may have moved between files), from hipcc --cuda-device-only -S with build.FLAGS, as kres.sh:
#   python3 scripts/isa_same.py old_a.s [old_b.s ...] -- new_a.s [new_b.s ...]
# Exit status 0 when every kernel is SAME on both counts and the name sets are equal.
import re
import sys

RES = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
       "private_segment_fixed_size", "group_segment_fixed_size")


def opcodes(lines):
    """The instructions' mnemonics in order; local labels kept as the order of their first appearance."""
    seen, out = {}, []
    for ln in lines:
        s = ln.split(";", 1)[0].strip()
        if not s:
            continue
        m = re.match(r"(\.L\w+):$", s)
        if m:
            out.append("L%d:" % seen.setdefault(m.group(1), len(seen)))
        elif not s.startswith(".") and not s.endswith(":"):
            out.append(s.split()[0])
    return out


def kernels(paths):
    """{kernel name: (opcode list, {resource field: value})} over the files of one side."""
    code, res = {}, {}
    for path in paths:
        asm = open(path).read()
        for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", asm, re.S | re.M):
            code[m.group(1)] = opcodes(m.group(2).splitlines())
        meta = asm.split("amdhsa.kernels:", 1)
        for entry in re.split(r"^  - (?=\.)", meta[1] if len(meta) > 1 else "", flags=re.M)[1:]:
            f = dict(re.findall(r"^\s*\.(\w+):\s+(\S+)\s*$", entry, re.M))
            res[f["name"]] = {k: f.get(k) for k in RES}
    return {n: (code.get(n), res[n]) for n in res}   # kernels only: device functions carry no metadata


def first_diff(a, b):
    n = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    return "at %d: %s | %s (%d, %d instructions)" % (n, " ".join(a[n:n + 3]), " ".join(b[n:n + 3]), len(a), len(b))


def main(argv):
    if "--" not in argv:
        sys.exit("usage: isa_same.py OLD.s [...] -- NEW.s [...]")
    cut = argv.index("--")
    old, new = kernels(argv[:cut]), kernels(argv[cut + 1:])
    bad = 0
    for n in sorted(set(old) - set(new)):
        print("MISSING  %s" % n)
    for n in sorted(set(new) - set(old)):
        print("ADDED    %s" % n)
    bad += len(set(old) ^ set(new))
    for n in sorted(set(old) & set(new)):
        (ca, ra), (cb, rb) = old[n], new[n]
        ops = "SAME" if ca == cb else "DIFF"
        rs = "SAME" if ra == rb else "DIFF"
        print("opcodes %s  resources %s  %s" % (ops, rs, n))
        if ca != cb:
            print("    " + first_diff(ca or [], cb or []))
        if ra != rb:
            print("    " + ", ".join("%s %s -> %s" % (k, ra[k], rb[k]) for k in RES if ra[k] != rb[k]))
        bad += ca != cb or ra != rb
    print("kernel names: %s (%d | %d); %d of %d kernels differ" %
          ("SAME" if set(old) == set(new) else "DIFF", len(old), len(new), bad, len(set(old) | set(new))))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
