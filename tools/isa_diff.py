"""Compare the kernels of two gfx950 assembly files (hipcc -S --cuda-device-only of the same source before and after a change):

    python3 tools/isa_diff.py before.s after.s

A file is cut at its kernel symbols (`_Z...:` up to `.Lfunc_end`, plus the kernel's `.amdhsa_kernel` descriptor: registers,
LDS, scratch); local labels (`.LBB3_7` -> `L`) are normalised and `;` comments and blank lines are dropped, so renumbered
functions compare equal.  Prints the kernels only in A, only in B and the
kernels whose bodies differ; exit status 1 if any body differs or B has a kernel that A lacks."""
import re
import sys


def kernels(path):
    out, name, body = {}, None, []
    for l in open(path):
        m = re.match(r"^(_Z\w+):", l) or re.match(r"^\s*\.amdhsa_kernel\s+(_Z\w+)", l)
        if m and name is None:
            name = m.group(1)
            body = out.setdefault(name, [])
        elif name is not None and l.strip().startswith((".Lfunc_end", ".end_amdhsa_kernel")):
            name = None
        elif name is not None:
            t = re.sub(r"\.L\w+", "L", l.split(";")[0]).strip()
            if t:
                body.append(t)
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = sorted(k for k in set(a) & set(b) if a[k] != b[k])
    print(f"kernels: {len(a)} in A, {len(b)} in B, {len(set(a) & set(b))} in both")
    for title, names in (("only in A", only_a), ("only in B", only_b), ("bodies differ", differ)):
        print(f"{title}: {len(names)}")
        for n in names:
            print("   ", n)
    return 1 if differ or only_b else 0


if __name__ == "__main__":
    sys.exit(main())
