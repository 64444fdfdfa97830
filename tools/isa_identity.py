#!/usr/bin/env python3
"""Are the kernels of two assembly files the same text?

    python tools/isa_identity.py before.s after.s

Both files are `hipcc -S --cuda-device-only` output of one unit (the compile line of tests/isa.py).  A kernel is the text from its
`<symbol>:` line through its `.end_amdhsa_kernel`.  Reports the symbols present in one file only and the symbols whose text differs, each
with its first differing line; exits 1 on any difference.  Text is compared as it stands: nothing is normalised and no instruction is
looked for.  This is how a change that only moves source text is shown to leave the device code alone."""
import re
import sys


def kernels(path):
    """symbol -> lines of the kernel, in file order"""
    lines = open(path).read().split("\n")
    label_at, found, name = {}, {}, None
    for i, line in enumerate(lines):
        m = re.match(r"([A-Za-z_.$][\w.$]*):", line)
        if m:
            label_at[m.group(1)] = i
        elif line.strip().startswith(".amdhsa_kernel "):
            name = line.split()[1]
        elif line.strip() == ".end_amdhsa_kernel":
            found[name] = lines[label_at[name]:i + 1]
    return found


def main(argv):
    if len(argv) != 3:
        print(__doc__)
        return 2
    a, b = kernels(argv[1]), kernels(argv[2])
    bad = 0
    for path, mine, other in ((argv[1], a, b), (argv[2], b, a)):
        for sym in mine:
            if sym not in other:
                print(f"only in {path}: {sym}")
                bad += 1
    same = 0
    for sym in a:
        if sym not in b:
            continue
        if a[sym] == b[sym]:
            same += 1
            continue
        bad += 1
        n = next((i for i, (x, y) in enumerate(zip(a[sym], b[sym])) if x != y), min(len(a[sym]), len(b[sym])))
        print(f"differs: {sym} ({len(a[sym])} / {len(b[sym])} lines), first at line {n + 1} of the kernel:")
        print(f"  < {a[sym][n] if n < len(a[sym]) else '(end)'}")
        print(f"  > {b[sym][n] if n < len(b[sym]) else '(end)'}")
    print(f"{argv[1]}: {len(a)} kernels; {argv[2]}: {len(b)} kernels; {same} identical, {bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
