#!/usr/bin/env python3
"""Compare two gfx950 assembly listings of csrc/gemm.hip (the `hipcc -S --cuda-device-only` line of tools/scan_isa.py), kernel
by kernel: every kernel symbol of OLD must exist in NEW with an identical body - instructions, labels and the resource
summary (registers, LDS, scratch) behind it.  Lines that carry only file-wide numbering (.Lfunc_end / .LBB function indices,
section ordinals) are normalised; nothing else is.  Prints one line per kernel of NEW; exit status 1 when a kernel of OLD
differs or is missing.

    python tools/isa_identity.py old.s new.s
"""
import hashlib
import re
import sys


def kernels(path):
    """{symbol: normalised body text} of every .amdhsa kernel in the listing"""
    out, name, body = {}, None, []
    names = set()
    lines = open(path).read().split("\n")
    for ln in lines:
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            names.add(m.group(1))
    for ln in lines:
        m = re.match(r"^(\S+):\s*(;.*)?$", ln)
        if m and m.group(1) in names and name is None:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if re.match(r"\s*\.end_amdhsa_kernel", ln):
            out[name] = "\n".join(body)
            name = None
            continue
        # function-local labels are numbered by the function's index in the file: .LBB12_3 -> .LBB_3
        # (and so are the loop comments that name them: "Header=BB12_8")
        ln = re.sub(r"\bL?BB\d+_(?=\d)", "BB_", ln)
        # ... and the comment behind a label is aligned to a column, so the padding changes with the index's digit count
        # (.LBB99_6: -> .LBB100_6: once a file has a hundred functions): one space there
        ln = re.sub(r"^(\.BB_\d+:)\s+;", r"\1 ;", ln)
        ln = re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", ln)
        ln = re.sub(r"\.Lfunc_begin\d+", ".Lfunc_begin", ln)
        body.append(ln.rstrip())
    return out


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for k in sorted(new):
        h = hashlib.sha256(new[k].encode()).hexdigest()[:16]
        if k not in old:
            state = "NEW"
        elif old[k] == new[k]:
            state = "identical"
        else:
            state, bad = "DIFFERS", bad + 1
        print(f"{state:9s} {h} {len(new[k].splitlines()):6d} lines  {k}")
    for k in sorted(set(old) - set(new)):
        print(f"MISSING   {k}")
        bad += 1
    n_same = sum(1 for k in old if k in new and old[k] == new[k])
    print(f"# {len(old)} kernels in old, {len(new)} in new: {n_same} identical, {len(set(new) - set(old))} new, {bad} differing or missing")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
