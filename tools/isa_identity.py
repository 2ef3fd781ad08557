#!/usr/bin/env python3
"""Compare two gfx950 assembly listings of csrc/gemm.hip (the `hipcc -S --cuda-device-only` line of tools/scan_isa.py), kernel
by kernel: every kernel symbol of OLD must exist in NEW with an identical body - instructions, labels and the resource
summary (registers, LDS, scratch) behind it.  Lines that carry only file-wide numbering (.Lfunc_end / .LBB function indices,
section ordinals) are normalised; nothing else is.  Prints one line per kernel of NEW; exit status 1 when a kernel of OLD
differs or is missing.

    python tools/isa_identity.py old.s new.s [--map REGEX REPL ...]

--map: a kernel that gained a template parameter has a new mangled name.  Each REGEX -> REPL pair (re.sub, in order) turns a
symbol of NEW into the symbol it had in OLD; such a kernel is compared under its old name (its own name inside its body is
rewritten the same way) and printed as `identical` / `DIFFERS` with `<- old symbol` behind it.
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
    args = sys.argv[1:]
    maps = []
    while "--map" in args:
        i = args.index("--map")
        maps.append((re.compile(args[i + 1]), args[i + 2]))
        del args[i:i + 3]
    old, new = kernels(args[0]), kernels(args[1])
    bad = n_same = n_new = 0
    seen = set()
    for k in sorted(new):
        ko = k
        for rx, repl in maps:
            ko = rx.sub(repl, ko)
        body = new[k].replace(k, ko) if ko != k else new[k]
        h = hashlib.sha256(body.encode()).hexdigest()[:16]
        if ko not in old:
            state, n_new = "NEW", n_new + 1
        elif old[ko] == body:
            state, n_same = "identical", n_same + 1
        else:
            state, bad = "DIFFERS", bad + 1
        seen.add(ko)
        print(f"{state:9s} {h} {len(body.splitlines()):6d} lines  {k}" + (f"  <- {ko}" if ko != k and ko in old else ""))
    for k in sorted(set(old) - seen):
        print(f"MISSING   {k}")
        bad += 1
    print(f"# {len(old)} kernels in old, {len(new)} in new: {n_same} identical, {n_new} new, {bad} differing or missing")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
