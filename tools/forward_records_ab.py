#!/usr/bin/env python3
"""Print what the library named by RAJNI_HIP_LIB (default: the tree's build) answers to every case of tests/forward_records.py:
one line per (case, entry point) with the return code, the refusal text, and every size function's return on the case's
records.  No GPU: every plan has workspace = NULL, nothing is launched.  Run it on two builds and compare the outputs: a
refactor of the forward's host code must leave them identical line for line.

  RAJNI_HIP_LIB=/path/to/parent/librajni_hip.so python tools/forward_records_ab.py --digest
  python tools/forward_records_ab.py --digest

Columns, tab separated: entry point, the case's labels, rc, message, the five sizes, and LAST: rajni_last_error after each
size function that returned 0 ("-" where it left the error of the call in front of it untouched).  The last column is apart
because it is the one place where two correct builds may differ; --digest hashes it apart too.  --sizes prints one line per
(plan, prefix, image, query, pool) with the sizes and that column alone: short enough to diff."""
import argparse
import hashlib
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "rajni-vit_amd"))

import forward_records as fr  # noqa: E402
from rajni_amd import _native as nat  # noqa: E402


def size_columns(lib, key, cache):
    """(sizes, last errors) of the five size functions on (plan, prefix, image, query, pool), each behind a refused call
    with a known text so that an untouched error is visible as such"""
    labels = tuple(v.label for v in key)
    hit = cache.get(labels)
    if hit is None:
        sizes, errors = [], []
        for level in range(len(fr.SIZE_FUNCTIONS)):
            lib.rajni_vit_forward(None, None, None, None)
            marker = lib.rajni_last_error()
            n = fr.size(lib, level, key[: level + 1])
            err = lib.rajni_last_error()
            sizes.append(str(n))
            errors.append("" if n else ("-" if err == marker else err.decode()))
        hit = cache[labels] = ("\t".join(sizes), "|".join(errors))
    return hit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--digest", action="store_true", help="print the line count and sha256 of the columns, not the lines")
    ap.add_argument("--sizes", action="store_true", help="one line per size-function case only")
    args = ap.parse_args()
    lib = nat.lib()
    cache = {}
    main_hash, last_hash, lines = hashlib.sha256(), hashlib.sha256(), 0
    out = sys.stdout
    if args.sizes:
        for key in fr.size_cases(len(fr.SIZE_RECORDS)):
            sizes, errors = size_columns(lib, key, cache)
            out.write("\t".join([",".join(v.label for v in key), sizes, errors]) + "\n")
        return
    null = fr.axes()["pool"][0]
    for level, name in enumerate(fr.ENTRY_POINTS):
        for case in fr.cases(level):
            rc, msg = fr.forward(lib, level, case)
            full = case + (null,) * (len(fr.ENTRY_POINTS) - len(case))
            sizes, errors = size_columns(lib, (full[0], full[2], full[4], full[5], full[6]), cache)
            line = "\t".join([name, ",".join(v.label for v in case), str(rc), msg.decode() if rc else "", sizes])
            lines += 1
            if args.digest:
                main_hash.update(line.encode() + b"\n")
                last_hash.update(errors.encode() + b"\n")
            else:
                out.write(line + "\t" + errors + "\n")
    if args.digest:
        print(f"library {nat.LIB_PATH}")
        print(f"lines {lines} sha256 {main_hash.hexdigest()} last_error_after_zero_size sha256 {last_hash.hexdigest()}")


if __name__ == "__main__":
    main()
