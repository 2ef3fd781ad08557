#!/usr/bin/env python3
"""Generate tests/golden/noclass_importance.{json,npz} by RUNNING THE REFERENCE's compute_importance on CPU.

Run where the reference is at hand, like make_golden.py (whose loader this uses; nothing of the reference is copied):
        PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_noclass.py

The reference has no mean query.  What ties the mean-query rule (include/rajni_hip_query.h) to it is an input on which the
two coincide: fp32 qkv whose N query rows are all THE SAME row, so that the mean query is the reference's q[:, :, 0].  The
equality is exact in every summation order: N is a power of two (x 1/N and / N agree) and the Q entries are integer
multiples of 2^-6 in [-4, 4] (any partial sum of up to 256 of them has at most 19 significant bits).  K and V are standard
normal.  Arrays only: the reference's fp32 scores of each case and, like importance_cases.json's `stored_qkv`, the qkv of the
two small cases; every qkv is rebuilt from (seed, case) by tests/numerics_noclass.py::fixture_qkv, which the tests check
against the stored ones."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, os.path.dirname(HERE), ROOT, os.path.join(ROOT, "rajni-vit_amd")):
    sys.path.insert(0, p)
sys.dont_write_bytecode = True

from make_golden import load_reference  # noqa: E402
from numerics_noclass import fixture_qkv  # noqa: E402

SEED = 20
CASES = [dict(B=2, N=64, H=2, D=16, stored_qkv=True), dict(B=2, N=256, H=3, D=64, stored_qkv=False),
         dict(B=1, N=64, H=2, D=80, stored_qkv=True)]


def main():
    _, refw = load_reference()
    from rajni_ref.wrapper.importance import compute_importance
    arrays = {}
    for j, c in enumerate(CASES):
        qkv = fixture_qkv(SEED, j, c["B"], c["N"], c["H"], c["D"])
        if c["stored_qkv"]:
            arrays[f"c{j}.qkv"] = qkv
        arrays[f"c{j}.scores"] = compute_importance(torch.from_numpy(qkv), c["H"]).numpy()
    np.savez_compressed(os.path.join(HERE, "noclass_importance.npz"), **arrays)
    with open(os.path.join(HERE, "noclass_importance.json"), "w") as f:
        json.dump(dict(seed=SEED, cases=CASES, note="Q rows identical per image: the mean query is the reference's CLS query"), f,
                  indent=1)
    print("wrote", len(CASES), "cases,", os.path.getsize(os.path.join(HERE, "noclass_importance.npz")), "bytes")


if __name__ == "__main__":
    main()
