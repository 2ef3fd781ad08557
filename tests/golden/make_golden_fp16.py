"""Generate base224_fp16.{json,npz}: the reference wrapper run in float16 on CPU on the base224 case - the same config,
seeds, weights, images and schedule as base224_fp32 / base224_bf16 (make_golden.py, whose run_case this calls).

    python tests/golden/make_golden_fp16.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402


def compact(name):
    """Store the float arrays that hold fp16 values (all of them: the run is fp16 end to end) as float16 - lossless, and
    half the bytes of the float32 copies run_case writes (those compress poorly: no zero low mantissa bits as in bf16)."""
    path = os.path.join(mg.HERE, name + ".npz")
    data = dict(np.load(path))
    for k, v in data.items():
        if v.dtype == np.float32 and np.array_equal(v.astype(np.float16).astype(np.float32), v, equal_nan=True):
            data[k] = v.astype(np.float16)
    np.savez_compressed(path, **data)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    ref, refw = mg.load_reference()
    mg.run_case(ref, refw, "base224_fp16", "vit_base_patch16_224", mg.README_SCHEDULE, 2, 2, 0.04, 0.02, torch.float16)
    compact("base224_fp16")


if __name__ == "__main__":
    main()
