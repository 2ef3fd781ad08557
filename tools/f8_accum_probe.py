#!/usr/bin/env python3
"""How exactly does the fp8 matrix instruction (v_mfma_f32_16x16x128_f8f6f4, unscaled form) add its 128 products?
GPU box.  python tools/f8_accum_probe.py

Runs rajni_linear's fp8 x fp8 kernel on e4m3 codes drawn UNIFORMLY (magnitudes log-uniform over 2^-9 .. 448 within a row - the
worst case for an adder of limited width, and nothing a quantised LayerNorm or weight row looks like) with unit scales, K = 512
of which only the first `blocks` * 128 columns are non-zero, through the RESID epilogue on a zero fp32 residual: the output
IS the fp32 accumulator.  Every product and the exact sum are representable in fp64, so the error is known exactly.

Recorded on an MI355X: one instruction is off by up to 3400 * 2^-24 * sum|products| (2.0e-4 relative to the
sum of magnitudes; about 2^-11 of the largest product, either sign), four chained instructions by up to 1100 * 2^-24 * sum;
an fp32 chain of round-to-nearest adds stays below 128 * 2^-24 * sum.  Not e4m3-subnormal flushing (checked by flushing them
in the reference), not a truncation of each product to a fixed grid below the largest one.
tests/test_gpu_numerics.py::test_fp8_matrix_instruction_accumulation_as_recorded pins these figures."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rajni-vit_amd"))
import numpy as np
import torch
from rajni_amd import ops, _native as nat


def run(blocks=1, seed=0, M=256, N=256, K=512):
    """returns {"err_over_u32S": max |err| / (2^-24 sum|products|), "err_over_maxprod": max |err| / largest |product|,
    "exactly_rounded": fraction of outputs equal to the correctly rounded exact sum}"""
    rng = np.random.default_rng([seed, blocks])

    def codes(shape):
        c = rng.integers(0, 256, size=shape, dtype=np.uint8)
        c[(c & 0x7F) == 0x7F] = 0x38                      # no NaN patterns
        c[:, 128 * blocks:] = 0
        return c

    xq, wq = codes((M, K)), codes((N, K))
    f64 = lambda c: torch.from_numpy(c).view(torch.float8_e4m3fn).to(torch.float32).numpy().astype(np.float64)
    x, w = f64(xq), f64(wq)
    exact, S = x @ w.T, np.abs(x) @ np.abs(w).T
    wp = np.zeros(((N + 255) // 256 * 256, K), np.uint8)
    wp[:N] = wq
    t = lambda a: torch.from_numpy(a).to("cuda")
    r = torch.zeros(1, M, N, device="cuda")
    y = ops.linear(t(xq).reshape(1, M, K), t(wp), N, None, nat.EPI_BIAS_RESID, resid=r, out=r.reshape(M, N),
                   w_scale=t(np.ones(N, np.float32)), x_scale=t(np.ones(M, np.float32)))
    got = y.reshape(M, N).cpu().numpy().astype(np.float64)
    pm = np.zeros_like(exact)
    for k in range(128 * blocks):
        pm = np.maximum(pm, np.abs(np.outer(x[:, k], w[:, k])))
    e = np.abs(got - exact)
    return {"err_over_u32S": float((e / (2.0 ** -24 * S)).max()), "err_over_maxprod": float((e / pm).max()),
            "exactly_rounded": float(np.mean(got == exact.astype(np.float32).astype(np.float64)))}


if __name__ == "__main__":
    for blocks in (1, 4):
        r = run(blocks)
        print(f"{blocks} instruction(s): max |err| = {r['err_over_u32S']:.0f} * 2^-24 sum|products| = 2^{np.log2(r['err_over_maxprod']):.2f} of the "
              f"largest product; {100 * r['exactly_rounded']:.2f} % of the outputs are the correctly rounded sum")
