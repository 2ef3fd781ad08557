"""rajni_hidden_norm (include/rajni_hip_mlpnorm.h) on the device, through ops.hidden_norm: the norm over the first n columns of
the rows of the MLP's hidden buffer, in place.  GPU box only (`-m gpu`).

Yardstick: tests/numerics_eva.py::hidden_norm_budget - the fp64 rule and a per-element budget derived from the row's own magnitudes
(tests/test_eva_cpu.py holds the kernel's numpy restatement inside it and the one-pass and divisor-ld mutants outside it).
Every case also holds: the padding columns [n, ld) are +0 afterwards, bit for bit; the guard bytes around the buffer, the weight and
the bias are untouched (tests/guarded.py); a row normalised alone has the bits it has as row 200 of 259."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import numerics as nm
import numerics_eva as ne
from guarded import Guarded
from rajni_amd import _native as nat
from rajni_amd import ops

DEV = "cuda"
TORCH = nm.TORCH
EPS = 1e-6
ROWS = (1, 5, 259)                                   # one wave; a workgroup and a wave of the next; the wave and block tails
WIDTHS = (8, 342, 344, 2048, 2730, ne.CAP)           # one chunk; a partial last chunk; whole chunks short of the K step; each chunk count


def run(x_np, w, b, n, dt, rms):
    """the kernel on guarded copies of x [rows, ld] (values of dt), w and b; (result as fp64 [rows, ld], raw result tensor)"""
    rows, ld = x_np.shape
    gx = Guarded((rows, ld), TORCH[dt], DEV).fill_(torch.from_numpy(x_np))
    gw = Guarded((n,), torch.float32, DEV, align=16).fill_(torch.from_numpy(w))
    gb = Guarded((n,), torch.float32, DEV, align=16).fill_(torch.from_numpy(b)) if b is not None else None
    out = ops.hidden_norm(gx.t, gw.t, gb.t if gb is not None else None, EPS, n=n, rms=rms)
    torch.cuda.synchronize()
    assert out.data_ptr() == gx.t.data_ptr()
    for g, what in ((gx, "x"), (gw, "w"), (gb, "b")):
        if g is not None:
            g.check(f"hidden_norm {what} rows={rows} n={n} {dt}", written=True)
    return gx.t.double().cpu().numpy(), gx.t.clone()


def bits(t):
    return t.contiguous().view(torch.uint8)


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("n", WIDTHS)
def test_hidden_norm_against_the_derived_budget(n, dt):
    ld = (n + 63) // 64 * 64
    x_all, names, w, b = ne.kernel_rows(259, n, ld, dt, seed=3)
    x_all[7, :n] = 3.25                               # sums of it are exact in fp32: the mean is 3.25, every deviation 0
    worst = 0.0
    for kind in ("layernorm", "rms"):
        for bias in (b, None):
            row200 = None
            for rows in ROWS[::-1]:
                x = x_all[:rows] if rows != 1 else x_all[200:201]
                got, raw = run(x, w, bias, n, dt, kind == "rms")
                want, bud = ne.hidden_norm_budget(x, w, bias, EPS, n, kind, dt)
                what = f"hidden_norm {kind} rows={rows} n={n} ld={ld} {dt} b={'yes' if bias is not None else 'no'}"
                # the padding columns: +0, every bit
                assert int(bits(raw[:, n:]).count_nonzero()) == 0, what
                ratio, at = nm.worst_ratio(got[:, :n], want[:, :n], bud[:, :n])
                worst = max(worst, ratio)
                assert ratio <= 1.0, f"{what}: err / budget {ratio:.3g} at row {at // n} ({names[at // n] if rows != 1 else names[200]}) column {at % n}"
                if rows == 259:
                    row200 = raw[200:201].clone()
                    # the rows with a large mean and a small spread, on their own
                    big = names == "big_mean"
                    assert nm.worst_ratio(got[big][:, :n], want[big][:, :n], bud[big][:, :n])[0] <= 1.0, what
                    if kind == "layernorm":      # zero variance, eps alone under the root: b (0 without one), exactly
                        const = nm.round_to(np.zeros(n, np.float32) if bias is None else bias, dt)
                        np.testing.assert_array_equal(got[7, :n], const.astype(np.float64), err_msg=what)
                if rows == 1:                    # the same row, alone in its launch
                    assert torch.equal(bits(raw), bits(row200)), what
    print(f"[hidden_norm] n={n} {dt}: worst err / budget {worst:.3f}")


def test_a_width_over_the_cap_is_refused_with_the_cap_in_the_message():
    n = ne.CAP + 8
    x = torch.zeros((2, n + 56), dtype=torch.bfloat16, device=DEV)
    w = torch.ones(n, dtype=torch.float32, device=DEV)
    with pytest.raises(NotImplementedError, match=rf"a width of {n} is over the cap of {ne.CAP} columns"):
        ops.hidden_norm(x, w, None, EPS)
    torch.cuda.synchronize()
    assert int(x.count_nonzero()) == 0
    with pytest.raises(nat.NativeError, match="ld must be at least n and a multiple of 8"):
        ops.hidden_norm(torch.zeros((2, 12), dtype=torch.bfloat16, device=DEV), torch.ones(12, dtype=torch.float32, device=DEV), None, EPS)
