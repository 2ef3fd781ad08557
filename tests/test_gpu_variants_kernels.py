"""The three kernels of csrc/variants.hip alone, through the C ABI, on the stress inputs of tests/numerics.py against fp64 numpy,
element by element (budgets: tests/numerics.py's LayerNorm budget as it stands, tests/numerics_variants.py's pool budget), inside
poisoned guard bands (tests/guarded.py).  GPU box only (`-m gpu`)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import numerics as nm
import numerics_variants as nv
from guarded import Guarded
from rajni_amd import ops

DEV = "cuda"
DTYPES = ["bf16", "fp16", "fp32"]
EPS = 1e-6
H = 3
# (token, head) groups on both sides of the one dispatch threshold (65536 groups = 10922.67 rows at 2H = 6), and a few rows
QK_ROWS = (45, nv.QK_R4_GROUPS // (2 * H), nv.QK_R4_GROUPS // (2 * H) + 1)


def dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(nm.TORCH[dt]).to(DEV)


def host(t):
    return t.float().cpu().numpy()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("D", nv.HEAD_DIMS)
def test_qk_norm_stress_rows_in_place_with_v_and_guards_untouched(D, dt):
    assert QK_ROWS[1] * 2 * H < nv.QK_R4_GROUPS <= QK_ROWS[2] * 2 * H
    big, qw, qb, kw, kb = nv.qk_norm_case(max(QK_ROWS), H, D, dt)
    C = H * D
    for rows in QK_ROWS:
        qkv = big[:rows]
        want, bud = nv.qk_norm_budget(qkv, H, D, qw, qb, kw, kb, EPS, dt)
        g = Guarded((rows, 3 * C), nm.TORCH[dt], DEV).fill_(dev(qkv, dt))
        before = g.t.clone()
        args = (H, dev(qw, "fp32"), dev(qb, "fp32"), dev(kw, "fp32"), dev(kb, "fp32"), EPS)
        ops.qk_norm(g.t, *args)
        torch.cuda.synchronize()
        g.check(f"qk_norm D={D} {dt} rows={rows}", written=False)
        got = host(g.t)
        nm.assert_within(got[:, :2 * C], want, bud, f"qk_norm D={D} {dt} rows={rows}")
        assert torch.equal(g.t[:, 2 * C:].view(torch.uint8), before[:, 2 * C:].view(torch.uint8)), "the v third changed"
        # the same input gives the same bits, whatever launch it is part of: again from the saved input, and the first
        # rows alone (a launch below the threshold) against the same rows of this one
        first = g.t.clone()
        g.t.copy_(before)
        ops.qk_norm(g.t, *args)
        assert torch.equal(g.t.view(torch.uint8), first.view(torch.uint8))
        sub = before[:7].clone()
        ops.qk_norm(sub, *args)
        assert torch.equal(sub.view(torch.uint8), first[:7].view(torch.uint8))


def test_qk_norm_without_biases_and_argument_checks():
    qkv, qw, qb, kw, kb = nv.qk_norm_case(33, 2, 64, "bf16", seed=3)
    t = dev(qkv, "bf16")
    ops.qk_norm(t, 2, dev(qw, "fp32"), None, dev(kw, "fp32"), None, EPS)
    want, bud = nv.qk_norm_budget(qkv, 2, 64, qw, np.zeros_like(qb), kw, np.zeros_like(kb), EPS, "bf16")
    nm.assert_within(host(t)[:, :256], want, bud, "qk_norm, bias-free LayerNorm")
    with pytest.raises(NotImplementedError, match="head dim"):
        ops.qk_norm(torch.zeros((4, 3 * 2 * 136), dtype=torch.bfloat16, device=DEV), 2, torch.ones(136, device=DEV), None,
                    torch.ones(136, device=DEV), None, EPS)
    with pytest.raises(ValueError, match="contiguous"):
        ops.qk_norm(t[:, :192], 1, dev(qw, "fp32"), None, dev(kw, "fp32"), None, EPS)


@pytest.mark.parametrize("stream_dt,model_dt", [("fp32", "fp32"), ("fp32", "bf16"), ("fp32", "fp16"), ("bf16", "bf16"), ("fp16", "fp16")])
@pytest.mark.parametrize("C", [128] + nm.LN_C)
def test_layernorm_stream_stress_rows_in_place(C, stream_dt, model_dt):
    for rows in nm.LN_ROW_COUNTS:
        x, _, w, b = nm.layernorm_rows(rows, C, stream_dt)
        want, bud = nm.layernorm_budget(x, w, b, EPS, stream_dt)
        g = Guarded((rows, C), nm.TORCH[stream_dt], DEV).fill_(dev(x, stream_dt))
        before = g.t.clone()
        ops.layernorm_stream(g.t, dev(w, "fp32"), dev(b, "fp32"), EPS, model_dtype=nm.TORCH[model_dt])
        torch.cuda.synchronize()
        g.check(f"layernorm_stream C={C} {stream_dt} rows={rows}")
        nm.assert_within(host(g.t), want, bud, f"layernorm_stream C={C} stream {stream_dt} model {model_dt} rows={rows}")
        first = g.t.clone()
        g.t.copy_(before)
        ops.layernorm_stream(g.t, dev(w, "fp32"), dev(b, "fp32"), EPS, model_dtype=nm.TORCH[model_dt])
        assert torch.equal(g.t.view(torch.uint8), first.view(torch.uint8))


POOL_MODES = [("avg", False, True), ("avg", True, True), ("avg", True, False), ("avg", False, False), ("token", True, True),
              ("token", False, True)]


@pytest.mark.parametrize("stream_dt,out_dt", [("fp32", "fp32"), ("fp32", "bf16"), ("fp32", "fp16"), ("bf16", "bf16"), ("fp16", "fp16")])
@pytest.mark.parametrize("Np", nv.POOL_NP)
def test_pool_norm_stress_tokens(Np, stream_dt, out_dt):
    for C in (192, 768):
        B = 3
        x, (nw, nb), (fw, fb) = nv.pool_case(B, Np, C, stream_dt)
        gx = Guarded((B, Np, C), nm.TORCH[stream_dt], DEV).fill_(dev(x, stream_dt))
        for pool, use_norm, use_fc in POOL_MODES:
            norm = (nw, nb, EPS) if use_norm else None
            fc = (fw, fb, 1e-5) if use_fc else None
            want, bud = nv.pool_norm_budget(x, pool, norm, fc, out_dt)
            dn = (dev(nw, "fp32"), dev(nb, "fp32"), EPS) if use_norm else None
            df = (dev(fw, "fp32"), dev(fb, "fp32"), 1e-5) if use_fc else None
            y = ops.pool_norm(gx.t, pool, dn, df, out_dtype=nm.TORCH[out_dt])
            torch.cuda.synchronize()
            nm.assert_within(host(y), want, bud, f"pool_norm Np={Np} C={C} {stream_dt}->{out_dt} {pool} norm={use_norm} fc_norm={use_fc}")
            again = ops.pool_norm(gx.t, pool, dn, df, out_dtype=nm.TORCH[out_dt])
            assert torch.equal(y.view(torch.uint8), again.view(torch.uint8))
            # an image's row does not depend on the images around it
            one = ops.pool_norm(gx.t[1:2].clone(), pool, dn, df, out_dtype=nm.TORCH[out_dt])
            assert torch.equal(one.view(torch.uint8), y[1:2].view(torch.uint8))
        gx.check(f"pool_norm input Np={Np} C={C}", written=False)


def test_pool_norm_output_guards_and_refusals():
    from rajni_amd import _native as nat
    B, Np, C = 5, 17, 128
    x, (nw, nb), (fw, fb) = nv.pool_case(B, Np, C, "bf16", seed=2)
    out = Guarded((B, C), torch.bfloat16, DEV)
    xd, w1, b1, w2, b2 = dev(x, "bf16"), dev(nw, "fp32"), dev(nb, "fp32"), dev(fw, "fp32"), dev(fb, "fp32")
    nat.check(nat.lib().rajni_pool_norm(xd.data_ptr(), B, Np, C, nat.POOL_AVG, w1.data_ptr(), b1.data_ptr(), EPS, w2.data_ptr(),
                                        b2.data_ptr(), 1e-5, out.ptr(), nat.RAJNI_BF16, 0, nat.stream_ptr(xd.device)), "rajni_pool_norm")
    torch.cuda.synchronize()
    out.check("pool_norm output")
    want, bud = nv.pool_norm_budget(x, "avg", (nw, nb, EPS), (fw, fb, 1e-5), "bf16")
    nm.assert_within(host(out.t), want, bud, "pool_norm into a guarded output")
    with pytest.raises(NotImplementedError, match="pool"):
        ops.pool_norm(xd, "map")
    with pytest.raises(nat.NativeError, match="patch token"):
        ops.pool_norm(xd[:, :1].contiguous(), "avg")
