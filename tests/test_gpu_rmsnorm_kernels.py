"""rajni_norm_rows and rajni_embed_norm (include/rajni_hip_norm.h) alone, through the C ABI into guarded buffers
(tests/guarded.py).  GPU box only (`-m gpu`).

Every result is held to the per-element budgets of tests/numerics_rmsnorm.py - |err| <= u_out |want| + c_rms u32 max|w| |n|, the
constant measured on two references and never on the kernel - on the stress rows of numerics.layernorm_rows, every guard zone
must come back intact, every input unchanged, and b is NULL wherever the kind is RMS."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import numerics as nm
import numerics_rmsnorm as nr
from guarded import Guarded
from rajni_amd import _native as nat

DEV = "cuda"
F32 = np.float32
CODE = {"bf16": nat.RAJNI_BF16, "fp16": nat.RAJNI_F16, "fp32": nat.RAJNI_F32}
EPS = nr.EPS


def arena(a, dt, **kw):
    a = np.asarray(a, F32)
    return Guarded(a.shape, nm.TORCH[dt], device=DEV, **kw).fill_(torch.from_numpy(a))


def out_arena(shape, dt, **kw):
    return Guarded(shape, nm.TORCH[dt], device=DEV, **kw)


def host(t):
    return t.float().cpu().numpy().astype(np.float64)


def bits(g):
    return g.arena.clone()


def norm_rows(kind, x, w, b, y, rows, C, out_dt, x_f32, stride=None, eps=EPS):
    rc = nat.lib().rajni_norm_rows(kind, x.ptr(), stride or C, w.ptr(), b.ptr() if b is not None else None, y.ptr(), rows, C, eps,
                                   CODE[out_dt], int(x_f32), nat.stream_ptr(torch.device(DEV)))
    nat.check(rc, "rajni_norm_rows")
    torch.cuda.synchronize()


FORMS = [("bf16", False), ("bf16", True), ("fp16", False), ("fp16", True), ("fp32", False)]     # (output type, fp32 rows in)


@pytest.mark.parametrize("out_dt,x_f32", FORMS, ids=[f"{d}{'_f32in' if f else ''}" for d, f in FORMS])
@pytest.mark.parametrize("C", nr.RMS_C)
@pytest.mark.parametrize("rows", nm.LN_ROW_COUNTS)
def test_rms_rows_budget_in_guarded_buffers(rows, C, out_dt, x_f32):
    in_dt = "fp32" if x_f32 else out_dt
    xv, names, wv, _ = nm.layernorm_rows(rows, C, in_dt)
    want, bud = nr.rmsnorm_budget(xv, wv, EPS, out_dt)
    x, w, y = arena(xv, in_dt), arena(wv, "fp32"), out_arena((rows, C), out_dt)
    before = bits(x), bits(w)
    norm_rows(nat.NORM_RMS, x, w, None, y, rows, C, out_dt, x_f32)
    y.check(f"rms rows {rows}x{C} {in_dt}->{out_dt}: y")
    assert torch.equal(bits(x), before[0]) and torch.equal(bits(w), before[1]), "an input was written"
    got = host(y.t)
    for case in sorted(set(names)):
        sel = names == case
        nm.assert_within(got[sel], want[sel], bud[sel], f"rms rows {case} {rows}x{C} {in_dt}->{out_dt}")


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_rms_strided_cls_rows(dt):
    rows, C, N = 77, 768, 5
    xv, names, wv, _ = nm.layernorm_rows(rows, C, dt)
    x3 = np.random.default_rng(0).standard_normal((rows, N, C), dtype=F32)
    x3[:, 0] = xv
    want, bud = nr.rmsnorm_budget(xv, wv, EPS, dt)
    x, w, y = arena(x3.reshape(rows, N * C), dt), arena(wv, "fp32"), out_arena((rows, C), dt)
    norm_rows(nat.NORM_RMS, x, w, None, y, rows, C, dt, False, stride=N * C)
    y.check(f"rms strided {dt}: y")
    nm.assert_within(host(y.t), want, bud, f"rms strided CLS rows {dt}")


@pytest.mark.parametrize("out_dt,x_f32", FORMS, ids=[f"{d}{'_f32in' if f else ''}" for d, f in FORMS])
@pytest.mark.parametrize("rows", nm.LN_ROW_COUNTS)
def test_kind_layernorm_gives_the_bits_of_rajni_layernorm(rows, out_dt, x_f32):
    C = 768
    in_dt = "fp32" if x_f32 else out_dt
    xv, names, wv, bv = nm.layernorm_rows(rows, C, in_dt)
    x, w, b = arena(xv, in_dt), arena(wv, "fp32"), arena(bv, "fp32")
    y0, y1 = out_arena((rows, C), out_dt), out_arena((rows, C), out_dt)
    rc = nat.lib().rajni_layernorm(x.ptr(), C, w.ptr(), b.ptr(), y0.ptr(), rows, C, 1e-6, CODE[out_dt], int(x_f32),
                                   nat.stream_ptr(torch.device(DEV)))
    nat.check(rc, "rajni_layernorm")
    norm_rows(nat.NORM_LAYERNORM, x, w, b, y1, rows, C, out_dt, x_f32, eps=1e-6)
    y1.check("kind LAYERNORM: y")
    assert torch.equal(y0.t.contiguous().view(torch.uint8), y1.t.contiguous().view(torch.uint8))
    # ... and the RMS form of the same launch is another function of the same rows
    norm_rows(nat.NORM_RMS, x, w, None, y1, rows, C, out_dt, x_f32, eps=1e-6)
    assert not torch.equal(y0.t.contiguous().view(torch.uint8), y1.t.contiguous().view(torch.uint8))


def test_rms_rows_do_not_depend_on_the_batch_around_them():
    # the same row at another position of another launch, on either side of the two-rows-per-wave switch: the same bits
    C = 1024
    xv, _, wv, _ = nm.layernorm_rows(4109, C, "fp32")
    w = arena(wv, "fp32")
    y_all, y_few = out_arena((4109, C), "bf16"), out_arena((77, C), "bf16")
    norm_rows(nat.NORM_RMS, arena(xv, "fp32"), w, None, y_all, 4109, C, "bf16", True)
    norm_rows(nat.NORM_RMS, arena(xv[4000:4077], "fp32"), w, None, y_few, 77, C, "bf16", True)
    assert torch.equal(y_all.t[4000:4077].contiguous().view(torch.uint8), y_few.t.contiguous().view(torch.uint8))


# ---- rajni_embed_norm ------------------------------------------------------------------------------------------------------

def embed_case(B, P, n, C, stream_dt, pos_dt, pos_off, seed=0):
    rng = np.random.default_rng([seed, B, P, n, C])
    x = rng.standard_normal((B, P + n, C), dtype=F32) * 1.5 + 0.75
    x[:, :, ::7] += 3.0
    x[0, P] *= 1e-3                                         # a tiny row, an offset row and a large row among the patches
    x[-1, -1] = 100.0 + 0.1 * x[-1, -1]
    x[B // 2, P + n // 2] *= 300.0
    w = (1 + 0.1 * rng.standard_normal(C)).astype(F32)
    b = (0.1 * rng.standard_normal(C)).astype(F32)
    pos = (0.5 + 0.3 * rng.standard_normal((pos_off + n, C))).astype(F32)
    return nm.round_to(x, stream_dt), w, b, nm.round_to(pos, pos_dt)


def embed_norm(kind, x, w, b, pos, pos_off, B, N, P, C, dt, x_f32):
    rc = nat.lib().rajni_embed_norm(kind, x.ptr(), w.ptr(), b.ptr() if b is not None else None, pos.ptr(), pos_off, B, N, P, C, EPS,
                                    CODE[dt], int(x_f32), nat.stream_ptr(torch.device(DEV)))
    nat.check(rc, "rajni_embed_norm")
    torch.cuda.synchronize()


STREAMS = [("bf16", False), ("bf16", True), ("fp16", False), ("fp32", False)]     # (model dtype, fp32 stream)


@pytest.mark.parametrize("dt,x_f32", STREAMS, ids=[f"{d}{'_f32stream' if f else ''}" for d, f in STREAMS])
@pytest.mark.parametrize("kind", ["rms", "layernorm"])
@pytest.mark.parametrize("C", [128, 320, 1280])
@pytest.mark.parametrize("n", [16, 17])
@pytest.mark.parametrize("P", [0, 1, 5])
def test_embed_norm_budget_and_untouched_prefix_rows(P, n, C, kind, dt, x_f32):
    B = 3
    stream_dt = "fp32" if x_f32 else dt
    for pos_off in sorted({0, P}):
        xv, wv, bv, pv = embed_case(B, P, n, C, stream_dt, dt, pos_off)
        x, w, pos = arena(xv.reshape(B * (P + n), C), stream_dt), arena(wv, "fp32"), arena(pv, dt)
        b = arena(bv, "fp32") if kind == "layernorm" else None
        before = bits(w), bits(pos)
        prefix_before = x.t.reshape(B, P + n, C)[:, :P].clone()
        embed_norm(nat.NORM_RMS if kind == "rms" else nat.NORM_LAYERNORM, x, w, b, pos, pos_off, B, P + n, P, C, dt, x_f32)
        x.check(f"embed_norm {kind} P={P} n={n} C={C} {dt}: x", written=False)
        assert torch.equal(bits(w), before[0]) and torch.equal(bits(pos), before[1]), "an input was written"
        after = x.t.reshape(B, P + n, C)
        assert torch.equal(after[:, :P].contiguous().view(torch.uint8), prefix_before.contiguous().view(torch.uint8)), "a prefix row changed"
        rows = xv[:, P:].reshape(B * n, C)
        want, bud = nr.embed_norm_budget(rows, wv, bv if kind == "layernorm" else None, np.tile(pv[pos_off:], (B, 1)), EPS, kind,
                                         stream_dt)
        nm.assert_within(host(after[:, P:]).reshape(B * n, C), want, bud, f"embed_norm {kind} P={P} n={n} C={C} {dt} off={pos_off}")


@pytest.mark.parametrize("kind", ["rms", "layernorm"])
def test_embed_norm_at_the_minimum_alignment_gives_the_same_bits(kind):
    B, P, n, C, dt = 3, 1, 17, 320, "bf16"
    xv, wv, bv, pv = embed_case(B, P, n, C, dt, dt, P)
    k = nat.NORM_RMS if kind == "rms" else nat.NORM_LAYERNORM
    outs = []
    for mis in (0, 16):
        kw = dict(misalign=mis, align=16) if mis else {}
        x = arena(xv.reshape(B * (P + n), C), dt, **kw)
        w, pos = arena(wv, "fp32", **kw), arena(pv, dt, **kw)
        b = arena(bv, "fp32", **kw) if kind == "layernorm" else None
        assert x.ptr() % 256 == mis
        embed_norm(k, x, w, b, pos, P, B, P + n, P, C, dt, False)
        x.check(f"embed_norm at {mis} bytes past a 256-byte boundary", written=False)
        outs.append(x.t.clone())
    assert torch.equal(outs[0].view(torch.uint8), outs[1].view(torch.uint8))
