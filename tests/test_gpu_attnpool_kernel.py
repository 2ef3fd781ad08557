"""rajni_attention_pool (include/rajni_hip_attnpool.h) alone, through the C ABI into guarded buffers.  GPU box only (`-m gpu`).

Yardstick: tests/numerics_attnpool.py::pool_attention_budget - the attention restated in fp64 and a per-element budget derived
from the arithmetic (fp32 logits, softmax and weighted sum in some fixed order, one rounding of the output), in the style of
tests/numerics.py::attention_budget.  Shapes: N = 1 (a softmax of one token), 9, 16, 17 (one token past a round count) and 625
(several passes of every token slot: the workgroup holds 16 .. 256 slots, by head dim); head dims 64 (a 128-byte line per row),
80 (10-lane groups, idle lanes), 128 and 8 (one lane per row); B = 1 and 5."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import numerics as nm
import numerics_attnpool as na
from guarded import Guarded
from rajni_amd import _native as nat
from rajni_amd import ops

DEV = "cuda"
TORCH = nm.TORCH
NS = [1, 9, 16, 17, 625]
HEADS = [(2, 64), (4, 80), (1, 128), (3, 8)]


def launch(kv, q, dt, check=True):
    """kv [B, N, 2C] and q [H, D] numpy -> (out [B, C] torch on the device, its bits): every operand guarded"""
    B, N, _ = kv.shape
    H, D = q.shape
    gkv = Guarded(kv.shape, TORCH[dt], DEV).fill_(torch.from_numpy(kv))
    gq = Guarded(q.shape, torch.float32, DEV).fill_(torch.from_numpy(q))
    out = Guarded((B, H * D), TORCH[dt], DEV)
    nat.check(nat.lib().rajni_attention_pool(gkv.ptr(), gq.ptr(), out.ptr(), B, N, H, D, nat.dtype_code(TORCH[dt]),
                                             nat.stream_ptr(torch.device(DEV))), "rajni_attention_pool")
    torch.cuda.synchronize()
    if check:
        what = f"attention_pool B={B} N={N} H={H} D={D} {dt}"
        gkv.check(what + ": kv", written=False)
        gq.check(what + ": q", written=False)
        out.check(what + ": out")
    return out.t.clone()


def bits(t):
    return t.contiguous().view(torch.uint8)


@pytest.mark.parametrize("H,D", HEADS)
@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_the_pool_meets_its_budget_at_every_token_count(dt, H, D):
    for kind in na.KV_KINDS:
        for N in NS:
            for B in (1, 5):
                kv, q = na.pool_operands(kind, B, N, H, D, dt)
                want, bud = na.pool_attention_budget(kv, q, dt)
                got = launch(kv, q, dt).float().cpu().numpy()
                nm.assert_within(got, want, bud, f"attention_pool {kind} {dt} B={B} N={N} H={H} D={D}")
                if kind == "equal":      # all logits equal: the plain mean of V, within the same budget
                    mean = kv.reshape(B, N, 2, H * D)[:, :, 1].astype(np.float64).mean(axis=1)
                    nm.assert_within(got, mean, bud, f"attention_pool equal logits = the mean, {dt} B={B} N={N} H={H} D={D}")
                if N == 1:               # one token: the output is its V row, exactly (softmax = 1, one rounding of a dt value)
                    assert np.array_equal(got, kv[:, 0, H * D:])


@pytest.mark.parametrize("H,D", HEADS)
@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_an_image_has_the_same_bits_at_any_batch_size_and_position(dt, H, D):
    for N in (17, 625):
        kv, q = na.pool_operands("normal", 5, N, H, D, dt, seed=3)
        kv[4] = kv[0]
        out5 = launch(kv, q, dt)
        out1 = launch(kv[:1].copy(), q, dt)
        assert torch.equal(bits(out5[0]), bits(out5[4])), f"positions 0 and 4 differ ({dt} N={N} H={H} D={D})"
        assert torch.equal(bits(out5[0]), bits(out1[0])), f"B = 1 and B = 5 differ ({dt} N={N} H={H} D={D})"
        assert not torch.equal(bits(out5[0]), bits(out5[1]))
        # and the same launch again: no atomics, no order that depends on timing
        assert torch.equal(bits(launch(kv, q, dt, check=False)), bits(out5))


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_the_tensor_level_op_is_the_entry_point(dt):
    kv, q = na.pool_operands("normal", 3, 33, 2, 64, dt, seed=1)
    got = ops.attention_pool(torch.from_numpy(kv).to(DEV).to(TORCH[dt]), torch.from_numpy(q).to(DEV))
    assert got.dtype == TORCH[dt] and tuple(got.shape) == (3, 128)
    assert torch.equal(bits(got), bits(launch(kv, q, dt)))
    with pytest.raises(ValueError, match="float32"):
        ops.attention_pool(torch.from_numpy(kv).to(DEV).to(TORCH[dt]), torch.from_numpy(q).to(DEV).half())
    with pytest.raises(ValueError, match=r"2 \* H \* D"):
        ops.attention_pool(torch.from_numpy(kv).to(DEV).to(TORCH[dt])[:, :, :128], torch.from_numpy(q).to(DEV))


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_misaligned_pointers_are_refused_as_the_placement_table_states(dt):
    """kv 16, q 16, out 16: each pointer one element past a 16-byte boundary is refused by name and nothing is launched (the
    output keeps its poison)"""
    kv, q = na.pool_operands("normal", 2, 9, 2, 64, dt)
    es = 4 if dt == "fp32" else 2
    gkv = Guarded(kv.shape, TORCH[dt], DEV).fill_(torch.from_numpy(kv))
    gq = Guarded(q.shape, torch.float32, DEV).fill_(torch.from_numpy(q))
    out = Guarded((2, 128), TORCH[dt], DEV)
    lib, code, s = nat.lib(), nat.dtype_code(TORCH[dt]), nat.stream_ptr(torch.device(DEV))
    for args, word in (((gkv.ptr() + es, gq.ptr(), out.ptr()), "kv must be 16-byte aligned"),
                       ((gkv.ptr(), gq.ptr() + 4, out.ptr()), "q must be 16-byte aligned"),
                       ((gkv.ptr(), gq.ptr(), out.ptr() + es), "out must be 16-byte aligned")):
        assert lib.rajni_attention_pool(*args, 2, 9, 2, 64, code, s) == 1
        assert word in lib.rajni_last_error().decode()
    torch.cuda.synchronize()
    assert out.unwritten() == 2 * 128 and out.guard_damage() is None
    nat.check(lib.rajni_attention_pool(gkv.ptr(), gq.ptr(), out.ptr(), 2, 9, 2, 64, code, s), "rajni_attention_pool")
    torch.cuda.synchronize()
    out.check("attention_pool after the refusals")
