"""rajni_rope_qk (include/rajni_hip_rope.h) alone, through the C ABI.  GPU box only (`-m gpu`).

Every element is held to the derived budget of tests/numerics_rope.py::rope_budget - two fp32 products and one add in any order
or contraction, then one rounding:  |err| <= UNIT[dt] |want| + 2 U32 (|x cos| + |x' sin|) + FLOOR[dt]  - and every case asserts
bit for bit that the v third and all prefix rows are what they were.  Tables are random in [-1, 1], not sines: no trigonometric
identity hides a swapped table.  The launch has ONE form (one wave per patch token at every size), so there is no threshold
between forms to sit on; the shapes are the smallest that reach each way the kernel can go wrong:
  head dims   8 (half layout: the partner inside the lane's own chunk), 24 and 40 (the partner runs straddle a 16-byte chunk
              boundary; 3 and 5 of a slot's lanes busy), 64 (a head is one 128-byte line), 128 (16 lanes per head), both layouts
  heads       1, 3, 12 (fewer heads than a wave has slots, and more: a second batch of the head walk at D = 128)
  rows        (B, N, P) = (1, 2, 1), (3, 7, 0), (2, 21, 5), (5, 197, 1): none fills a workgroup of four tokens evenly
  source map  NULL, and a strict sub-selection of a larger grid in non-identity order, different per image
  tables      one for all heads, and one per head."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bigmem as bm
import numerics as nm
import numerics_rope as nrp
from guarded import Guarded
from rajni_amd import _native as nat
from rajni_amd import ops

DEV = "cuda"
F32 = np.float32
CODE = {"bf16": nat.RAJNI_BF16, "fp16": nat.RAJNI_F16, "fp32": nat.RAJNI_F32}
DIMS = [8, 24, 40, 64, 128]
HEADS = [1, 3, 12]
ROWS = [(1, 2, 1), (3, 7, 0), (2, 21, 5), (5, 197, 1)]


def make_case(B, N, P, H, D, dt, mapped, per_head, seed=0):
    """(qkv [B, N, 3, H, D] values of `dt`, src [B, N] or None, cos, sin fp32 [rows, D] or [H, rows, D])"""
    rng = np.random.default_rng([seed, B, N, P, H, D, int(mapped), int(per_head)])
    qkv = nm.round_to(rng.standard_normal((B, N, 3, H, D), dtype=F32) * 2.0, dt)
    n = N - P
    rows = 2 * n + 3 if mapped else n
    src = None
    if mapped:      # a strict sub-selection of the larger grid, in non-identity order, per image
        src = np.zeros((B, N), np.int32)
        src[:, :P] = np.arange(P)
        for b in range(B):
            src[b, P:] = P + rng.permutation(rows)[:n]
    shape = (H, rows, D) if per_head else (rows, D)
    cos = rng.uniform(-1, 1, shape).astype(F32)
    sin = rng.uniform(-1, 1, shape).astype(F32)
    return qkv, src, cos, sin


def launch(qkv, src, cos, sin, head_stride, B, N, P, H, D, layout, dt):
    """qkv, src (or None), cos, sin: device tensors or Guarded buffers - the OBJECTS, so that each stays alive until the kernel
    has finished (the pointer of a temporary names memory the allocator hands to the next allocation)"""
    ptr = lambda o: None if o is None else (o.ptr() if isinstance(o, Guarded) else o.data_ptr())
    rc = nat.lib().rajni_rope_qk(ptr(qkv), ptr(src), ptr(cos), ptr(sin), head_stride, B, N, P, H, D, layout, CODE[dt],
                                 nat.stream_ptr(torch.device(DEV)))
    nat.check(rc, "rajni_rope_qk")
    torch.cuda.synchronize()


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def check_result(got_t, before_t, qkv, src, cos, sin, P, layout, dt, what):
    """budget on q and k of the patch rows; v and the prefix rows bit for bit what they were"""
    assert torch.equal(bits(got_t[:, :, 2]), bits(before_t[:, :, 2])), f"{what}: the v third changed"
    assert torch.equal(bits(got_t[:, :P]), bits(before_t[:, :P])), f"{what}: a prefix row changed"
    want, bud = nrp.rope_qkv(qkv, cos, sin, P, layout, src, dt)
    got = got_t.float().cpu().numpy().astype(np.float64)
    nm.assert_within(got[:, P:, :2], want[:, P:, :2], bud[:, P:, :2], what)


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("layout", [nrp.INTERLEAVED, nrp.HALF], ids=["interleaved", "half"])
@pytest.mark.parametrize("D", DIMS)
def test_rotation_within_the_derived_budget(D, layout, dt):
    for H, (B, N, P), mapped, per_head in itertools.product(HEADS, ROWS, (False, True), (False, True)):
        qkv, src, cos, sin = make_case(B, N, P, H, D, dt, mapped, per_head)
        x = dev(qkv, nm.TORCH[dt])
        before = x.clone()
        s, c, sn = (dev(src) if mapped else None), dev(cos), dev(sin)
        launch(x, s, c, sn, cos.shape[-2] * D if per_head else 0, B, N, P, H, D, layout, dt)
        check_result(x, before, qkv, src, cos, sin, P, layout, dt,
                     f"rope D={D} layout={layout} {dt} H={H} (B,N,P)={(B, N, P)} src={'map' if mapped else 'NULL'} "
                     f"tables={'per head' if per_head else 'shared'}")


def test_the_two_layouts_are_different_functions():
    # (a kernel that ignored `layout` would pass one of the two parametrisations above only by luck: say it outright)
    B, N, P, H, D, dt = 2, 21, 5, 3, 24, "fp32"
    qkv, src, cos, sin = make_case(B, N, P, H, D, dt, True, False)
    outs = []
    for layout in (nrp.INTERLEAVED, nrp.HALF):
        x = dev(qkv)
        launch(x, dev(src), dev(cos), dev(sin), 0, B, N, P, H, D, layout, dt)
        outs.append(x)
    assert not torch.equal(bits(outs[0]), bits(outs[1]))


@pytest.mark.parametrize("layout", [nrp.INTERLEAVED, nrp.HALF], ids=["interleaved", "half"])
@pytest.mark.parametrize("D,dt", [(40, "bf16"), (64, "fp16"), (24, "fp32")])
def test_guarded_buffers_come_back_intact(D, dt, layout):
    B, N, P, H = 2, 21, 5, 3
    qkv, src, cos, sin = make_case(B, N, P, H, D, dt, True, True)
    x = Guarded((B * N, 3 * H * D), nm.TORCH[dt], device=DEV).fill_(torch.from_numpy(qkv.reshape(B * N, -1)))
    c = Guarded(cos.reshape(-1, D).shape, torch.float32, device=DEV).fill_(torch.from_numpy(cos.reshape(-1, D)))
    sn = Guarded(sin.reshape(-1, D).shape, torch.float32, device=DEV).fill_(torch.from_numpy(sin.reshape(-1, D)))
    s = Guarded((B, N), torch.int32, device=DEV, fill_int32=P).fill_(torch.from_numpy(src))      # (the arena holds a valid position)
    before = x.t.clone().reshape(B, N, 3, H, D)
    arenas = [g.arena.clone() for g in (c, sn, s)]
    launch(x, s, c, sn, cos.shape[-2] * D, B, N, P, H, D, layout, dt)
    for g, name in ((x, "qkv"), (c, "cos"), (sn, "sin"), (s, "src")):
        g.check(f"rope guarded D={D} {dt}: {name}", written=False)
    for g, a, name in zip((c, sn, s), arenas, ("cos", "sin", "src")):
        assert torch.equal(g.arena, a), f"{name} was written"
    check_result(x.t.reshape(B, N, 3, H, D), before, qkv, src, cos, sin, P, layout, dt, f"rope guarded D={D} {dt}")


@pytest.mark.parametrize("layout", [nrp.INTERLEAVED, nrp.HALF], ids=["interleaved", "half"])
def test_minimum_alignment_gives_the_same_bits(layout):
    # every pointer 16 bytes (src: 4) past a 256-byte boundary - the contract's minimum - against every pointer on one
    B, N, P, H, D, dt = 3, 7, 0, 3, 40, "bf16"
    qkv, src, cos, sin = make_case(B, N, P, H, D, dt, True, False)
    outs = []
    for mis in (0, 16):
        kw = dict(misalign=mis, align=16) if mis else {}
        kws = dict(misalign=4, align=4) if mis else {}
        x = Guarded((B * N, 3 * H * D), nm.TORCH[dt], device=DEV, **kw).fill_(torch.from_numpy(qkv.reshape(B * N, -1)))
        c = Guarded(cos.shape, torch.float32, device=DEV, **kw).fill_(torch.from_numpy(cos))
        sn = Guarded(sin.shape, torch.float32, device=DEV, **kw).fill_(torch.from_numpy(sin))
        s = Guarded((B, N), torch.int32, device=DEV, fill_int32=P, **kws).fill_(torch.from_numpy(src))
        assert x.ptr() % 256 == mis and c.ptr() % 256 == mis and s.ptr() % 256 == (4 if mis else 0)
        launch(x, s, c, sn, 0, B, N, P, H, D, layout, dt)
        for g in (x, c, sn, s):
            g.check(f"rope at {mis} bytes past a 256-byte boundary", written=False)
        outs.append(x.t.clone())
    assert torch.equal(bits(outs[0]), bits(outs[1]))


def test_python_binding_and_its_checks():
    B, N, P, H, D = 2, 21, 5, 3, 24
    qkv, src, cos, sin = make_case(B, N, P, H, D, "bf16", True, True)
    x = dev(qkv.reshape(B, N, 3 * H * D), torch.bfloat16)
    before = x.clone().reshape(B, N, 3, H, D)
    assert ops.rope_qk(x, H, dev(cos), dev(sin), num_prefix=P, src=dev(src), half=True) is x
    torch.cuda.synchronize()
    check_result(x.reshape(B, N, 3, H, D), before, qkv, src, cos, sin, P, nrp.HALF, "bf16", "ops.rope_qk")
    bad = src.copy()
    bad[1, N - 1] = P + cos.shape[-2]
    with pytest.raises(ValueError, match="outside the tables"):
        ops.rope_qk(x, H, dev(cos), dev(sin), num_prefix=P, src=dev(bad))
    with pytest.raises(ValueError, match="patch rows but the tables"):
        ops.rope_qk(x, H, dev(cos[:, :3]), dev(sin[:, :3]), num_prefix=P)


@pytest.fixture
def big():
    torch.cuda.synchronize()
    b = bm.Big(DEV)
    yield b
    torch.cuda.synchronize()
    b.close()


@pytest.mark.parametrize("layout", [nrp.INTERLEAVED, nrp.HALF], ids=["interleaved", "half"])
def test_offsets_past_2_31_elements(big, layout):
    # rows * 3 * H * D > 2^31 elements (and > 2^32 bytes of bf16): the first and the last 64 rows against the rule, the whole v
    # third compared on the device.  Rows repeat with a prime period and the source map walks a small table with another
    # stride, so an offset that wrapped would land on another phase of both
    B, P, H, D, dt = 2, 1, 12, 64, "bf16"
    ld = 3 * H * D
    N = -(-(bm.T31 + ld) // (B * ld)) + 1
    rows_total = B * N
    bm.assert_crosses_all(rows_total * ld, 2, "rope qkv")
    T = 4099 - 64                                           # table rows: not the period of the fill
    rng = np.random.default_rng(7)
    block = nm.round_to(rng.standard_normal((bm.PERIOD, ld), dtype=F32) * 2.0, dt)
    cos, sin = rng.uniform(-1, 1, (T, D)).astype(F32), rng.uniform(-1, 1, (T, D)).astype(F32)
    x = big.dense((rows_total, ld), torch.bfloat16)
    blk = torch.from_numpy(block).to(DEV).to(torch.bfloat16)
    bm.periodic_fill(x, blk)
    t = torch.arange(N, device=DEV, dtype=torch.int64)
    src = (P + (t * 7 + torch.arange(B, device=DEV, dtype=torch.int64)[:, None] * 13) % T).to(torch.int32)
    src[:, :P] = torch.arange(P, device=DEV, dtype=torch.int32)
    launch(x, src, dev(cos), dev(sin), 0, B, N, P, H, D, layout, dt)
    src_h = src.cpu().numpy()
    for lo, hi in ((0, 64), (rows_total - 64, rows_total)):
        r = np.arange(lo, hi)
        b, tok = r // N, r % N
        orig = block[r % bm.PERIOD].reshape(-1, 3, H, D).astype(np.float64)
        got = x[lo:hi].float().cpu().numpy().astype(np.float64).reshape(-1, 3, H, D)
        patch = tok >= P
        p = src_h[b, tok] - P
        want, bud = nrp.rope_budget(orig[patch][:, :2], cos[p[patch]][:, None, None, :], sin[p[patch]][:, None, None, :], layout, dt)
        nm.assert_within(got[patch][:, :2], want, bud, f"rope rows {lo}..{hi} of {rows_total}")
        np.testing.assert_array_equal(got[~patch], orig[~patch])
        np.testing.assert_array_equal(got[:, 2], orig[:, 2])
    vb = bits(blk[:, 2 * H * D:])
    step = bm.PERIOD * 16
    bad = torch.zeros((), dtype=torch.bool, device=DEV)
    for r0 in range(0, rows_total, step):
        r1 = min(rows_total, r0 + step)
        idx = torch.arange(r0, r1, device=DEV) % bm.PERIOD
        bad |= (bits(x[r0:r1, 2 * H * D:]) != vb[idx]).any()
    assert not bool(bad), "the v third changed somewhere in the buffer"
