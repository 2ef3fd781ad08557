"""Bounds and isolation of the *_prefix entry points of the C ABI, with poisoned inputs and guarded outputs (tests/guarded.py,
the harness of tests/test_gpu_guarded.py).  GPU box only (`-m gpu`).

The [B, P + keep] outputs are the ones a kernel that still strides by keep + 1 would overrun or leave holes in: every element
must be written, both guards intact, and the values exactly the restated rule's."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import numerics_prefix as npx
import rajni_amd
from guarded import Guarded
from oracle import rajni_oracle as orc
from rajni_amd import timm_shaped as ts, _native as nat

DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = [BF16, F16, F32]
IDS = ["bf16", "f16", "f32"]


def lib():
    return nat.lib()


def stream():
    return nat.stream_ptr()


def run(rc, what):
    nat.check(rc, what)
    torch.cuda.synchronize()


def ceil(a, b):
    return (a + b - 1) // b * b


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def randn(shape, g, scale=1.0, dtype=BF16):
    return (torch.randn(shape, generator=g, device=DEV) * scale).to(dtype)


def close(got, want, rel, what):
    got, want = got.double(), want.double()
    scale = float(want.abs().max().clamp_min(1e-30))
    err = float((got - want).abs().max())
    assert err <= rel * scale, f"{what}: max err {err:.4g} vs scale {scale:.4g} (rel {err / scale:.3g})"


def guarded_input(t, row_stride=None, **kw):
    return Guarded(tuple(t.shape), t.dtype, DEV, row_stride=row_stride, **kw).fill_(t)


def out(shape, dtype, row_stride=None):
    return Guarded(shape, dtype, DEV, row_stride=row_stride)


def _keeps(n):
    return sorted({1, max(1, n // 2), n})


# (P, patches): the smallest sizes, the lanes-per-token edges, P = 32
SELECT_SHAPES = [(2, 1), (5, 1), (2, 2), (5, 3), (4, 60), (5, 128), (2, 129), (4, 192), (5, 257), (2, 576), (32, 1), (32, 33)]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("P,n", SELECT_SHAPES)
def test_select_topk_prefix_guarded(P, n, dtype):
    """scores in an arena whose tail is NaN (NaN ranks as +inf: a read past the last score changes the pick)"""
    B, N = 3, P + n
    s = randn((B, N), gen(N * 3 + P), dtype=dtype)
    s[1, :: 3] = s[1, 0].clone()                      # runs of ties
    sg = guarded_input(s)
    sh = s.float().cpu().numpy()
    for keep in _keeps(n):
        what = f"select_topk_prefix P={P} n={n} keep={keep} {dtype}"
        ig, ng = out((B, P + keep), torch.int32), out((B, P + keep), dtype)
        run(lib().rajni_select_topk_prefix(sg.ptr(), B, N, P, keep, ig.ptr(), ng.ptr(), nat.dtype_code(dtype), stream()),
            "rajni_select_topk_prefix")
        ig.check(f"{what}: keep_idx")
        ng.check(f"{what}: next_scores")
        sel = npx.select_tokens(sh, keep, P)
        np.testing.assert_array_equal(ig.t.cpu().numpy(), sel, err_msg=what)
        assert np.array_equal(ng.t.float().cpu().numpy(), np.take_along_axis(sh, sel, axis=1)), what
    sg.check("select_topk_prefix: scores", written=False)


@pytest.mark.parametrize("two_pass", [0, 1], ids=["one_pass", "two_pass"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("B,P,n,H,D", [(3, 2, 1, 1, 8), (2, 2, 2, 1, 8), (2, 5, 1, 2, 8), (2, 5, 3, 2, 64), (2, 4, 60, 3, 64),
                                       (2, 2, 63, 2, 40), (2, 5, 192, 4, 64), (1, 4, 573, 16, 64)])
def test_score_select_prefix_guarded(B, P, n, H, D, dtype, two_pass):
    """qkv whose Q third is poisoned for tokens 1..N-1 (importance reads only the CLS query - the registers' queries too are never
    read); scores equal rajni_importance's bits, the selection is the rule applied to them"""
    N = P + n
    qkv = randn((B, N, 3 * H * D), gen(N * H + D + P), dtype=dtype)
    qg = guarded_input(qkv)
    qg.arena[qg.offset:qg.end].view(B, N, -1)[:, 1:, : H * D * qg.esize] = 0xFF
    code = nat.dtype_code(dtype)
    lib().rajni_debug_force_score_two_pass(two_pass)
    try:
        sg = out((B, N), dtype)
        run(lib().rajni_importance(qg.ptr(), sg.ptr(), B, N, H, D, 1e-6, code, stream()), "rajni_importance")
        sg.check(f"importance N={N}: scores")
        if N > 2:
            want = orc.importance_scores(qkv.float().cpu().numpy(), H)
            close(sg.t, torch.from_numpy(want).to(DEV), 2e-5 if dtype == F32 else 6e-3, f"importance N={N} H={H} D={D}")
        for keep in _keeps(n):
            what = f"score_select_prefix B={B} P={P} n={n} H={H} D={D} keep={keep} {dtype}"
            s2, ig, ng = out((B, N), dtype), out((B, P + keep), torch.int32), out((B, P + keep), dtype)
            run(lib().rajni_score_select_prefix(qg.ptr(), B, N, H, D, 1e-6, P, keep, s2.ptr(), ig.ptr(), ng.ptr(), code, stream()),
                "rajni_score_select_prefix")
            for gd, nm in ((s2, "scores"), (ig, "keep_idx"), (ng, "next_scores")):
                gd.check(f"{what}: {nm}")
            assert torch.equal(s2.t.view(torch.uint8), sg.t.view(torch.uint8)), what
            s = s2.t.float().cpu().numpy()
            sel = npx.select_tokens(s, keep, P)
            np.testing.assert_array_equal(ig.t.cpu().numpy(), sel, err_msg=what)
            assert np.array_equal(ng.t.float().cpu().numpy(), np.take_along_axis(s, sel, axis=1), equal_nan=True), what
        qg.check("score_select_prefix: qkv", written=False)
    finally:
        lib().rajni_debug_force_score_two_pass(0)


@pytest.mark.parametrize("fmt", ["bf16", "bf16_to_f32", "f16", "f32"])
@pytest.mark.parametrize("S,Pz,Cc,B,R,has_prefix", [(32, 8, 64, 3, 4, True), (64, 16, 128, 2, 1, False), (64, 16, 128, 1, 4, True),   # fused loader
                                                    (28, 7, 64, 3, 1, True), (56, 14, 128, 2, 4, False), (56, 14, 128, 1, 31, True)])   # columns
def test_patch_embed_prefix_guarded(S, Pz, Cc, B, R, has_prefix, fmt):
    """weight rows >= C and the tails of pos / cls / reg / bias poisoned; x [B, P + n, C] guarded: every row written, prefix rows
    exact, patch rows at tests/test_gpu_guarded.py::test_patch_embed_guarded's tolerances"""
    g = gen(S * Pz + Cc + R)
    dt = {"bf16": BF16, "bf16_to_f32": BF16, "f16": F16, "f32": F32}[fmt]
    Cin, K = 3, 3 * Pz * Pz
    kpad = ceil(K, 64)
    n, P = (S // Pz) ** 2, 1 + R
    img = randn((B, Cin, S, S), g, dtype=dt)
    w = randn((Cc, K), g, 0.05, dt)
    b = randn(Cc, g, 0.1, dt).float()
    cls, reg = randn(Cc, g, dtype=dt), randn((R, Cc), g, dtype=dt)
    pos = randn((n + (P if has_prefix else 0), Cc), g, dtype=dt)
    wg = Guarded((ceil(Cc, 256), kpad), dt, DEV)
    wg.t[:Cc] = 0
    wg.t[:Cc, :K] = w
    ig, bg, cg, rg, pg = guarded_input(img), guarded_input(b), guarded_input(cls), guarded_input(reg), guarded_input(pos)
    xdt = F32 if fmt in ("bf16_to_f32", "f32") else dt
    xg = out((B, P + n, Cc), xdt)
    code = nat.dtype_code(dt)
    nbytes = lib().rajni_patch_embed_workspace_bytes(B, Cin, S, Pz, code)
    ws = out((B * n, kpad), dt) if nbytes else None
    assert ws is None or ws.region == nbytes
    run(lib().rajni_patch_embed_prefix(ig.ptr(), wg.ptr(), bg.ptr(), cg.ptr(), rg.ptr(), P, pg.ptr(), int(has_prefix), xg.ptr(),
                                       int(fmt == "bf16_to_f32"), B, Cin, S, Pz, Cc, code, ws.ptr() if ws is not None else None, nbytes,
                                       stream()), "rajni_patch_embed_prefix")
    what = f"patch embed prefix S={S} patch={Pz} C={Cc} R={R} {fmt}"
    for gd, nm in ((ig, "images"), (wg, "w"), (bg, "bias"), (cg, "cls"), (rg, "reg"), (pg, "pos")):
        gd.check(f"{what}: {nm}", written=False)
    xg.check(f"{what}: x")
    if ws is not None:
        ws.check(f"{what}: workspace")
    cols = img.double().view(B, Cin, S // Pz, Pz, S // Pz, Pz).permute(0, 2, 4, 1, 3, 5).reshape(B, n, K)
    tok = cols @ w.double().T + b.double() + pos.double()[P if has_prefix else 0:][None]
    close(xg.t[:, P:], tok, {"bf16": 1e-2, "f16": 1e-2, "bf16_to_f32": 1e-5, "f32": 3e-6}[fmt], what)
    pre = torch.cat([cls[None], reg]).float()
    if has_prefix:
        pre = pre + pos[:P].float()
    pre = pre.to(xdt)
    for bi in range(B):
        assert torch.equal(xg.t[bi, :P].contiguous().view(torch.uint8), pre.view(torch.uint8)), f"{what}: prefix rows of image {bi}"


@pytest.mark.parametrize("xdt,odt", [(F32, F32), (F32, BF16), (BF16, BF16), (F16, F16)], ids=["f32", "f32_to_bf16", "bf16", "f16"])
@pytest.mark.parametrize("P,N", [(2, 3), (5, 6), (5, 7), (4, 21), (2, 201), (32, 40)])
def test_pool_norm_prefix_guarded(P, N, xdt, odt):
    """the prefix rows of x are POISONED: the 'avg' pool must not read them ('token' reads row 0 only); out [B, C] guarded"""
    B, Cc = 3, 192
    g = gen(P * 100 + N)
    x = randn((B, N, Cc), g, dtype=xdt)
    nw, nb, fw, fb = (randn(Cc, g, 0.1, F32) + 1), randn(Cc, g, 0.1, F32), (randn(Cc, g, 0.1, F32) + 1), randn(Cc, g, 0.1, F32)
    xg = guarded_input(x)
    xg.arena[xg.offset:xg.end].view(B, N, -1)[:, :P] = 0xFF
    og = out((B, Cc), odt)
    code, x_f32 = nat.dtype_code(odt), int(xdt == F32 and odt != F32)
    run(lib().rajni_pool_norm_prefix(xg.ptr(), B, N, P, Cc, nat.POOL_AVG, nw.data_ptr(), nb.data_ptr(), 1e-6, fw.data_ptr(), fb.data_ptr(),
                                     1e-5, og.ptr(), code, x_f32, stream()), "rajni_pool_norm_prefix")
    what = f"pool_norm_prefix P={P} N={N} {xdt}->{odt}"
    og.check(f"{what}: out")
    xg.check(f"{what}: x", written=False)
    ln = torch.nn.functional.layer_norm
    want = ln(ln(x[:, P:].double(), (Cc,), nw.double(), nb.double(), 1e-6).mean(1), (Cc,), fw.double(), fb.double(), 1e-5)
    close(og.t, want, 1e-5 if odt == F32 else 1e-2, what)
    # 'token': row 0 alone
    xg.t[:, 0] = x[:, 0]
    xg.arena[xg.offset:xg.end].view(B, N, -1)[:, 1:] = 0xFF
    og = out((B, Cc), odt)
    run(lib().rajni_pool_norm_prefix(xg.ptr(), B, N, P, Cc, nat.POOL_TOKEN, nw.data_ptr(), nb.data_ptr(), 1e-6, None, None, 0.0, og.ptr(),
                                     code, x_f32, stream()), "rajni_pool_norm_prefix")
    og.check(f"{what} token: out")
    close(og.t, ln(x[:, 0].double(), (Cc,), nw.double(), nb.double(), 1e-6), 1e-5 if odt == F32 else 1e-2, what + " token")


# ---------------------------------------------------------------------------------------------
# the whole forward
# ---------------------------------------------------------------------------------------------

SCHED = {1: {"keep_ratio": 0.75, "update": True}, 2: {"keep_ratio": 0.6, "update": False}}
LAST_PRUNES = {1: {"keep_ratio": 0.75, "update": True}, 3: {"keep_ratio": 0.5, "update": False}}
# (config, format, schedule, resid_bf16, cls_only_last_block)
FWD_CASES = [
    ("vit_micro_reg4_patch16_64", "bf16", SCHED, False, False),
    ("vit_micro_reg4_patch16_64", "fp32", LAST_PRUNES, False, True),
    ("deit3_micro_reg4_patch16_64", "bf16", SCHED, True, True),
    ("deit3_micro_reg4_patch16_64", "fp16", LAST_PRUNES, False, False),
    ("vit_micro_reg1_gap_patch14_56", "bf16", SCHED, False, False),
    ("vit_micro_reg1_gap_patch14_56", "fp32", LAST_PRUNES, False, False),
    ("vit_micro512_reg4_patch16_64", "fp8", SCHED, False, True),
    ("vit_micro512_reg4_patch16_64", "fp8_mfma", SCHED, False, False),
    ("vit_micro512_reg4_patch16_64", "fp8_mfma", LAST_PRUNES, True, True),
]


def _forward_guarded(w, images, ws_fill):
    """rajni_vit_forward_ext_prefix on a copy of the wrapper's plan with a guarded workspace (exactly
    rajni_vit_workspace_bytes_prefix, prefilled with ws_fill), guarded logits and guarded [B, P + keep] stage buffers"""
    entry = w._plan
    plan0, bufs, ext, pre = entry[1], entry[3], entry[2][4], entry[2][6]
    assert pre is not None
    plan = nat.VitPlan.from_buffer_copy(plan0)
    depth, B, ncls = plan.depth, plan.B, plan.num_classes
    blocks = (nat.Block * depth)(*[nat.Block.from_buffer_copy(plan0.blocks[i]) for i in range(depth)])
    plan.blocks = blocks
    tc = (C.c_int32 * depth)(*([-1] * depth))
    plan.token_counts = tc
    stages = {}
    dt = {nat.RAJNI_BF16: BF16, nat.RAJNI_F16: F16, nat.RAJNI_F32: F32}[plan.dtype]
    for i, kb in bufs.items():
        np_, n = kb["keep_idx"].shape[1], kb["scores"].shape[1]
        assert np_ == blocks[i].keep + pre.num_prefix
        st = dict(keep_idx=out((B, np_), torch.int32), next_scores=out((B, np_), dt), scores=out((B, n), dt))
        blocks[i].keep_idx, blocks[i].next_scores, blocks[i].scores = st["keep_idx"].ptr(), st["next_scores"].ptr(), st["scores"].ptr()
        stages[i] = st
    nbytes = lib().rajni_vit_workspace_bytes_prefix(C.byref(plan), C.byref(pre))
    assert nbytes == plan0.workspace_bytes > lib().rajni_vit_workspace_bytes(C.byref(plan))
    ws = Guarded((nbytes,), torch.uint8, DEV)
    ws.t.fill_(ws_fill)
    plan.workspace, plan.workspace_bytes = ws.ptr(), nbytes
    ld = ceil(ncls, 8) + 8
    plan.logits_ld = ld
    lg = out((B, ncls), dt, row_stride=ld)
    run(lib().rajni_vit_forward_ext_prefix(C.byref(plan), C.byref(ext) if ext is not None else None, C.byref(pre), images.data_ptr(),
                                           lg.ptr(), stream()), "rajni_vit_forward_ext_prefix")
    # one byte short is refused before any launch
    plan.workspace_bytes = nbytes - 1
    assert lib().rajni_vit_forward_ext_prefix(C.byref(plan), C.byref(ext) if ext is not None else None, C.byref(pre), images.data_ptr(),
                                              lg.ptr(), stream()) == 1
    return lg, [int(tc[i]) for i in range(depth)], stages, ws


@pytest.mark.parametrize("cfg_name,fmt,sched,resid16,cls_only", FWD_CASES,
                         ids=[f"{c[0]}-{c[1]}-{'lastprunes' if c[2] is LAST_PRUNES else 'sched'}"
                              f"{'-resid16' if c[3] else ''}{'-clsonly' if c[4] else ''}" for c in FWD_CASES])
def test_forward_with_registers_workspace_independence_and_bounds(cfg_name, fmt, sched, resid16, cls_only):
    cfg = ts.CONFIGS[cfg_name]
    P = 1 + cfg.reg_tokens
    model = ts.create_model(cfg, seed=3, std=0.06, bias_std=0.02, round_bf16=True)
    dtype = {"fp32": F32, "fp16": F16}.get(fmt, BF16)
    w = rajni_amd.RAJNIViTWrapper(model, sched).to(DEV).to(dtype).eval().trace_scores(True)
    if fmt in ("fp8", "fp8_mfma"):
        w.set_weight_format(fmt)
    if resid16:
        w.set_residual_dtype(dtype)
    if cfg.global_pool != "avg":
        w.set_last_block_cls_only(cls_only)
    images = torch.randn((3, 3, cfg.img_size, cfg.img_size), generator=gen(7), device=DEV).to(dtype)
    base = w(images)
    counts0 = w.get_last_stats()["token_counts"]
    assert counts0[0] == cfg.num_patches + P
    runs = [_forward_guarded(w, images, f) for f in (0x00, 0x00, 0xFF)]
    what = f"forward {cfg_name} {fmt}"
    for k, (lg, counts, stages, ws) in enumerate(runs):
        ws.check(f"{what} run {k}: workspace", written=False)
        lg.check(f"{what} run {k}: logits")
        assert counts == counts0, what
        for i, st in stages.items():
            recomputed = w.pruning_schedule[i]["update"] or (i - 1) not in w.pruning_schedule
            st["keep_idx"].check(f"{what} run {k} stage {i}: keep_idx")
            st["next_scores"].check(f"{what} run {k} stage {i}: next_scores")
            st["scores"].check(f"{what} run {k} stage {i}: scores", written=recomputed)
            idx = st["keep_idx"].t.cpu().numpy()
            assert (idx[:, :P] == np.arange(P)).all() and (idx[:, P:] >= P).all() and (np.diff(idx, axis=1) > 0).all(), what
    a, b, c = runs

    def same(x, y, name):   # bitwise: the bytes of the views
        assert torch.equal(x.arena[x.offset:x.end], y.arena[y.offset:y.end]), f"{what}: {name} differ"

    for other, tag in ((b, "two runs with a zeroed workspace"), (c, "zeroed vs 0xFF workspace")):
        same(a[0], other[0], f"{tag}: logits")
        for i in a[2]:
            for nm in ("keep_idx", "next_scores", "scores"):
                same(a[2][i][nm], other[2][i][nm], f"{tag}: stage {i} {nm}")
    assert torch.equal(a[0].t, base), f"{what}: logits differ from the wrapper's own forward"
