"""Bounds and isolation of every C-ABI entry point in its fp16 form (RAJNI_F16), with poisoned inputs and guarded outputs
(tests/guarded.py; the helpers of tests/test_gpu_guarded.py).  GPU box only (`-m gpu`).

0xFFFF is NaN in fp16 as in bf16, so the rules are the bf16 ones: guards and row gaps intact, every output element
written, poisoned input memory never reaching a result.  Values are held to the fp16 tolerances of tests/test_gpu_fp16.py.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rajni_amd
from guarded import Guarded
from oracle import rajni_oracle as orc
from rajni_amd import timm_shaped as ts, _native as nat
from test_gpu_guarded import (DEV, F32, LAST_PRUNES, SCHED, Resid, _args, _attn_inputs, _attn_ref, _epi_ref, _keeps,
                              _qkv_cls_query_only, ceil, close, gen, guarded_input, index_input, lib, out, randn,
                              random_selection, run, stream)

F16 = torch.float16
REL16, REL16_ATTN = 2e-3, 4e-3


@pytest.fixture(params=[0, 1, 4, 5], ids=["auto", "small128x128", "wide256x256", "mid256x128"])
def tiling(request):
    lib().rajni_debug_force_gemm_tiling(request.param)
    yield request.param
    lib().rajni_debug_force_gemm_tiling(0)


def _linear_case(M, N, K, epi, seed, resid_mode=None, stream_f32=False):
    g = gen(seed)
    lda, ldc, ldr = K + 64, ceil(N, 8) + 24, ceil(N, 8) + 8
    x = randn((M, K), g, dtype=F16)
    xg = guarded_input(x, row_stride=lda)
    w = randn((N, K), g, 0.1 if epi == nat.EPI_BIAS_RESID else 0.05, F16)
    wg = Guarded((ceil(N, 256), K), F16, DEV)
    wg.t[:N] = w
    b = randn(N, g, 0.5, F32)
    bg = guarded_input(b)
    lin = x.double() @ w.double().T + b.double()
    ydt = F32 if stream_f32 else F16
    gam = gg = res = None
    if epi == nat.EPI_BIAS_RESID:
        gam = randn(N, g, 1.0, F32)
        gg = guarded_input(gam)
        res = Resid(resid_mode, M, N, ydt, ldc if resid_mode == "inplace" else ldr, g)
    yg = res.g if res is not None and res.mode == "inplace" else out((M, N), ydt, row_stride=ldc)
    a = _args(xg, lda, wg, K, M, N, K, epi, nat.RAJNI_F16, yg, ldc, bg, gamma=gg)
    if res is not None:
        res.fill_args(a)
        a.stream_f32 = int(stream_f32)
    want = _epi_ref(lin, epi, gam, res.rows if res is not None else None)
    run(lib().rajni_linear(C.byref(a), stream()), "rajni_linear")
    what = f"linear f16 {M}x{N}x{K} epi {epi} resid {resid_mode} f32stream {stream_f32}"
    for gd, nm in ((xg, "x"), (wg, "w"), (bg, "bias"), (gg, "gamma")):
        if gd is not None:
            gd.check(f"{what}: input {nm}", written=False)
    if res is not None and res.mode != "inplace":
        res.g.check(f"{what}: input resid", written=False)
    yg.check(f"{what}: y")
    close(yg.t, want, 1e-5 if stream_f32 else REL16, what)


@pytest.mark.parametrize("M,N,K", [(1, 200, 128), (127, 8, 64), (129, 320, 256), (255, 1000, 192), (1025, 320, 256),
                                   (1100, 2304, 768)])
@pytest.mark.parametrize("epi", [nat.EPI_BIAS, nat.EPI_BIAS_GELU], ids=["bias", "gelu"])
def test_linear_f16_bias_gelu_guarded(epi, M, N, K, tiling):
    _linear_case(M, N, K, epi, seed=M + N + K + epi)


@pytest.mark.parametrize("M,N,K", [(129, 200, 192), (1025, 320, 256), (1110, 768, 768)])
@pytest.mark.parametrize("mode", ["plain", "gathered", "inplace"])
@pytest.mark.parametrize("stream_f32", [False, True], ids=["f16stream", "f32stream"])
def test_linear_f16_resid_guarded(stream_f32, mode, M, N, K, tiling):
    _linear_case(M, N, K, nat.EPI_BIAS_RESID, seed=M + N + K, resid_mode=mode, stream_f32=stream_f32)


@pytest.mark.parametrize("D", [8, 40, 64, 128])
@pytest.mark.parametrize("n_p", [1, 33, 129, 224, 257])
@pytest.mark.parametrize("gathered", [False, True], ids=["identity", "gathered"])
def test_attention_f16_guarded(gathered, n_p, D):
    B, H = 2, 3
    qg, ig, kept, n_src = _attn_inputs(B, n_p, H, D, gathered, F16, seed=n_p * D + gathered)
    og = out((B, n_p, H * D), F16)
    scale = D ** -0.5
    run(lib().rajni_attention(qg.ptr(), ig.ptr() if ig is not None else None, og.ptr(), B, n_src, n_p, H, D, scale,
                              nat.RAJNI_F16, stream()), "rajni_attention")
    what = f"attention f16 np={n_p} D={D} gathered={gathered}"
    qg.check(f"{what}: qkv", written=False)
    og.check(f"{what}: out")
    close(og.t, _attn_ref(kept, H, D, scale), REL16_ATTN, what)


@pytest.mark.parametrize("B,N,H,D", [(3, 2, 2, 64), (2, 64, 3, 64), (2, 65, 2, 40), (2, 197, 4, 64), (1, 577, 16, 64)])
def test_score_select_f16_guarded(B, N, H, D):
    qg, qkv = _qkv_cls_query_only(B, N, H, D, F16, seed=N * H + D)
    for keep in _keeps(N):
        what = f"score_select f16 N={N} keep={keep}"
        s2, ig, ng = out((B, N), F16), out((B, keep + 1), torch.int32), out((B, keep + 1), F16)
        run(lib().rajni_score_select(qg.ptr(), B, N, H, D, 1e-6, keep, s2.ptr(), ig.ptr(), ng.ptr(), nat.RAJNI_F16,
                                     stream()), "rajni_score_select")
        for gd, nm in ((s2, "scores"), (ig, "keep_idx"), (ng, "next_scores")):
            gd.check(f"{what}: {nm}")
        s = s2.t.float().cpu().numpy()
        sel = orc.select_tokens(s, keep)
        np.testing.assert_array_equal(ig.t.cpu().numpy(), sel, err_msg=what)
        assert np.array_equal(ng.t.float().cpu().numpy(), np.take_along_axis(s, sel, axis=1)), what
        if N > 2:
            close(s2.t, torch.from_numpy(orc.importance_scores(qkv.float().cpu().numpy(), H)).to(DEV), REL16, what)
    qg.check("score_select f16: qkv", written=False)


@pytest.mark.parametrize("N", [2, 3, 65, 197, 577])
def test_select_topk_f16_guarded(N):
    B = 3
    g = gen(N)
    s = randn((B, N), g, dtype=F16)
    sg = guarded_input(s)
    for keep in _keeps(N):
        ig, ng = out((B, keep + 1), torch.int32), out((B, keep + 1), F16)
        run(lib().rajni_select_topk(sg.ptr(), B, N, keep, ig.ptr(), ng.ptr(), nat.RAJNI_F16, stream()), "rajni_select_topk")
        ig.check(f"select f16 N={N}: keep_idx")
        ng.check(f"select f16 N={N}: next_scores")
        sel = orc.select_tokens(s.float().cpu().numpy(), keep)
        np.testing.assert_array_equal(ig.t.cpu().numpy(), sel)
    sg.check("select f16: scores", written=False)


@pytest.mark.parametrize("kind,Cc", [(k, c) for k in ("f16", "f32x", "rows_f32x") for c in (8, 200, 768, 1024, 2048)
                                     if k != "rows_f32x" or c <= 1024])
def test_layernorm_f16_guarded(kind, Cc):
    rows = 4100 if kind == "rows_f32x" else 37
    xdt = F16 if kind == "f16" else F32
    g = gen(Cc + rows)
    x = (torch.randn((rows, Cc), generator=g, device=DEV) * 2 + 0.5).to(xdt)
    stride = Cc + 24
    xg = guarded_input(x, row_stride=stride)
    w = (1 + 0.1 * torch.randn(Cc, generator=g, device=DEV)).to(F16).float()
    b = (0.1 * torch.randn(Cc, generator=g, device=DEV)).to(F16).float()
    wg, bg = guarded_input(w), guarded_input(b)
    yg = out((rows, Cc), F16)
    run(lib().rajni_layernorm(xg.ptr(), stride, wg.ptr(), bg.ptr(), yg.ptr(), rows, Cc, 1e-6, nat.RAJNI_F16,
                              int(xdt == F32), stream()), "rajni_layernorm")
    what = f"layernorm f16 {kind} C={Cc}"
    for gd, nm in ((xg, "x"), (wg, "w"), (bg, "b")):
        gd.check(f"{what}: {nm}", written=False)
    yg.check(f"{what}: y")
    xd = x.double()
    mu = xd.mean(dim=1, keepdim=True)
    want = (xd - mu) / torch.sqrt(((xd - mu) ** 2).mean(dim=1, keepdim=True) + 1e-6) * w.double() + b.double()
    close(yg.t, want, REL16, what)


@pytest.mark.parametrize("E", [8, 40, 768, 2304])
def test_gather_rows_f16_guarded(E):
    B, n_src, n_dst = 3, 41, 29
    g = gen(E)
    src = randn((B, n_src, E), g, dtype=F16)
    unsel = n_src - 1
    idx = random_selection(B, n_src, n_dst, g, unsel)
    sg = Guarded((B, n_src, E), F16, DEV)
    for bi in range(B):
        sg.t[bi, idx[bi]] = src[bi, idx[bi]]
    ig = index_input(idx, unsel)
    og = out((B, n_dst, E), F16)
    run(lib().rajni_gather_rows(sg.ptr(), ig.ptr(), og.ptr(), B, n_src, n_dst, E, nat.RAJNI_F16, stream()),
        "rajni_gather_rows")
    og.check(f"gather f16 E={E}: dst")
    sg.check(f"gather f16 E={E}: src", written=False)
    assert torch.equal(og.t, torch.gather(src, 1, idx[:, :, None].expand(-1, -1, E)))


@pytest.mark.parametrize("out_f32", [False, True])
@pytest.mark.parametrize("S,P,Cc,B,has_cls", [(32, 8, 64, 3, True), (64, 16, 128, 2, False), (96, 32, 192, 2, True),
                                              (56, 14, 128, 3, True), (28, 7, 64, 2, False)])
def test_patch_embed_f16_guarded(S, P, Cc, B, has_cls, out_f32):
    g = gen(S + P + Cc)
    img = randn((B, 3, S, S), g, dtype=F16)
    K = 3 * P * P
    kpad = ceil(K, 64)
    w = randn((Cc, K), g, 0.05, F16)
    wg = Guarded((ceil(Cc, 256), kpad), F16, DEV)
    wg.t[:Cc].zero_()
    wg.t[:Cc, :K] = w
    b, cls = randn(Cc, g, 0.1, F32), randn(Cc, g, dtype=F16)
    npatch = (S // P) ** 2
    pos = randn((npatch + int(has_cls), Cc), g, dtype=F16)
    imgg, bg, clsg, posg = guarded_input(img), guarded_input(b), guarded_input(cls), guarded_input(pos)
    ydt = F32 if out_f32 else F16
    xg = out((B, npatch + 1, Cc), ydt)
    nbytes = lib().rajni_patch_embed_workspace_bytes(B, 3, S, P, nat.RAJNI_F16)
    ws = Guarded((max(nbytes, 16),), torch.uint8, DEV) if nbytes else None
    run(lib().rajni_patch_embed(imgg.ptr(), wg.ptr(), bg.ptr(), clsg.ptr(), posg.ptr(), int(has_cls), xg.ptr(),
                                int(out_f32), B, 3, S, P, Cc, nat.RAJNI_F16, ws.ptr() if ws else None, nbytes, stream()),
        "rajni_patch_embed")
    what = f"patch embed f16 S={S} P={P} out_f32={out_f32}"
    for gd, nm in ((imgg, "images"), (bg, "bias"), (clsg, "cls"), (posg, "pos")):
        gd.check(f"{what}: {nm}", written=False)
    if ws is not None:
        ws.check(f"{what}: workspace", written=False)
    xg.check(f"{what}: x")
    tok = orc.patch_embed(img.double().cpu().numpy(), w.double().cpu().numpy().reshape(Cc, 3, P, P), b.double().cpu().numpy())
    c, p = cls.double().cpu().numpy(), pos.double().cpu().numpy()
    if has_cls:
        want = np.concatenate([np.broadcast_to(c, (B, 1, Cc)), tok], axis=1) + p[None]
    else:
        want = np.concatenate([np.broadcast_to(c, (B, 1, Cc)), tok + p[None]], axis=1)
    close(xg.t, torch.from_numpy(want).to(DEV), 1e-5 if out_f32 else REL16, what)


# ---------------------------------------------------------------------------------------------
# whole fp16 forward: guarded workspace, logits and stage buffers; results independent of the workspace's contents
# ---------------------------------------------------------------------------------------------

FWD_CASES = [("vit_micro_patch16_64", SCHED, False, False), ("vit_micro_patch16_64", SCHED, True, True),
             ("vit_micro_patch16_64", LAST_PRUNES, False, True), ("vit_micro_d80_patch16_64", SCHED, False, True),
             ("vit_micro_patch14_56", SCHED, True, False), ("deit3_micro_patch16_64", LAST_PRUNES, False, False)]


def _forward_guarded(w, images, ws_fill):
    entry = w._plan
    plan0, bufs = entry[1], entry[3]
    plan = nat.VitPlan.from_buffer_copy(plan0)
    depth, B, ncls = plan.depth, plan.B, plan.num_classes
    blocks = (nat.Block * depth)(*[nat.Block.from_buffer_copy(plan0.blocks[i]) for i in range(depth)])
    plan.blocks = blocks
    tc = (C.c_int32 * depth)(*([-1] * depth))
    plan.token_counts = tc
    stages = {}
    for i, kb in bufs.items():
        keep1, n = kb["keep_idx"].shape[1], kb["scores"].shape[1]
        st = dict(keep_idx=out((B, keep1), torch.int32), next_scores=out((B, keep1), F16), scores=out((B, n), F16))
        blocks[i].keep_idx, blocks[i].next_scores, blocks[i].scores = (st["keep_idx"].ptr(), st["next_scores"].ptr(),
                                                                      st["scores"].ptr())
        stages[i] = st
    nbytes = lib().rajni_vit_workspace_bytes(C.byref(plan))
    assert nbytes == plan0.workspace_bytes
    ws = Guarded((nbytes,), torch.uint8, DEV)
    ws.t.fill_(ws_fill)
    plan.workspace, plan.workspace_bytes = ws.ptr(), nbytes
    ld = ceil(ncls, 8) + 8
    plan.logits_ld = ld
    lg = out((B, ncls), F16, row_stride=ld)
    run(lib().rajni_vit_forward(C.byref(plan), images.data_ptr(), lg.ptr(), stream()), "rajni_vit_forward")
    return lg, [int(tc[i]) for i in range(depth)], stages, ws


@pytest.mark.parametrize("cfg_name,sched,resid16,cls_only", FWD_CASES,
                         ids=[f"{c[0]}-{'lastprunes' if c[1] is LAST_PRUNES else 'sched'}{'-resid16' if c[2] else ''}"
                              f"{'-clsonly' if c[3] else ''}" for c in FWD_CASES])
def test_forward_f16_workspace_independence_and_bounds(cfg_name, sched, resid16, cls_only):
    cfg = ts.CONFIGS[cfg_name]
    model = ts.create_model(cfg, seed=3, std=0.06, bias_std=0.02, round_bf16=True)
    w = rajni_amd.RAJNIViTWrapper(model, sched).to(DEV).to(F16).eval().trace_scores(True)
    if resid16:
        w.set_residual_dtype(F16)
    w.set_last_block_cls_only(cls_only)
    images = torch.randn((3, 3, cfg.img_size, cfg.img_size), generator=gen(7), device=DEV).to(F16)
    base = w(images)
    runs = [_forward_guarded(w, images, f) for f in (0x00, 0x00, 0xFF)]
    what = f"forward f16 {cfg_name}"
    for k, (lg, counts, stages, ws) in enumerate(runs):
        ws.check(f"{what} run {k}: workspace", written=False)
        lg.check(f"{what} run {k}: logits")
        assert counts == w.get_last_stats()["token_counts"], what
        for i, st in stages.items():
            recomputed = w.pruning_schedule[i]["update"] or (i - 1) not in w.pruning_schedule
            st["keep_idx"].check(f"{what} run {k} stage {i}: keep_idx")
            st["next_scores"].check(f"{what} run {k} stage {i}: next_scores")
            st["scores"].check(f"{what} run {k} stage {i}: scores", written=recomputed)
    a = runs[0]
    for other in runs[1:]:
        assert torch.equal(a[0].arena[a[0].offset:a[0].end], other[0].arena[other[0].offset:other[0].end]), what
        for i in a[2]:
            for nm in ("keep_idx", "next_scores", "scores"):
                x, y = a[2][i][nm], other[2][i][nm]
                assert torch.equal(x.arena[x.offset:x.end], y.arena[y.offset:y.end]), f"{what}: stage {i} {nm}"
    assert torch.equal(a[0].t, base), f"{what}: logits differ from the wrapper's own forward"
