"""The last block computed for the rows the head reads (the default) against every row of it
(rajni_debug_set_last_block_all_rows(1), the reference's op graph row for row).

Behind the last block's K and V only x[:, 0] is observable (model.py:65-66), so the forward runs that block's attention for
the first query tile and proj / LN2 / FC1 / fc2 on the B CLS rows: the all-rows kernels on fewer rows.  No new arithmetic,
so logits must be BIT-identical, and stats and traces equal, for every dtype, weight format and timm variant; plans that are
not eligible (avg-pooled head, a last block that prunes) run all rows either way and are here to check the eligibility test."""
import ctypes as C
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

import rajni_amd
from rajni_amd import _native as nat
from rajni_amd import timm_shaped as ts

DEV = "cuda"
MICRO_SCHED = {1: {"keep_ratio": 0.75, "update": True}, 2: {"keep_ratio": 0.6, "update": False}}
TINY_SCHED = {3: {"keep_ratio": 0.8, "update": True}, 7: {"keep_ratio": 0.7, "update": True}}
README_SCHEDULE = {3: {"keep_ratio": 0.88, "update": True}, 4: {"keep_ratio": 0.88, "update": True},
                   7: {"keep_ratio": 0.80, "update": True}, 8: {"keep_ratio": 0.72, "update": True}}
PRENORM_FCNORM = dataclasses.replace(ts.CONFIGS["vit_micro_prenorm_patch16_64"], fc_norm=True)

# (id, config, schedule, model dtype, weight format, residual stream dtype, batch)
CASES = [
    ("micro_bf16", "vit_micro_patch16_64", MICRO_SCHED, torch.bfloat16, "model", None, 5),
    ("tiny_bf16", "vit_tiny_patch16_224", TINY_SCHED, torch.bfloat16, "model", None, 3),
    ("tiny_fp16", "vit_tiny_patch16_224", TINY_SCHED, torch.float16, "model", None, 3),
    ("tiny_fp32", "vit_tiny_patch16_224", TINY_SCHED, torch.float32, "model", None, 3),
    ("tiny_fp8_weights", "vit_tiny_patch16_224", TINY_SCHED, torch.bfloat16, "fp8", None, 3),
    ("micro_bf16_stream", "vit_micro_patch16_64", MICRO_SCHED, torch.bfloat16, "model", torch.bfloat16, 5),
    ("micro_registers", "vit_micro_reg4_patch16_64", MICRO_SCHED, torch.bfloat16, "model", None, 5),
    ("micro_qk_norm", "vit_micro_qknorm_patch16_64", MICRO_SCHED, torch.bfloat16, "model", None, 5),
    ("micro_prenorm_fcnorm", PRENORM_FCNORM, MICRO_SCHED, torch.bfloat16, "model", None, 5),
    # not eligible: both switch positions run all rows
    ("micro_avg_pool", "vit_micro_gap_patch16_64", MICRO_SCHED, torch.bfloat16, "model", None, 5),
    ("micro_last_block_prunes", "vit_micro_patch16_64", {1: {"keep_ratio": 0.75}, 3: {"keep_ratio": 0.5}}, torch.bfloat16,
     "model", None, 5),
    # the all-rows LN2 of the last block takes the two-rows-per-wave LayerNorm kernel (>= 4096 rows), the B-row LN2 the
    # one-row kernel: 320 images x 13 tokens = 4160 rows
    ("micro_ln_kernels", "vit_micro_patch16_64", {1: {"keep_ratio": 0.75}}, torch.bfloat16, "model", None, 320),
]


def _wrapped(cfg, sched, dtype, fmt, resid, seed=4):
    model = ts.create_model(cfg, seed=seed, std=0.08, bias_std=0.02, round_bf16=True)
    w = rajni_amd.RAJNIViTWrapper(model, sched).to(DEV).to(dtype).eval()
    if fmt != "model":
        w.set_weight_format(fmt)
    if resid is not None:
        w.set_residual_dtype(resid)
    return w


def _run(w, images):
    logits = w(images).clone()
    trace = {i: {k: v.clone() for k, v in d.items()} for i, d in w.get_last_trace().items()}
    return logits, w.get_last_stats(), trace


def _same(a, b):
    (la, sa, ta), (lb, sb, tb) = a, b
    assert la.dtype == lb.dtype and torch.equal(la, lb), "logits differ between the CLS-row and the all-rows last block"
    assert sa == sb
    assert ta.keys() == tb.keys()
    for i in ta:
        assert ta[i].keys() == tb[i].keys()
        for k in ta[i]:
            assert torch.equal(ta[i][k], tb[i][k]), (i, k)


def _compare(w, images):
    """default against all rows, free running and with the default run's own selection forced"""
    lib = nat.lib()
    try:
        rows = _run(w, images)
        lib.rajni_debug_set_last_block_all_rows(1)
        full = _run(w, images)
        _same(rows, full)
        w.force_keep_idx({i: d["keep_idx"] for i, d in rows[2].items()})
        full_forced = _run(w, images)
        lib.rajni_debug_set_last_block_all_rows(0)
        rows_forced = _run(w, images)
        _same(rows_forced, full_forced)
        assert torch.equal(rows_forced[0], rows[0])
    finally:
        lib.rajni_debug_set_last_block_all_rows(0)
        w.force_keep_idx(None)
    assert torch.isfinite(rows[0].float()).all()
    return rows


@pytest.mark.parametrize("name,cfg,sched,dtype,fmt,resid,batch", CASES, ids=[c[0] for c in CASES])
def test_cls_row_last_block_is_bit_identical_to_all_rows(name, cfg, sched, dtype, fmt, resid, batch):
    cfg = ts.CONFIGS[cfg] if isinstance(cfg, str) else cfg
    w = _wrapped(cfg, sched, dtype, fmt, resid)
    gen = torch.Generator(device=DEV).manual_seed(7)
    images = torch.randn(batch, cfg.in_chans, cfg.img_size, cfg.img_size, generator=gen, device=DEV).to(dtype)
    _, stats, _ = _compare(w, images)
    if name == "micro_ln_kernels":
        assert batch * stats["token_counts"][-1] >= 4096


def _plan(M, N, K, epi, sf32, cus):
    a = nat.LinearArgs()
    a.x, a.w, a.y, a.resid = 0x1000, 0x2000, 0x3000, 0x4000 if epi == nat.EPI_BIAS_RESID else None   # checked, never followed
    a.lda, a.ldw, a.ldc, a.ldr, a.M, a.N, a.K = K, K, N, N, M, N, K
    a.epilogue, a.dtype, a.stream_f32 = epi, nat.RAJNI_BF16, sf32
    out = nat.LinearPlan()
    assert nat.lib().rajni_debug_linear_plan(C.byref(a), cus, C.byref(out)) == 0
    return out.tiling


def test_vit_base_last_block_crosses_gemm_tilings():
    """ViT-B, README schedule, 12 images: the all-rows last block (12 x 87 = 1044 rows) takes the persistent 256-row tilings,
    the 12 CLS rows take 128 x 128 - a row of a rajni_linear result must not depend on the tiling of M."""
    cfg = ts.CONFIGS["vit_base_patch16_224"]
    batch, tokens = 12, 87
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    persistent = (nat.TILING_WIDE, nat.TILING_MID)
    for n, k, epi, sf32 in ((cfg.embed_dim, cfg.embed_dim, nat.EPI_BIAS_RESID, 1),          # proj
                            (4 * cfg.embed_dim, cfg.embed_dim, nat.EPI_BIAS_GELU, 0),       # FC1
                            (cfg.embed_dim, 4 * cfg.embed_dim, nat.EPI_BIAS_RESID, 1)):     # fc2
        assert _plan(batch * tokens, n, k, epi, sf32, cus) in persistent, (n, k)
        assert _plan(batch, n, k, epi, sf32, cus) == nat.TILING_SMALL, (n, k)
    model = ts.create_model(cfg, seed=0).to(torch.bfloat16).to(DEV)
    w = rajni_amd.RAJNIViTWrapper(model, README_SCHEDULE).eval()
    gen = torch.Generator(device=DEV).manual_seed(11)
    images = torch.randn(batch, 3, 224, 224, generator=gen, device=DEV).to(torch.bfloat16)
    _, stats, _ = _compare(w, images)
    assert stats["token_counts"][-1] == tokens
