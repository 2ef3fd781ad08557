"""The oracles against the reference's own outputs for shapes the other fixtures in tests/golden/ do not hold (other head
dims, patch 14, LayerScale, `update=False` stages, odd keep ratios).  The inputs are built from seeds by the functions
below; what the reference computed from them (`tests/golden/make_golden.py::oracle_vs_reference_cases`, the reference
imported read-only under an alias, nothing of it copied) is stored in tests/golden/oracle_vs_reference.npz, so the
comparison runs anywhere.
"""
import os

import numpy as np
import pytest
import torch

from oracle import rajni_oracle as orc
from oracle import rajni_oracle_torch as ort
from rajni_amd import timm_shaped as ts

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_vs_reference.npz")


@pytest.fixture(scope="module")
def ref():
    with np.load(FIXTURE) as f:
        return dict(f)


IMPORTANCE_SHAPES = [(2, 197, 12, 64), (3, 50, 4, 80), (1, 257, 16, 80), (2, 17, 2, 32), (2, 33, 3, 128), (4, 2, 1, 8)]


def importance_inputs(B, N, H, D):
    rng = np.random.default_rng(B * 1000 + N + D)
    return rng.standard_normal((B, N, 3 * H * D), dtype=np.float32) * rng.choice([0.3, 1.0, 3.0])


@pytest.mark.parametrize("B,N,H,D", IMPORTANCE_SHAPES)
def test_importance_on_fresh_inputs(ref, B, N, H, D):
    qkv = importance_inputs(B, N, H, D)
    want = ref[f"imp.{B}-{N}-{H}-{D}"]                                     # importance.py:4-34
    np.testing.assert_allclose(orc.importance_scores(qkv, H), want, rtol=3e-5, atol=1e-8)
    np.testing.assert_allclose(ort.importance_scores(torch.from_numpy(qkv), H).numpy(), want, rtol=3e-5, atol=1e-8)


CASES = [
    # cfg kwargs, schedule, batch
    (dict(img_size=64, embed_dim=128, depth=5, num_heads=2, num_classes=10),
     {1: {"keep_ratio": 0.75}, 2: {"keep_ratio": 0.61, "update": False}, 4: {"keep_ratio": 0.33}}, 3),
    (dict(img_size=56, patch_size=14, embed_dim=320, depth=4, num_heads=4, num_classes=7, layer_scale=0.3),
     {0: {"keep_ratio": 0.9}, 3: {"keep_ratio": 0.5}}, 2),
    (dict(img_size=64, embed_dim=192, depth=3, num_heads=3, num_classes=5, mlp_ratio=2.625),
     {1: {"keep_ratio": 0.01}}, 2),                    # keep = max(1, int(...)) = 1 patch token
    (dict(img_size=96, embed_dim=128, depth=4, num_heads=4, num_classes=10),
     {}, 2),                                           # nothing scheduled: the unpruned path
]


def forward_inputs(case):
    """(cfg, schedule, model, images) of CASES[case]: a freshly seeded timm-shaped model and its images."""
    kw, schedule, batch = CASES[case]
    cfg = ts.ViTConfig(**kw)
    seed = 4242 + case
    model = ts.create_model(cfg, seed=seed, std=0.08, bias_std=0.02)
    images = np.random.default_rng(seed).standard_normal((batch, 3, cfg.img_size, cfg.img_size), dtype=np.float32)
    return cfg, schedule, model, images


@pytest.mark.parametrize("case", range(len(CASES)))
def test_forward_on_fresh_models(ref, case):
    """RAJNIViTWrapper.forward of the reference on a freshly seeded timm-shaped model == both oracles: token counts
    exactly; logits to fp32 round-off when the selections coincide (they do unless two scores tie in fp32)."""
    cfg, schedule, model, images = forward_inputs(case)
    sd = ts.state_dict_numpy(model)
    want = ref[f"fwd{case}.logits"]
    counts = ref[f"fwd{case}.token_counts"].tolist()
    prefix = f"fwd{case}.blk"
    trace = {int(k[len(prefix):-len(".keep_idx")]): v for k, v in ref.items() if k.startswith(prefix)}

    got, stats, tr = orc.vit_forward(sd, images, schedule, depth=cfg.depth, num_heads=cfg.num_heads, ln_eps=cfg.ln_eps,
                                     dtype=np.float64, return_trace=True)
    assert stats["token_counts"] == counts == orc.token_counts(cfg.num_patches + 1, cfg.depth, schedule)
    sd_t = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)) for k, v in sd.items()}
    got_t, stats_t, tr_t = ort.vit_forward(sd_t, torch.from_numpy(images), schedule, depth=cfg.depth, num_heads=cfg.num_heads,
                                           ln_eps=cfg.ln_eps, return_trace=True)
    assert stats_t["token_counts"] == counts
    same = all(np.array_equal(tr[i]["keep_idx"], trace[i]) for i in trace)
    same_t = all(np.array_equal(tr_t[i]["keep_idx"].numpy(), trace[i]) for i in trace)
    assert sorted(trace) == sorted(int(k) for k in schedule)
    assert same and same_t, "selections differ from the reference's (an exact fp32 tie would be needed)"
    scale = max(1.0, np.abs(want).max())
    np.testing.assert_allclose(got, want, rtol=0, atol=2e-4 * scale)
    np.testing.assert_allclose(got_t.numpy(), want, rtol=0, atol=2e-4 * scale)


ATTENTION_CFG = dict(img_size=64, embed_dim=128, depth=1, num_heads=2, num_classes=3)


def attention_inputs():
    """(cfg, x, [(update, prev_scores)]) of the RAJNIAttention contract cases; weights are create_model(cfg, seed=9, ...)."""
    cfg = ts.ViTConfig(**ATTENTION_CFG)
    x = np.random.default_rng(1).standard_normal((3, 17, 128), dtype=np.float32)
    variants = [(True, None), (False, np.random.default_rng(2).random((3, 17), dtype=np.float32)), (False, None)]
    return cfg, x, variants


def test_rajni_attention_forward_contract(ref):
    """RAJNIAttention.forward(x, prev_scores) -> (out, keep_idx int64 ascending with CLS first, next_scores), with
    and without carried scores (attention.py:17-60) == oracle.rajni_attention on the same weights."""
    cfg, x, variants = attention_inputs()
    sd = ts.state_dict_numpy(ts.create_model(cfg, seed=9, std=0.1, bias_std=0.05))
    for j, (update, prev) in enumerate(variants):
        out, idx, nxt = ref[f"attn{j}.out"], ref[f"attn{j}.keep_idx"], ref[f"attn{j}.next_scores"]
        o, i, n, _ = orc.rajni_attention(x, sd, "blocks.0.attn.", 2, 0.6, update, prev)
        assert idx.dtype == np.int64 and (idx[:, 0] == 0).all() and (idx[:, 1:] > idx[:, :-1]).all()
        np.testing.assert_array_equal(i, idx)
        np.testing.assert_allclose(o, out, rtol=0, atol=2e-5)
        np.testing.assert_allclose(n, nxt, rtol=2e-5, atol=1e-8)
