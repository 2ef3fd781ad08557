"""End-to-end parity of the HIP forward (RAJNIViTWrapper -> rajni_vit_forward) against the golden
fixtures captured from the reference and against the CPU oracle.  GPU box only (`-m gpu`).

Design follows SURVEY 4-3 (selection-conditional parity), because top-k on bf16 scores is not
reproducible across implementations:
  (a) get_last_stats() token counts: exact;
  (b) with the REFERENCE's keep_idx injected, logits within 1e-2 of the logit scale (the bf16 budget
      of BASELINE.json) of the reference's fp32 logits on the same bf16-representable weights/inputs;
  (c) un-injected: the device's selection must be a valid top-k of the device's own scores (exact,
      integer), its scores must match the reference's within bf16 rounding, and the logits must match
      the ORACLE run with the device's selections injected.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rajni_amd
from oracle import rajni_oracle as orc
from rajni_amd import timm_shaped as ts
from helpers import load_case, case_state_dict, case_images, pruned_blocks

DEV = "cuda"
CASES = ["micro_fp32", "tiny224_fp32", "base224_fp32", "deit3_fp32", "large384_fp32", "microd80_fp32", "microp14_fp32"]


def build(meta):
    cfg = ts.CONFIGS[meta["cfg_name"]]
    model = ts.create_model(cfg, seed=meta["seed"], std=meta["std"], bias_std=meta["bias_std"], round_bf16=True)
    wrapped = rajni_amd.RAJNIViTWrapper(model, meta["schedule"]).to(DEV).to(torch.bfloat16).eval()
    return cfg, wrapped


@pytest.mark.parametrize("name", CASES)
def test_forward_selection_conditional(name):
    meta, data = load_case(name)
    cfg, wrapped = build(meta)
    images = torch.from_numpy(case_images(meta, data)).to(DEV)
    forced = {i: torch.from_numpy(data[f"blk{i}.keep_idx"]).to(DEV) for i in pruned_blocks(meta)}
    wrapped.force_keep_idx(forced)
    logits = wrapped(images).float().cpu().numpy()
    assert wrapped.get_last_stats()["token_counts"] == data["token_counts"].tolist()      # (a)
    ref = data["logits"]
    scale = np.abs(ref).max()
    err = np.abs(logits - ref).max()
    assert err <= 1e-2 * scale, f"{name}: max |dlogit| {err:.4g} vs scale {scale:.4g}"     # (b)
    assert (logits.argmax(1) == ref.argmax(1)).all()
    # carried scores of every stage (attention.py:58) match the reference's
    tr = wrapped.get_last_trace()
    for i in pruned_blocks(meta):
        want = data[f"blk{i}.next_scores"]
        got = tr[i]["next_scores"].float().cpu().numpy()
        # intermediate, softmax-sensitive quantity stored in bf16: 3e-2 (the logits carry the 1e-2 bar)
        assert np.abs(got - want).max() <= 3e-2 * np.abs(want).max()


@pytest.mark.parametrize("name", CASES)
def test_forward_free_running(name):
    meta, data = load_case(name)
    cfg, wrapped = build(meta)
    wrapped.trace_scores(True)
    images_np = case_images(meta, data)
    logits = wrapped(torch.from_numpy(images_np).to(DEV)).float().cpu().numpy()
    assert wrapped.get_last_stats()["token_counts"] == data["token_counts"].tolist()
    tr = wrapped.get_last_trace()
    forced = {}
    first = pruned_blocks(meta)[0]
    for i in pruned_blocks(meta):
        s = tr[i]["scores"].float().cpu().numpy().astype(np.float64)
        idx = tr[i]["keep_idx"].cpu().numpy()
        keep = idx.shape[1] - 1
        # integer part: exactly the defined rule on the device's own scores
        np.testing.assert_array_equal(idx, orc.select_tokens(s, keep))
        forced[i] = idx
        if i == first:
            # before any selection differs the inputs are identical: scores match the reference
            want = data[f"blk{i}.scores"]
            assert np.abs(s - want).max() <= 2e-2 * np.abs(want).max()
            agree = np.mean([len(set(a) & set(b)) / len(a) for a, b in zip(idx, data[f"blk{i}.keep_idx"])])
            assert agree >= 0.93, f"{name}: stage-0 selection overlap {agree:.3f}"
    # (c) logits vs the oracle with the device's selections injected
    _, sd = case_state_dict(meta)
    want, stats = orc.vit_forward(sd, images_np, meta["schedule"], depth=cfg.depth, num_heads=cfg.num_heads,
                                  ln_eps=cfg.ln_eps, forced_keep=forced, dtype=np.float32)
    scale = np.abs(want).max()
    err = np.abs(logits - want).max()
    assert err <= 1e-2 * scale, f"{name}: max |dlogit| {err:.4g} vs scale {scale:.4g}"
    assert stats["token_counts"] == wrapped.get_last_stats()["token_counts"]


def test_bf16_residual_stream_mode():
    """`set_residual_dtype(bfloat16)` keeps x in bf16 between blocks like the reference's own bf16
    model.  Measured on the oracle (DESIGN.md "numerics"): a bf16 residual stream alone costs
    ~1e-2 of the logit scale - the reference's own bf16 CPU run is 1.1e-2 away from its fp32 run -
    so this mode is held to 2e-2, and it must be no better than the fp32-stream default."""
    meta, data = load_case("base224_fp32")
    cfg, wrapped = build(meta)
    images = torch.from_numpy(case_images(meta, data)).to(DEV)
    forced = {i: torch.from_numpy(data[f"blk{i}.keep_idx"]).to(DEV) for i in pruned_blocks(meta)}
    wrapped.force_keep_idx(forced)
    ref = data["logits"]
    scale = np.abs(ref).max()
    e32 = np.abs(wrapped(images).float().cpu().numpy() - ref).max()
    wrapped.set_residual_dtype(torch.bfloat16)
    e16 = np.abs(wrapped(images).float().cpu().numpy() - ref).max()
    assert e16 <= 2e-2 * scale and e32 <= 1e-2 * scale, (e16, e32, scale)


def test_keep_ratio_one_and_empty_schedule_equal_base():
    """keep_ratio=1.0 and an empty schedule are the unpruned network."""
    cfg = ts.CONFIGS["vit_micro_patch16_64"]
    imgs = torch.from_numpy(ts.bf16_round_np(np.random.default_rng(0).standard_normal((3, 3, 64, 64), dtype=np.float32))).to(DEV)
    outs, live = [], []
    for sched in ({}, {1: {"keep_ratio": 1.0}, 2: {"keep_ratio": 1.0, "update": False}}):
        m = ts.create_model(cfg, seed=5, std=0.08, bias_std=0.02, round_bf16=True)
        w = rajni_amd.RAJNIViTWrapper(m, sched).to(DEV).to(torch.bfloat16)
        y = w(imgs)
        live.append((w, y))      # the first wrapper and its device result stay alive: the second cannot inherit them
        outs.append(y.float().cpu())
        assert w.get_last_stats()["token_counts"] == [17] * 4
    assert torch.equal(outs[0], outs[1])
    base = ts.create_model(cfg, seed=5, std=0.08, bias_std=0.02, round_bf16=True).to(DEV).to(torch.bfloat16)
    ref = base(imgs.to(torch.bfloat16)).float().cpu()
    assert (outs[0] - ref).abs().max() <= 2e-2 * ref.abs().max()


def test_string_keys_and_update_chain():
    """B1 fix: JSON-style string keys prune; Q3: update=False re-uses carried scores."""
    cfg = ts.CONFIGS["vit_micro_patch16_64"]
    imgs = torch.from_numpy(np.random.default_rng(1).standard_normal((2, 3, 64, 64), dtype=np.float32)).to(DEV)
    sched_int = {1: {"keep_ratio": 0.75}, 2: {"keep_ratio": 0.6, "update": False}}
    sched_str = {"1": {"keep_ratio": 0.75}, "2": {"keep_ratio": 0.6, "update": False}}
    res = []
    for s in (sched_int, sched_str):
        w = rajni_amd.RAJNIViTWrapper(ts.create_model(cfg, seed=2, std=0.08), s).to(DEV).to(torch.bfloat16)
        res.append(w(imgs))
        assert w.get_last_stats()["token_counts"] == [17, 17, 13, 8]
        tr = w.get_last_trace()
        # block 2 ranks the scores carried from block 1: its kept scores are a subset of block 1's
        a = tr[1]["next_scores"].float().cpu().numpy()
        b = tr[2]["next_scores"].float().cpu().numpy()
        i2 = tr[2]["keep_idx"].cpu().numpy()
        np.testing.assert_array_equal(b, np.take_along_axis(a, i2, axis=1))
    assert torch.equal(res[0], res[1])


def test_module_level_api_matches_oracle():
    """RAJNIAttention.forward / compute_importance used stand-alone (reference attention.py:17-60)."""
    from rajni_amd.wrapper import RAJNIAttention, compute_importance
    cfg = ts.CONFIGS["vit_tiny_patch16_224"]
    model = ts.create_model(cfg, seed=3, std=0.06, bias_std=0.02, round_bf16=True)
    sd = ts.state_dict_numpy(model)
    att = RAJNIAttention(model.blocks[0].attn, keep_ratio=0.7, update=True).to(DEV).to(torch.bfloat16)
    x = ts.bf16_round_np(np.random.default_rng(4).standard_normal((2, 197, 192), dtype=np.float32))
    out, keep_idx, nxt = att(torch.from_numpy(x).to(DEV).to(torch.bfloat16))
    assert keep_idx.dtype == torch.int64 and tuple(keep_idx.shape) == (2, 138) and tuple(out.shape) == (2, 138, 192)
    assert (keep_idx[:, 0] == 0).all() and (keep_idx[:, 1:].diff(dim=1) > 0).all()
    want_out, _, want_nxt, _ = orc.rajni_attention(x, sd, "blocks.0.attn.", 3, 0.7, True, None,
                                                   forced_keep_idx=keep_idx.cpu().numpy())
    assert np.abs(out.float().cpu().numpy() - want_out).max() <= 1.5e-2 * np.abs(want_out).max()
    assert np.abs(nxt.float().cpu().numpy() - want_nxt).max() <= 1e-2 * np.abs(want_nxt).max()
    # prev_scores + update=False: pure selection of the given scores
    att2 = RAJNIAttention(model.blocks[1].attn, keep_ratio=0.5, update=False).to(DEV).to(torch.bfloat16)
    prev = torch.rand(2, 197, device=DEV).to(torch.bfloat16)
    _, ki, _ = att2(torch.from_numpy(x).to(DEV).to(torch.bfloat16), prev)
    np.testing.assert_array_equal(ki.cpu().numpy(), orc.select_tokens(prev.float().cpu().numpy(), 98))
    qkv = torch.randn(2, 50, 3 * 128, device=DEV).to(torch.bfloat16)
    sc = compute_importance(qkv, 2)
    assert sc.dtype == torch.bfloat16 and tuple(sc.shape) == (2, 50)
    want = orc.importance_scores(qkv.float().cpu().numpy(), 2)
    assert np.abs(sc.float().cpu().numpy() - want).max() <= 6e-3 * want.max()


def test_evaluate_model_on_device():
    cfg = ts.CONFIGS["vit_micro_patch16_64"]
    w = rajni_amd.RAJNIViTWrapper(ts.create_model(cfg, seed=0, std=0.08), {1: {"keep_ratio": 0.5}}).to(torch.bfloat16)
    g = torch.Generator().manual_seed(0)
    loader = [(torch.randn(8, 3, 64, 64, generator=g), torch.randint(0, 10, (8,), generator=g)) for _ in range(3)]
    acc, thr = rajni_amd.evaluate_model(w, loader, device="cuda", max_batches=2, warmup=4)
    assert 0.0 <= acc <= 100.0 and thr > 0
    # accuracy is exactly argmax agreement of the model's own logits
    w.to(DEV)
    correct = sum(int((w(x.to(DEV)).argmax(1).cpu() == y).sum()) for x, y in loader[:2])
    assert acc == pytest.approx(100.0 * correct / 16)


def test_cli_synthetic_run(capsys):
    """`python -m rajni_amd.run` equivalent on synthetic batches: prunes (B1 fixed) and reports."""
    from rajni_amd import run
    acc, thr = run.main(["--model", "vit_micro_patch16_64", "--batch_size", "8", "--max_batches", "2", "--warmup", "1",
                         "--compare_base", "--synthetic"])
    out = capsys.readouterr().out
    assert thr > 0 and 0 <= acc <= 100
    assert "Speedup" in out and "Token counts" in out


# ---------------------------------------------------------------------------------------------
# Full-size run (BASELINE.json configs[1]: ViT-B/16 @224, batch 256, README schedule): the oracle cannot
# finish this in seconds, so parity is carried by size-independent properties of the path.
# ---------------------------------------------------------------------------------------------
README_SCHEDULE = {3: {"keep_ratio": 0.88, "update": True}, 4: {"keep_ratio": 0.88, "update": True},
                   7: {"keep_ratio": 0.80, "update": True}, 8: {"keep_ratio": 0.72, "update": True}}


@pytest.fixture(scope="module")
def full_size():
    cfg = ts.CONFIGS["vit_base_patch16_224"]
    model = ts.create_model(cfg, seed=0).to(torch.bfloat16).to(DEV)
    wrapped = rajni_amd.RAJNIViTWrapper(model, README_SCHEDULE).eval().trace_scores(True)
    gen = torch.Generator(device=DEV).manual_seed(99)
    images = torch.randn(256, 3, 224, 224, generator=gen, device=DEV).to(torch.bfloat16)
    logits = wrapped(images).float()
    trace = {i: {k: v.clone() for k, v in d.items()} for i, d in wrapped.get_last_trace().items()}
    return cfg, wrapped, images, logits, trace


def test_full_size_token_counts_and_selection_invariants(full_size):
    cfg, wrapped, images, logits, trace = full_size
    assert wrapped.get_last_stats()["token_counts"] == [197, 197, 197, 197, 173, 152, 152, 152, 121, 87, 87, 87]
    assert torch.isfinite(logits).all() and tuple(logits.shape) == (256, 1000)
    n_in = {3: 197, 4: 173, 7: 152, 8: 121}
    for i, d in trace.items():
        idx = d["keep_idx"]
        keep = idx.shape[1] - 1
        assert keep == orc.keep_count(README_SCHEDULE[i]["keep_ratio"], n_in[i])
        assert (idx[:, 0] == 0).all()                                   # CLS first (attention.py:39-40)
        assert (idx[:, 1:] > idx[:, :-1]).all()                          # strictly ascending = sorted and unique
        assert int(idx.max()) < n_in[i]
        # the kept set is EXACTLY the top-k of the scores the device ranked (ties: lower index first),
        # checked for every one of the 256 images with the oracle's integer rule
        s = d["scores"].float().cpu().numpy().astype(np.float64)
        np.testing.assert_array_equal(idx.cpu().numpy(), orc.select_tokens(s, keep))
        # carried scores are the ranked scores at the kept positions (attention.py:58)
        np.testing.assert_array_equal(d["next_scores"].float().cpu().numpy(),
                                      np.take_along_axis(s, idx.cpu().numpy(), axis=1).astype(np.float32))


def test_full_size_images_are_independent(full_size):
    """No cross-image term anywhere in the path (images shard freely): any sub-batch gives
    bit-identical logits and selections - also across different GEMM tile decompositions (M changes)."""
    cfg, wrapped, images, logits, trace = full_size
    for lo, hi in ((0, 64), (37, 38), (100, 256)):
        sub = wrapped(images[lo:hi]).float()
        assert torch.equal(sub, logits[lo:hi]), f"images {lo}:{hi} differ from the full-batch run"
        for i, d in wrapped.get_last_trace().items():
            assert torch.equal(d["keep_idx"], trace[i]["keep_idx"][lo:hi])
    wrapped(images)   # leave the fixture's plan as it was


def test_full_size_forcing_own_selection_is_idempotent(full_size):
    """Injecting the device's own keep_idx must reproduce the free-running logits bit for bit: the forced
    path (test hook) and the selecting path share every kernel but the top-k."""
    cfg, wrapped, images, logits, trace = full_size
    wrapped.force_keep_idx({i: d["keep_idx"] for i, d in trace.items()})
    try:
        assert torch.equal(wrapped(images).float(), logits)
    finally:
        wrapped.force_keep_idx(None)


def test_full_size_fp8_weights_same_invariants(full_size):
    cfg, wrapped, images, logits, trace = full_size
    wrapped.set_weight_format("fp8")
    try:
        l8 = wrapped(images).float()
        assert torch.isfinite(l8).all()
        assert wrapped.get_last_stats()["token_counts"] == [197, 197, 197, 197, 173, 152, 152, 152, 121, 87, 87, 87]
        for i, d in wrapped.get_last_trace().items():
            idx = d["keep_idx"]
            assert (idx[:, 0] == 0).all() and (idx[:, 1:] > idx[:, :-1]).all()
        sub = wrapped(images[5:9]).float()
        assert torch.equal(sub, l8[5:9])
    finally:
        wrapped.set_weight_format("model")


def test_large_384_aggressive_schedule_properties():
    """BASELINE.json configs[3]: ViT-L/16 @384 (577 tokens, chunked attention, 24 blocks) with the aggressive
    schedule {4: .7, 12: .5, 20: .3}: token counts, selection invariants, sub-batch bit-identity."""
    cfg = ts.CONFIGS["vit_large_patch16_384"]
    sched = {4: {"keep_ratio": 0.7}, 12: {"keep_ratio": 0.5}, 20: {"keep_ratio": 0.3}}
    model = ts.create_model(cfg, seed=1).to(torch.bfloat16).to(DEV)
    wrapped = rajni_amd.RAJNIViTWrapper(model, sched).eval().trace_scores(True)
    gen = torch.Generator(device=DEV).manual_seed(5)
    images = torch.randn(24, 3, 384, 384, generator=gen, device=DEV).to(torch.bfloat16)
    logits = wrapped(images).float()
    assert wrapped.get_last_stats()["token_counts"] == [577] * 5 + [404] * 8 + [202] * 8 + [61] * 3
    assert torch.isfinite(logits).all()
    trace = {i: {k: v.clone() for k, v in d.items()} for i, d in wrapped.get_last_trace().items()}
    for i, d in trace.items():
        idx = d["keep_idx"]
        assert (idx[:, 0] == 0).all() and (idx[:, 1:] > idx[:, :-1]).all()
        s = d["scores"].float().cpu().numpy().astype(np.float64)
        np.testing.assert_array_equal(idx.cpu().numpy(), orc.select_tokens(s, idx.shape[1] - 1))
    sub = wrapped(images[7:12]).float()
    assert torch.equal(sub, logits[7:12])
    for i, d in wrapped.get_last_trace().items():
        assert torch.equal(d["keep_idx"], trace[i]["keep_idx"][7:12])


def test_weight_changes_are_picked_up():
    """The wrapper packs the base model's weights once and caches them (and the parameter list): in-place
    edits, load_state_dict, a replaced Parameter object and a replaced module must all invalidate the cache on the
    NEXT forward (Q4: the wrapper shares parameters with the base model; the reference reads the live modules on
    every call)."""
    cfg = ts.CONFIGS["vit_micro_patch16_64"]
    model = ts.create_model(cfg, seed=3, std=0.08, bias_std=0.02, round_bf16=True)
    w = rajni_amd.RAJNIViTWrapper(model, {1: {"keep_ratio": 0.7}}).to(DEV).to(torch.bfloat16).eval()
    x = torch.randn(2, 3, 64, 64, device=DEV).to(torch.bfloat16)
    y0 = w(x).float()
    assert torch.equal(w(x).float(), y0)
    with torch.no_grad():
        model.head.bias.add_(1.0)                                  # in place: _version changes
    y1 = w(x).float()
    assert torch.allclose(y1, y0 + 1.0, atol=2e-2)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    sd["head.bias"] = sd["head.bias"] - 1.0
    model.load_state_dict(sd)                                       # copy_ into the same storage
    assert torch.allclose(w(x).float(), y0, atol=2e-2)
    model.head.bias = torch.nn.Parameter(model.head.bias.detach() + 2.0)   # a NEW Parameter object ...
    assert torch.allclose(w(x).float(), y0 + 2.0, atol=3e-2)              # ... is seen on the very next forward
    # a replaced MODULE (the classic fine-tuning edit) too: new class count, new weights, next forward
    new_head = torch.nn.Linear(cfg.embed_dim, 7).to(DEV).to(torch.bfloat16)
    model.head = new_head
    y3 = w(x).float()
    assert y3.shape == (2, 7)
    feats = model.head.weight.float()
    with torch.no_grad():
        new_head.bias.add_(1.0)
    assert torch.allclose(w(x).float(), y3 + 1.0, atol=2e-2)
    del feats
    # and a replaced block-level Linear
    blk = model.blocks[0]
    old_fc2 = blk.mlp.fc2
    blk.mlp.fc2 = torch.nn.Linear(old_fc2.in_features, old_fc2.out_features).to(DEV).to(torch.bfloat16)
    y4 = w(x).float()
    assert not torch.allclose(y4, y3 + 1.0, atol=1e-3)
    blk.mlp.fc2 = old_fc2
    assert torch.equal(w(x).float(), w(x).float())
    assert torch.allclose(w(x).float(), y3 + 1.0, atol=2e-2)


@pytest.mark.parametrize("name,dtype,fp8", [("micro_fp32", torch.bfloat16, ""), ("base224_fp32", torch.bfloat16, ""),
                                            ("deit3_fp32", torch.bfloat16, ""), ("base224_fp32", torch.bfloat16, "fp8"),
                                            ("base224_fp32", torch.bfloat16, "fp8_mfma"), ("deit3_fp32", torch.bfloat16, "fp8_mfma"),
                                            ("tiny224_fp32", torch.float32, "")])
def test_cls_only_last_block_gives_the_same_logits(name, dtype, fp8):
    """`set_last_block_cls_only(True)`: the last block is computed for the CLS row only (the head reads nothing
    else, model.py:65-66).  Same logits as the row-for-row forward up to summation order (the CLS attention
    row is a VALU kernel with an un-rounded P; the B-row GEMMs take the 128x128 tiling), same stats, same
    selections; and it stays within the parity bar against the reference fixture."""
    meta, data = load_case(name)
    cfg = ts.CONFIGS[meta["cfg_name"]]
    model = ts.create_model(cfg, seed=meta["seed"], std=meta["std"], bias_std=meta["bias_std"], round_bf16=True)
    wrapped = rajni_amd.RAJNIViTWrapper(model, meta["schedule"]).to(DEV).to(dtype).eval()
    if fp8:
        wrapped.set_weight_format(fp8)
    images = torch.from_numpy(case_images(meta, data)).to(DEV)
    forced = {i: torch.from_numpy(data[f"blk{i}.keep_idx"]).to(DEV) for i in pruned_blocks(meta)}
    wrapped.force_keep_idx(forced)
    full = wrapped(images).float().cpu().numpy()
    stats = wrapped.get_last_stats()
    wrapped.set_last_block_cls_only(True)
    fast = wrapped(images).float().cpu().numpy()
    assert wrapped.get_last_stats() == stats
    scale = np.abs(full).max()
    tol = 2e-5 if dtype == torch.float32 else 8e-3          # bf16 logits: one output ulp (2^-8 of the value) may flip
    if fp8 == "fp8_mfma":
        # the CLS-row branch runs LN2 -> e4m3 and the fp8 x fp8 fc1 / fc2 on B rows (forward.hip: act_fp8 with
        # cls_only_last_block): its CLS attention row is not rounded like the packed kernel's, so a few of the last block's
        # e4m3 codes of the CLS rows flip - one block deep, no compounding (measured: max 4-5e-3, rms 1.1e-3 of the scale).
        tol = 1.5e-2
        rms = float(np.sqrt(np.mean((fast - full) ** 2)))
        print(f"\ncls-only + fp8_mfma {name}: max {np.abs(fast - full).max() / scale:.4g} rms {rms / scale:.4g} of the logit scale")
        assert rms <= 3e-3 * scale
        assert (fast.argmax(1) == full.argmax(1)).mean() >= 0.9
    assert np.abs(fast - full).max() <= tol * scale, np.abs(fast - full).max() / scale
    if not fp8:
        ref = data["logits"]
        assert np.abs(fast - ref).max() <= (1e-3 if dtype == torch.float32 else 1e-2) * np.abs(ref).max()
    wrapped.set_last_block_cls_only(False)
    assert np.array_equal(wrapped(images).float().cpu().numpy(), full)


def test_cls_only_last_block_is_skipped_when_the_last_block_prunes():
    cfg = ts.CONFIGS["vit_micro_patch16_64"]
    model = ts.create_model(cfg, seed=2, std=0.08, bias_std=0.02, round_bf16=True)
    w = rajni_amd.RAJNIViTWrapper(model, {3: {"keep_ratio": 0.5}}).to(DEV).to(torch.bfloat16).eval()
    x = torch.randn(3, 3, 64, 64, device=DEV).to(torch.bfloat16)
    ya = w(x)                    # kept alive until the second call has returned: it cannot inherit this block
    yb = w.set_last_block_cls_only(True)(x)
    a, b = ya.float(), yb.float()
    assert torch.equal(a, b) and w.get_last_trace()[3]["keep_idx"].shape[1] == orc.keep_count(0.5, 17) + 1


def test_forward_on_a_side_stream_and_changing_batch_shapes():
    """The launches go to torch's CURRENT stream ("current stream only, no host sync inside forward"):
    a forward enqueued on a side stream behind a slow producer must see the producer's data, and plans for
    different batch / image shapes coexist (one native plan per shape)."""
    meta, data = load_case("micro_fp32")
    cfg, wrapped = build(meta)
    images = torch.from_numpy(case_images(meta, data)).to(DEV).to(torch.bfloat16)
    want = wrapped(images).float()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        junk = torch.randn(4096, 4096, device=DEV)
        for _ in range(20):
            junk = junk @ junk * 1e-3                 # keeps the side stream busy
        staged = torch.empty_like(images)
        staged.copy_(images)                          # produced ON the side stream, behind the matmuls
        got = wrapped(staged).float()
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(got, want)
    # other shapes in between, then the first shape again
    for b in (1, 7, 4):
        y = wrapped(images[:1].repeat(b, 1, 1, 1))
        assert y.shape[0] == b
        assert torch.equal(y.float(), want[:1].expand(b, -1))
    assert torch.equal(wrapped(images).float(), want)
