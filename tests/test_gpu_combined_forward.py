"""Whole forwards of the pairwise crossing of every model option (tests/numerics_combined.py::generate_cases) on the device: one
parametrised test per case.  GPU box only (`-m gpu`).

Each case: (1) free-running with traced scores, the device's selections are the restated rule on the device's own scores
(tests/test_gpu_long_forward.py's rule: no case hinges on a near-tie) and the token counts are the plan's; (2) the output - logits
or pooled row, and the case's feature surface - against numerics_combined.reference_forward on those selections (on the
dequantised weights under "fp8"), at the bar the project already holds for the condition; (3) the bit identities the headers
promise; (4) every debug hook a case sets is reset in `finally`.  The plan the forward ran with is read back (activation code,
prefix count, head rows, pool, query, stream), and a 16-bit QuickGELU case also runs its fp32 twin at 1e-3: the two
activations differ by about one 16-bit bar, so only the twin can tell a forward that wired the wrong one.

The bars, each from the test that owns the condition (none is new, none is loosened; all in units of max|reference|):
  logits, fp32 model                       1e-3   test_gpu_prefix_forward.py / test_gpu_noclass_forward.py / test_gpu_attnpool_forward.py BAR
  logits, bf16 / fp16 model, fp32 stream   1e-2   the same BAR tables (test_gpu_forward.py holds 1.5e-2 for one attention kernel's
                                                  output, not for logits)
  logits, 16-bit residual stream           2e-2   test_gpu_prefix_forward.py, test_gpu_variants_forward.py, test_gpu_noclass_forward.py,
                                                  test_gpu_attnpool_forward.py ("the project's 2e-2 bar")
  logits, e4m3 weights                     1e-2   against the dequantised weights: test_gpu_attnpool_forward.py
                                                  ::test_fp8_weights_leave_the_pool_in_the_model_dtype, test_gpu_fp8.py; with the 16-bit
                                                  stream as well the stream's 2e-2 (test_gpu_prefix_forward.py's micro512 stream case)
  pooled row of a headless model           max(the logits bar, 1.5 x d16)   test_gpu_features.py (bar_pooled); test_gpu_attnpool_forward.py
                                                  holds the plain bar for the same row - the looser of the two is taken
  tokens / dense / fill="last" / slabs     max(1e-2 | 1e-3, 1.5 x d16)      test_gpu_features.py, test_gpu_features_last.py,
                                                  test_gpu_layers.py (with and without the 16-bit stream), test_gpu_noclass_forward.py
  set_last_block_cls_only(True) vs off     8e-3 16-bit, 2e-5 fp32           test_gpu_forward.py::test_cls_only_last_block_gives_the_same_logits
d16 is the same graph on the same selections in the model's 16-bit type on the CPU (0 for fp32)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import numerics_combined as nc
import numerics_prefix as npx
import rajni_amd
from rajni_amd import _native as nat

DEV = "cuda"
CASES = nc.generate_cases()
CASE_IDS = [c["id"] for c in CASES]
FEATURE_BAR = {"bf16": 1e-2, "fp16": 1e-2, "fp32": 1e-3}
CLS_ONLY_TOL = {"bf16": 8e-3, "fp16": 8e-3, "fp32": 2e-5}


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def set_hooks(case, on):
    lib = nat.lib()
    lib.rajni_debug_force_score_two_pass(int(on and case["score"] == "two_pass"))
    lib.rajni_debug_force_score_tiled(int(on and case["score"] == "tiled"))
    lib.rajni_debug_set_last_block_all_rows(int(on and case["last"] == "all_rows"))


def traced_selections(w, P):
    """{block: keep_idx} of the last forward, each checked against the restated rule on the device's own traced scores"""
    forced = {}
    for i, t in w.get_last_trace().items():
        idx = t["keep_idx"].cpu().numpy()
        s = t["scores"].float().cpu().numpy()
        np.testing.assert_array_equal(idx, npx.select_tokens(s.astype(np.float64), idx.shape[1] - P, P), err_msg=f"block {i}")
        assert np.array_equal(t["next_scores"].float().cpu().numpy(), np.take_along_axis(s, idx, axis=1)), f"block {i}: next_scores"
        forced[i] = idx
    return forced


class Worst:
    """the largest error / bar of a case, and where"""

    def __init__(self, cid):
        self.cid, self.ratio, self.what, self.failed = cid, 0.0, "-", []

    def close(self, got, want, bar, what):
        got = got.float().cpu().numpy() if isinstance(got, torch.Tensor) else got
        assert got.shape == want.shape, (what, got.shape, want.shape)
        scale, err = float(np.abs(want).max()), float(np.abs(got - want).max())
        r = err / (bar * scale)
        print(f"[combined] {self.cid} {what}: max |d| {err:.4g} (scale {scale:.4g}, bar {bar:.3g}): {r:.3f} of the bar")
        if r > self.ratio:
            self.ratio, self.what = r, what
        if not r <= 1.0:
            self.failed.append(f"{what}: max |d| {err:.4g} vs {bar:.3g} x {scale:.4g}")


def d16_of(ref16, ref, key=None):
    a, b = (ref16, ref) if key is None else (ref16[key], ref[key])
    return float(np.abs(a - b).max() / np.abs(b).max())


def wrapped(case, wseed):
    """the case's wrapper on the device with every option of the case set, scores traced"""
    tdt = nc.TORCH[nc.model_dtype(case)]
    w = rajni_amd.RAJNIViTWrapper(nc.build_model(case, wseed), nc.SCHEDULES[case["schedule"]]).to(DEV).to(tdt).eval()
    if case["dtype"].endswith("_stream"):
        w.set_residual_dtype(tdt)
    w.set_weight_format(case["weights"])
    if case["query"] == "mean":
        w.set_importance_query("mean")
    if case["last"] == "cls_only":
        w.set_last_block_cls_only(True)
    if nc.INPUTS[case["input"]][2] is not None:
        w.set_dynamic_img_size(True)
    return w.trace_scores(True)


MLP_CODE = {"gelu": nat.MLP_GELU, "quick_gelu": nat.MLP_QUICK_GELU, "swiglu_packed": nat.MLP_SWIGLU, "swiglu": nat.MLP_SWIGLU}


def check_plan_says_what_the_case_says(w, case, cfg):
    """the records the forward just ran with: the activation code, the prefix count, the head rows, the pool, the stream"""
    plan, ext, pre, qry, apr = w._plan[1], w._plan[2][4], w._plan[2][6], w._plan[8][4], w._plan[8][5]
    assert (ext.mlp_act if ext is not None else nat.MLP_GELU) == MLP_CODE[case["mlp"]], "mlp_act"
    P = cfg.num_prefix_tokens
    assert (pre.num_prefix if pre is not None else int(cfg.class_token)) == P, "num_prefix"
    assert (pre.head_rows if pre is not None else 0) == (2 if cfg.distilled else 0), "head_rows"
    assert (qry is not None) == (nc.effective_query(case) == "mean") and (qry is None or qry.class_token == int(cfg.class_token))
    assert (apr is not None) == (cfg.global_pool == "map")
    pool = {"avg": nat.POOL_AVG, "map": nat.POOL_MAP}.get(cfg.global_pool, nat.POOL_TOKEN)
    assert (ext.pool if ext is not None else nat.POOL_TOKEN) == pool, "pool"
    assert plan.resid_bf16 == int(case["dtype"].endswith("_stream")) and plan.cls_only_last_block == int(case["last"] == "cls_only")
    assert plan.hidden == (cfg.hidden_dim + 63) // 64 * 64 and plan.dtype == nat.dtype_code(nc.TORCH[nc.model_dtype(case)])


def fp32_twin_tells_the_activations_apart(case, wseed, imgs, worst):
    """A 16-bit QuickGELU case cannot tell QuickGELU from exact GELU (they differ by about one of its bars): its fp32 twin - the
    same model, options, schedule and hooks in fp32 with the model's weight format - is held to 1e-3, the bar the separation
    check of tests/test_combined_cpu.py is stated for."""
    twin = nc.activation_twin(case)
    if twin is None:
        return
    cfg, P = nc.config_of(twin), nc.config_of(twin).num_prefix_tokens
    w = wrapped(twin, wseed)
    got = w(torch.from_numpy(imgs).to(DEV)).clone()
    check_plan_says_what_the_case_says(w, twin, cfg)
    forced = traced_selections(w, P)
    ref = nc.reference_forward(nc.reference_model(twin, nc.build_model(twin, wseed)), imgs, nc.SCHEDULES[twin["schedule"]], forced,
                               nc.effective_query(twin))
    assert w.get_last_stats()["token_counts"] == ref.counts
    worst.close(got, ref.out, nc.logits_bar(twin), "fp32 twin")


@pytest.mark.parametrize("cid", CASE_IDS)
def test_combined_forward(cid):
    case = CASES[CASE_IDS.index(cid)]
    cfg = nc.config_of(case)
    wseed, iseed = nc.SEEDS[cid]
    dt = nc.model_dtype(case)
    tdt = nc.TORCH[dt]
    sched = nc.SCHEDULES[case["schedule"]]
    P, depth, Cd, B = cfg.num_prefix_tokens, cfg.depth, cfg.embed_dim, case["batch"]
    imgs = nc.images_of(case, iseed)
    h, wd = nc.image_size(case)
    n0 = (h // cfg.patch_size) * (wd // cfg.patch_size) + P
    counts = npx.token_counts(n0, depth, sched, P)
    worst = Worst(cid)
    lib = nat.lib()
    set_hooks(case, True)
    try:
        w = wrapped(case, wseed)
        x = torch.from_numpy(imgs).to(DEV)

        # ---- 1. free-running: the selections are the rule on the device's own scores
        free = w(x).clone()
        assert tuple(free.shape) == (B, Cd if case["classifier"] == "headless" else cfg.num_classes) and free.dtype == tdt
        assert w.get_last_stats()["token_counts"] == counts
        check_plan_says_what_the_case_says(w, case, cfg)
        forced = traced_selections(w, P)
        assert sorted(forced) == sorted(sched)
        for i, idx in forced.items():
            assert idx.shape == (B, counts[i + 1] if i + 1 < depth else npx.keep_count(sched[i]["keep_ratio"], counts[i], P) + P)

        # ---- 2. the output against the reference on those selections
        deq = w.dequantized_state_dict() if case["weights"] == "fp8" else None
        rm = nc.reference_model(case, nc.build_model(case, wseed), deq)
        q = nc.effective_query(case)
        ref = nc.reference_forward(rm, imgs, sched, forced, q)
        ref16 = nc.reference_forward(rm, imgs, sched, forced, q, dtype=tdt) if dt != "fp32" else None
        assert ref.counts == counts
        bar = nc.logits_bar(case)
        if case["classifier"] == "headless" and ref16 is not None:
            bar = max(bar, 1.5 * d16_of(ref16.out, ref.out))
        worst.close(free, ref.out, bar, "pooled row" if case["classifier"] == "headless" else "logits")

        # ---- 3. bit identities on the logits
        assert same_bits(w(x), free), "a second call returns other bits"
        if B > 1:
            assert same_bits(w(x[:1].contiguous()), free[:1]), "image 0 alone differs from image 0 inside the batch"
            assert same_bits(w(x), free)
        flip = int(case["last"] != "all_rows")
        lib.rajni_debug_set_last_block_all_rows(flip)
        try:
            assert same_bits(w(x), free), f"rajni_debug_set_last_block_all_rows({flip}) changes the bits"
        finally:
            lib.rajni_debug_set_last_block_all_rows(1 - flip)
        if case["last"] == "cls_only":
            full = w.set_last_block_cls_only(False)(x).clone()
            scale = float(full.float().abs().max())
            d = float((full.float() - free.float()).abs().max())
            print(f"[combined] {cid} cls_only vs all rows: {d / scale:.3g} of the scale (bar {CLS_ONLY_TOL[dt]:g})")
            assert d <= CLS_ONLY_TOL[dt] * scale, (d, scale)
            w.set_last_block_cls_only(True)
        w.force_keep_idx({i: torch.from_numpy(v).to(DEV) for i, v in forced.items()})
        assert same_bits(w(x), free), "forcing the device's own selections does not reproduce the free run"
        assert w.get_last_stats()["token_counts"] == counts

        # ---- the case's feature surface, free-running again: every call's selections are the rule on its own traced scores,
        #      and the ones the logits plan made
        w.force_keep_idx(None)

        def free_selections(what):
            sel = traced_selections(w, P)
            assert sorted(sel) == sorted(forced) and all(np.array_equal(sel[i], forced[i]) for i in forced), f"{what}: other selections"
            assert w.get_last_stats()["token_counts"] == counts

        out = case["output"]
        fbar = lambda d16: max(FEATURE_BAR[dt], 1.5 * d16)
        if out != "forward":
            caps = tuple(nc.INTER_INDICES) if out == "inter" else nc.GIL_BLOCKS if out == "gil" else ()
            norm = out != "gil"
            want = nc.feature_surfaces(ref, caps, norm)
            want16 = nc.feature_surfaces(ref16, caps, norm) if ref16 is not None else None
            d16 = lambda key, c=None: 0.0 if want16 is None else (d16_of(want16, want, key) if c is None else d16_of(want16[key][c], want[key][c]))
            gather = lambda t, src: torch.gather(t, 1, src.long()[:, :, None].expand(-1, -1, Cd))
        if out in ("tokens", "dense_last", "inter"):
            tokens = w.forward_features(x).clone()
            free_selections("forward_features")
            src = w.get_last_stats()["source_idx"]
            np.testing.assert_array_equal(src.cpu().numpy(), want["source_idx"])
            assert tuple(tokens.shape) == (B, want["tokens"].shape[1], Cd) and w.get_last_stats()["token_counts"] == counts
            dense = w.forward_features(x, dense=True).clone()
            free_selections("forward_features(dense=True)")
            assert tuple(dense.shape) == (B, n0, Cd) and same_bits(gather(dense, src), tokens), "dense != tokens scattered by source_idx"
            mask = torch.ones((B, n0), dtype=torch.bool, device=DEV).scatter_(1, src.long(), False)
            assert int(mask.sum()) == B * (n0 - tokens.shape[1]) and not dense[mask].contiguous().view(torch.uint8).any()
        if out == "tokens":
            worst.close(tokens, want["tokens"], fbar(d16("tokens")), "tokens")
        if out == "dense_last":
            last = w.forward_features(x, dense=True, fill="last").clone()
            free_selections('forward_features(fill="last")')
            stats = w.get_last_stats()
            np.testing.assert_array_equal(stats["exit_block"].cpu().numpy(), want["exit_block"])
            np.testing.assert_array_equal(stats["source_idx"].cpu().numpy(), want["source_idx"])
            assert same_bits(gather(last, src), tokens), 'fill="last" differs from the dense output on the surviving rows'
            assert not torch.isnan(last.float()).any() and bool((last[mask].float().abs().amax(dim=-1) > 0).all())
            worst.close(last, want["dense_last"], fbar(d16("dense_last")), 'dense, fill="last"')
        if out == "inter":
            final, inter = w.forward_intermediates(x, indices=nc.INTER_INDICES, norm=True, output_fmt="NLC", return_prefix_tokens=True)
            free_selections("forward_intermediates")
            assert same_bits(final, dense), "forward_intermediates' final is not forward_features(dense=True)"
            np.testing.assert_array_equal(w.get_last_stats()["exit_block"].cpu().numpy(), want["exit_block"])
            for c, (spatial, prefix) in zip(caps, inter):
                slab = torch.cat([prefix, spatial], 1).float().cpu().numpy()
                alive = want["exit_block"] > c
                assert not slab[~alive].any() and (np.abs(slab[alive]).max(axis=-1) > 0).all() and alive[:, :P].all(), f"alive mask of block {c}"
                worst.close(slab, want["slabs"][c], fbar(d16("slabs", c)), f"intermediate of block {c}")
        if out == "gil":
            got = w.get_intermediate_layers(x, n=len(caps), norm=False, fill="last")
            free_selections("get_intermediate_layers")
            np.testing.assert_array_equal(w.get_last_stats()["exit_block"].cpu().numpy(), want["exit_block"])
            assert len(got) == len(caps)
            for c, spatial in zip(caps, got):
                assert tuple(spatial.shape) == (B, n0 - P, Cd)
                worst.close(spatial, want["slabs_last"][c][:, P:], fbar(d16("slabs_last", c)), f"un-normed layer of block {c}")
        if out in ("inter", "gil"):
            # the logits plan with the layers record beside it: `logits` receives what it would have received without the record
            (beside, _), _ = w._run(x, ("layers", "logits", caps, norm, "zero" if out == "inter" else "last"))
            assert same_bits(beside[:, :free.shape[1]], free), "the logits beside the layers record are not the plain forward's"
        fp32_twin_tells_the_activations_apart(case, wseed, imgs, worst)
    finally:
        set_hooks(case, False)
        lib.rajni_debug_set_last_block_all_rows(0)
    print(f"[combined-headroom] {cid}  worst error / bar {worst.ratio:.3f}  ({worst.what})")
    assert not worst.failed, worst.failed
