"""The pairwise crossing of every model option (tests/numerics_combined.py) without a GPU: the module-driven reference against
the seven per-feature restatements, the coverage of the case list recomputed from the axes, every refused pair shown to raise,
every case accepted by the host with a descriptor that says what the config says, and the committed seeds held to their purpose -
switching one option of a case off moves the reference's output by 5 x the case's bar."""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

import numerics_activations as nact
import numerics_attnpool as nap
import numerics_combined as nc
import numerics_distilled as nd
import numerics_noclass as nq
import numerics_prefix as npx
import numerics_swiglu as ns
import numerics_variants as nv
import rajni_amd
from rajni_amd import timm_shaped as ts


@functools.lru_cache(maxsize=None)
def cases():
    return nc.generate_cases()


CASE_IDS = [c["id"] for c in cases()]


# ---- 1. the anchor ---------------------------------------------------------------------------------------------------------------

SCHED = nq.SCHED
# (restatement, its micro configs, its schedule): each file's own
ANCHORS = [
    ("prefix", ["vit_micro_patch16_64", "vit_micro_reg4_patch16_64", "deit3_micro_reg4_patch16_64", "vit_micro_reg1_gap_patch14_56"], SCHED),
    ("variants", ["vit_micro_qknorm_patch16_64", "vit_micro_prenorm_patch16_64", "vit_micro_gap_patch16_64", "vit_micro_fcnorm_patch16_64",
                  "vit_micro_all_patch16_64", "vit_micro_d80_qknorm_patch16_64"], SCHED),
    ("activations", ["vit_micro_quickgelu_patch16_64", "vit_micro_clip_quickgelu_patch16_64", "vit_micro_quickgelu_h344_patch16_64"], SCHED),
    ("swiglu", ["vit_micro_swiglu_patch16_64", "vit_micro_swiglu_split_patch16_64", "vit_micro_swiglu_h344_patch16_64",
                "vit_micro_reg4_swiglu_patch14_56"], ns.SCHED),
    ("distilled", ["vit_micro_distilled_patch16_64"], nd.SCHEDULES["carried"]),
    ("distilled", ["vit_micro_distilled_patch16_64"], nd.SCHEDULES["last"]),
    ("noclass", ["vit_micro_nocls_gap_patch16_64", "vit_micro_reg4_nocls_gap_patch16_64", "vit_micro_reg1_nocls_gap_d80_patch16_64",
                 "vit_micro_gap_patch16_64"], SCHED),
    ("attnpool", ["vit_micro_map_patch16_64", "vit_micro_cls_map_patch16_64", "vit_micro_reg4_map_d80_patch16_64"], nap.SCHED),
]


def _restated(which, sd, imgs, sched, cfg):
    if which == "prefix":
        return npx.vit_forward_restated(sd, imgs, sched, cfg)
    if which == "variants":
        return nv.vit_forward_restated(sd, imgs, sched, cfg)
    if which == "activations":
        return nact.vit_forward_restated(sd, imgs, sched, cfg, nact.quick_gelu_torch)
    if which == "swiglu":
        return ns.vit_forward_restated(sd, imgs, sched, cfg)
    if which == "distilled":
        return nd.vit_forward_restated(sd, imgs, sched, cfg)
    if which == "noclass":
        return nq.vit_forward_restated(sd, imgs, sched, cfg)
    return nap.vit_forward_restated(sd, imgs, sched, cfg)


@pytest.mark.parametrize("n", range(len(ANCHORS)))
def test_the_reference_is_each_of_the_seven_restatements_on_their_own_configs(n):
    which, names, sched = ANCHORS[n]
    for name in names:
        cfg = ts.config_of(name)
        model = ts.create_model(cfg, seed=7, round_bf16=True, **nc.FIX_BASE)
        sd = ts.state_dict_numpy(model)
        imgs = nq.images_of(cfg, 3, 11)
        want, counts, tr = _restated(which, sd, imgs, sched, cfg)
        got = nc.reference_forward(model, imgs, sched)
        assert got.counts == counts and sorted(got.trace) == sorted(tr)
        for i in tr:
            np.testing.assert_array_equal(got.trace[i]["keep_idx"], tr[i]["keep_idx"], err_msg=f"{which} {name} block {i}")
        scale, err = float(np.abs(want).max()), float(np.abs(got.out - want).max())
        print(f"[combined] anchor {which} {name}: max |d| {err:.3g} (logit scale {scale:.3g})")
        assert err <= 1e-12 * scale, (which, name, err, scale)


def test_the_reference_takes_a_mean_query_forced_selections_and_the_feature_surfaces_of_the_noclass_helper():
    """numerics_noclass's forced selections, named query and feature_outputs, on its R = 4 model (no stage at block 0, where that
    helper stops); and the generalisation: a stage at block 0 leaves the embedded stream's rows behind"""
    name = "vit_micro_reg4_nocls_gap_patch16_64"
    cfg = ts.config_of(name)
    model = ts.create_model(cfg, seed=7, round_bf16=True, **nc.FIX_BASE)
    sd, imgs = ts.state_dict_numpy(model), nq.images_of(cfg, 3, 11)
    want = nq.feature_outputs(sd, imgs, SCHED, cfg, caps=(1, 3))
    ref = nc.reference_forward(model, imgs, SCHED)
    got = nc.feature_surfaces(ref, caps=(1, 3), norm=False)
    for k in ("tokens", "dense", "dense_last"):
        assert np.abs(got[k] - want[k]).max() <= 1e-12 * np.abs(want[k]).max(), k
    np.testing.assert_array_equal(got["source_idx"], want["source_idx"])
    np.testing.assert_array_equal(got["exit_block"], want["exit_block"])
    for c in (1, 3):
        assert np.abs(got["slabs"][c] - want["slabs"][c]).max() <= 1e-12 * np.abs(want["slabs"][c]).max()
    cls = "vit_micro_gap_patch16_64"
    m2 = ts.create_model(ts.config_of(cls), seed=7, round_bf16=True, **nc.FIX_BASE)
    x2 = nq.images_of(ts.config_of(cls), 2, 3)
    a = nc.reference_forward(m2, x2, SCHED, query="mean")
    w2, _, tr2 = nq.vit_forward_restated(ts.state_dict_numpy(m2), x2, SCHED, ts.config_of(cls), query="mean")
    assert np.abs(a.out - w2).max() <= 1e-12 * np.abs(w2).max()
    b = nc.reference_forward(m2, x2, SCHED, forced_keep={i: t["keep_idx"] for i, t in tr2.items()}, query="cls")
    assert all(np.array_equal(b.trace[i]["keep_idx"], tr2[i]["keep_idx"]) for i in tr2)
    # a stage at block 0: the rows it drops hold norm(the embedded stream), exit_block 0, nothing zero
    first = nc.reference_forward(model, imgs, nc.SCHEDULES["first"])
    f = nc.feature_surfaces(first)
    gone = f["exit_block"] == 0
    assert gone.sum() == 3 * (16 - npx.keep_count(0.72, 20, 4)) and not gone[:, :4].any()
    np.testing.assert_array_equal(f["dense_last"][gone], first.normed_entries[0][gone])
    assert (np.abs(f["dense_last"]).max(axis=-1) > 0).all() and not f["dense"][gone].any()
    assert set(np.unique(f["exit_block"])) == {0, 4}      # (block 2 of that schedule keeps everything)


# ---- 2. coverage -----------------------------------------------------------------------------------------------------------------

def test_every_legal_pair_is_covered_and_the_list_is_what_the_generator_returns():
    listed = cases()
    assert listed == nc.generate_cases() and len({c["id"] for c in listed}) == len(listed)
    covered = set()
    for c in listed:
        assert set(c) == set(nc.AXES) | {"id"} and all(c[a] in nc.AXES[a] for a in nc.AXES)
        assert nc.refused_in(c) == [], (c["id"], nc.refused_in(c))
        items = nc.case_items(c)
        covered |= {frozenset((a, b)) for n, a in enumerate(items) for b in items[n + 1:]}
    refused = {frozenset((a, b)) for a, b, _, _ in nc.REFUSED_PAIRS}
    assert len(refused) == len(nc.REFUSED_PAIRS)
    every = {frozenset(p) for p in nc.all_pairs()}
    assert refused < every
    missing = every - refused - covered
    assert not missing, sorted(map(sorted, missing))[:10]
    print(f"[combined] {len(listed)} cases cover {len(every - refused)} legal pairs of {len(every)}; {len(refused)} refused")
    assert len(listed) <= 64 and all(c["batch"] <= 3 for c in listed)


# ---- 3. no pair hides behind "illegal" -------------------------------------------------------------------------------------------

def host_prepare(case):
    """everything the host does for a case, without a device: config, model, wrapper, setters, check_supported(), and the
    refusals of the case's output surface and weight format.  Returns (wrapper, descriptor)."""
    model = nc.build_model(case, 1)
    w = rajni_amd.RAJNIViTWrapper(model, nc.SCHEDULES[case["schedule"]]).to(nc.TORCH[nc.model_dtype(case)]).eval()
    if case["dtype"].endswith("_stream"):
        w.set_residual_dtype(nc.TORCH[nc.model_dtype(case)])
    w.set_weight_format(case["weights"])
    if case["query"] == "mean":
        w.set_importance_query("mean")
    if case["last"] == "cls_only":
        w.set_last_block_cls_only(True)
    if nc.INPUTS[case["input"]][2] is not None:
        w.set_dynamic_img_size(True)
    d = w.check_supported()
    if case["output"] in ("tokens", "dense_last"):
        w._check_features(d)
    elif case["output"] in ("inter", "gil"):
        caps = tuple(nc.INTER_INDICES) if case["output"] == "inter" else nc.GIL_BLOCKS
        w._check_layers(dict(norm=d["norm"], depth=d["depth"]), caps, case["output"] == "inter")
    if case["weights"] == "fp8" and nc.model_dtype(case) != "bf16":
        w._pack_weights(torch.device("cpu"), nc.TORCH[nc.model_dtype(case)])
    return w, d


def case_around(a, b):
    """a case that holds the refused pair (a, b): every other axis takes the first value legal with all chosen so far, else the
    first legal with all but a, else its first value (some refused pairs force a second one: no head is legal with both
    cls_only and a model without a class token - the model is then built as its config allows, and the setter refuses)"""
    case = {a[0]: a[1], b[0]: b[1]}
    for axis, vals in nc.AXES.items():
        if axis in case:
            continue
        legal = lambda v, skip=None: all(nc.pair_is_legal((axis, v), it) for it in case.items() if it != skip)
        ok = [v for v in vals if legal(v)] or [v for v in vals if legal(v, a)] or list(vals)
        case[axis] = ok[0]
    return case


@pytest.mark.parametrize("n", range(len(nc.REFUSED_PAIRS)))
def test_every_refused_pair_raises_on_the_host_with_the_option_named(n):
    a, b, source, word = nc.REFUSED_PAIRS[n]
    assert a[1] in nc.AXES[a[0]] and b[1] in nc.AXES[b[0]] and a[0] != b[0] and source
    case = case_around(a, b)
    with pytest.raises((ValueError, NotImplementedError)) as e:
        host_prepare(case)
    assert word in str(e.value), (a, b, str(e.value))


# ---- 4. every case is accepted by the host -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", CASE_IDS)
def test_the_host_accepts_the_case_and_describes_what_the_config_says(cid):
    case = cases()[CASE_IDS.index(cid)]
    cfg = nc.config_of(case)
    w, d = host_prepare(case)
    gated = cfg.mlp != "mlp"
    assert d["mlp_act"] == ("swiglu" if gated else cfg.act)
    assert d["pool"] == cfg.global_pool and d["num_prefix"] == cfg.num_prefix_tokens and d["class_token"] is cfg.class_token
    assert d["head_rows"] == (2 if cfg.distilled else 1)
    assert d["fc_norm"] is cfg.use_fc_norm and d["norm"] is (not cfg.use_fc_norm) and d["norm_pre"] is cfg.pre_norm
    assert d["qk_norm"] is cfg.qk_norm and d["hidden"] == cfg.hidden_dim and d["hidden_pad"] == (cfg.hidden_dim + 63) // 64 * 64
    assert (d["hidden_pad"] != d["hidden"]) == (case["width"] == "odd")
    assert d["headless"] is (case["classifier"] == "headless") and d["num_classes"] == (0 if d["headless"] else 10)
    assert (d["C"], d["H"], d["D"], d["depth"], d["patch"]) == (cfg.embed_dim, cfg.num_heads, cfg.head_dim, 4, cfg.patch_size)
    if cfg.global_pool == "map":
        assert d["attn_pool"] == dict(heads=cfg.num_heads, hidden=cfg.hidden_dim, hidden_pad=d["hidden_pad"], act=cfg.act, eps=cfg.ln_eps)
    else:
        assert "attn_pool" not in d
    assert w.importance_query == nc.effective_query(case)
    has_ls = all(isinstance(blk.ls1, ts.LayerScale) for blk in w.blocks)
    assert has_ls is (case["layer_scale"] == "on")
    assert w.m.pos_embed.shape[1] == cfg.num_patches + (0 if cfg.no_embed_class else cfg.num_prefix_tokens)
    assert isinstance(w.m.head, nn.Identity) is d["headless"]


# ---- 5. a wrong answer would move the output ---------------------------------------------------------------------------------------

MUST_SEPARATE = {"registers", "dist_token", "head_alone", "quick_gelu", "gate", "pool"}      # MLP kind, prefix count, head kind


def test_the_seed_table_names_every_case_and_nothing_else():
    assert set(nc.SEEDS) == set(CASE_IDS)
    assert set(nc.UNSEPARATED) <= set(CASE_IDS) and not set(nc.UNSEPARATED.values()) & MUST_SEPARATE


@pytest.mark.parametrize("cid", CASE_IDS)
def test_switching_one_option_off_moves_the_reference_past_the_bar(cid):
    case = cases()[CASE_IDS.index(cid)]
    wseed, iseed = nc.SEEDS[cid]
    ratios = nc.separations(case, wseed, iseed)
    assert sorted(ratios) == sorted(nc.options_on(case))
    print(f"[combined] {cid}: moved / (5 x bar {nc.logits_bar(case):g} x scale{'; quick_gelu: 5 x 1e-3, its fp32 twin' if nc.activation_twin(case) else ''}): "
          + ", ".join(f"{k} {v:.2f}" for k, v in sorted(ratios.items())))
    short = sorted(k for k, v in ratios.items() if v < 1.0)
    assert short == ([nc.UNSEPARATED[cid]] if cid in nc.UNSEPARATED else []), (cid, ratios)
    # and the draw leaves the format room: an ideal forward of the case's 16-bit format, no device involved, within 0.75 bar
    cost, spread = nc.format_cost(case, wseed, iseed), nc.format_spread(case, wseed, iseed)
    print(f"[combined] {cid}: the {case['dtype']} format alone costs {cost:.2f} of the bar, the largest of {nc.SPREAD_DRAWS} random "
          f"draws of its roundings {spread:.2f}")
    assert cost <= nc.FORMAT_HEADROOM and spread <= nc.FORMAT_HEADROOM, (cid, cost, spread)
