#!/usr/bin/env python3
"""Bit identity of the whole forward between two builds of the library (GPU box): one forward per configuration on seeded
weights and inputs with the library named by RAJNI_HIP_LIB (as tools/fwd_time.py uses it), one line per configuration with
a sha256 (first 16 hex digits) over token_counts, the output, every slab and every traced keep_idx / next_scores / scores
buffer.  Run it in a fresh process per library and compare:

    RAJNI_HIP_LIB=$PWD/parent.so python tools/forward_identity.py > a.txt
    python tools/forward_identity.py > b.txt
    python tools/forward_identity.py --compare a.txt b.txt         # "name parent=... tree=... equal", exit 1 on a difference

  --only a,b        those configurations alone
  --trace-hash CSV  the launch list of a `rocprofv3 --kernel-trace --output-format csv -- python tools/forward_identity.py ...`
                    run: its length and a sha256 over the ordered (kernel name, grid, workgroup, LDS bytes) of every dispatch

Every micro configuration runs a 64-pixel, 4-block, 128-wide model at batch 3; base224_bf16_readme is ViT-B/16 at batch 8."""
import argparse
import csv
import hashlib
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rajni-vit_amd"))

CARRY = {1: {"keep_ratio": 0.75, "update": True}, 2: {"keep_ratio": 0.6, "update": False}}
LAST = {**CARRY, 3: {"keep_ratio": 0.7, "update": True}}
README = {3: {"keep_ratio": 0.88, "update": True}, 4: {"keep_ratio": 0.88, "update": True},
          7: {"keep_ratio": 0.80, "update": True}, 8: {"keep_ratio": 0.72, "update": True}}
MICRO = "vit_micro_patch16_64"

# name -> options: model, sched, dtype, batch, size (H, W), and what to set or call
CONFIGS = {
    "micro_bf16_update_then_carry": {},
    "micro_bf16_last_block_prunes": dict(sched=LAST),
    "micro_bf16_forced_trace_on": dict(sched=LAST, forced=True, trace=True),
    "micro_bf16_forced_trace_off": dict(sched=LAST, forced=True),
    "micro_bf16_trace_on": dict(trace=True),
    "micro_fp16": dict(dtype="float16", trace=True),
    "micro_fp32": dict(dtype="float32", trace=True),
    "micro_bf16_stream": dict(resid="bfloat16"),
    "micro_fp8_weights": dict(weights="fp8"),
    "micro_cls_only_optin": dict(cls_only=True),
    "micro_all_rows_hook": dict(all_rows=True),
    "micro_qk_norm": dict(model="vit_micro_qknorm_patch16_64"),
    "micro_pre_norm": dict(model="vit_micro_prenorm_patch16_64"),
    "micro_fc_norm": dict(model="vit_micro_fcnorm_patch16_64"),
    "micro_avg_pool_no_norm": dict(model="vit_micro_gap_patch16_64"),
    "micro_all_variants": dict(model="vit_micro_all_patch16_64"),
    "micro_registers_P5": dict(model="vit_micro_reg4_patch16_64", trace=True),
    "micro_deit3_layerscale": dict(model="deit3_micro_patch16_64"),
    "micro_long_tiled_scores": dict(model="vit_micro_patch16_400", trace=True),
    "micro_long_tiled_scores_forced": dict(model="vit_micro_reg4_patch16_400", forced=True, trace=True),
    # the records the list above predates
    "micro_distilled_carried": dict(model="vit_micro_distilled_patch16_64"),
    "micro_distilled_last_block_prunes": dict(model="vit_micro_distilled_patch16_64", sched=LAST),
    "micro_nocls_registers": dict(model="vit_micro_reg4_nocls_gap_patch16_64"),
    "micro_mean_query_on_cls": dict(query="mean"),
    "micro_map_nocls": dict(model="vit_micro_map_patch16_64"),
    "micro_map_cls": dict(model="vit_micro_cls_map_patch16_64"),
    "micro_rect_48x96": dict(size=(48, 96)),
    "micro_layers_13_norm0_zero": dict(layers=dict(norm=False, fill="zero")),
    "micro_layers_13_norm0_last": dict(layers=dict(norm=False, fill="last")),
    "micro_layers_13_norm1_zero": dict(layers=dict(norm=True, fill="zero")),
    "micro_layers_13_norm1_last": dict(layers=dict(norm=True, fill="last")),
    "micro_features_tokens": dict(features=dict()),
    "micro_features_dense": dict(features=dict(dense=True)),
    "micro_features_dense_last": dict(features=dict(dense=True, fill="last")),
    "micro_headless": dict(headless=True),
    "micro_swiglu": dict(model="vit_micro_swiglu_patch16_64"),
    "micro_quickgelu": dict(model="vit_micro_quickgelu_patch16_64"),
    # attention pool, no class row, registers, a rectangular input and a layers record: every record at once
    "micro_most_records": dict(model="vit_micro_reg4_map_d80_patch16_64", size=(48, 96),
                               layers=dict(norm=True, fill="last", intermediates_only=True)),
    "base224_bf16_readme": dict(model="vit_base_patch16_224", sched=README, batch=8),
}


def forced_selections(w, cfg, sched, B, size, gen):
    """a legal forced keep_idx per scheduled block: the prefix tokens, then ascending patch indices drawn with `gen`"""
    import torch
    from rajni_amd import ops
    P = cfg.num_prefix_tokens
    N = (size[0] // cfg.patch_size) * (size[1] // cfg.patch_size) + P
    forced = {}
    for i in sorted(sched):
        keep = ops.keep_count(sched[i]["keep_ratio"], N, P)
        rows = [torch.cat([torch.arange(P), torch.randperm(N - P, generator=gen)[:keep].sort().values + P]) for _ in range(B)]
        forced[i] = torch.stack(rows).to(torch.int32).cuda()
        N = keep + P
    return forced


def run(name, opt):
    import torch
    import torch.nn as nn
    import rajni_amd
    from rajni_amd import _native as nat, timm_shaped as ts
    cfg = ts.config_of(opt.get("model", MICRO))
    dtype = getattr(torch, opt.get("dtype", "bfloat16"))
    sched, B = opt.get("sched", CARRY), opt.get("batch", 3)
    size = opt.get("size", (cfg.img_size, cfg.img_size))
    base = ts.create_model(cfg, seed=0)
    if opt.get("headless"):
        base.head = nn.Identity()
    w = rajni_amd.RAJNIViTWrapper(base.to(dtype).cuda(), sched).eval()
    gen = torch.Generator().manual_seed(1234)
    x = torch.randn(B, cfg.in_chans, *size, generator=gen).to(dtype).cuda()
    if "resid" in opt:
        w.set_residual_dtype(getattr(torch, opt["resid"]))
    if "weights" in opt:
        w.set_weight_format(opt["weights"])
    if "query" in opt:
        w.set_importance_query(opt["query"])
    if size[0] != size[1]:
        w.set_dynamic_img_size(True)
    if opt.get("cls_only"):
        w.set_last_block_cls_only(True)
    if opt.get("trace"):
        w.trace_scores(True)
    if opt.get("forced"):
        w.force_keep_idx(forced_selections(w, cfg, sched, B, size, gen))
    nat.lib().rajni_debug_set_last_block_all_rows(1 if opt.get("all_rows") else 0)
    outs = {}
    if "layers" in opt:
        res = w.forward_intermediates(x, indices=(1, 3), output_fmt="NLC", return_prefix_tokens=True, **opt["layers"])
        final, inter = (None, res) if opt["layers"].get("intermediates_only") else res
        if final is not None:
            outs["final"] = final
        for l, (spatial, prefix) in enumerate(inter):
            outs[f"slab{l}.prefix"], outs[f"slab{l}.patches"] = prefix, spatial
    elif "features" in opt:
        outs["features"] = w.forward_features(x, **opt["features"])
    else:
        outs["logits"] = w(x)
    nat.lib().rajni_debug_set_last_block_all_rows(0)
    torch.cuda.synchronize()
    stats = w.get_last_stats()
    for i, bufs in sorted(w.get_last_trace().items()):
        for key in ("keep_idx", "next_scores", "scores"):
            if bufs.get(key) is not None:
                outs[f"{i}.{key}"] = bufs[key]
    h = hashlib.sha256(repr(list(stats["token_counts"])).encode())
    for key, t in outs.items():
        h.update(key.encode())
        h.update(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes())
    print(f"{name} sha256={h.hexdigest()[:16]}  (token_counts={list(stats['token_counts'])} buffers={','.join(outs)})", flush=True)


def compare(a, b):
    rows = [dict(line.split(" ", 1) for line in open(f) if " sha256=" in line) for f in (a, b)]
    same = rows[0].keys() == rows[1].keys()
    for name in rows[0]:
        pa, pb = rows[0][name].split("  ", 1), rows[1].get(name, "sha256=missing  ").split("  ", 1)
        ok = pa == pb
        same = same and ok
        print(f"{name} parent={pa[0][7:]} tree={pb[0][7:]} {'equal' if ok else 'DIFFERENT'}  {pa[1].strip()}")
    return 0 if same else 1


def trace_hash(path):
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r.get("Dispatch_Id") or r["Start_Timestamp"]))
    cols = ["Kernel_Name", "Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z", "Workgroup_Size_X", "Workgroup_Size_Y", "Workgroup_Size_Z",
            "LDS_Block_Size"]
    h = hashlib.sha256()
    for r in rows:
        h.update("\t".join(r[c] for c in cols).encode() + b"\n")
    print(f"kernel trace: {len(rows)} launches sha256 {h.hexdigest()[:16]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--trace-hash")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    if args.trace_hash:
        return trace_hash(args.trace_hash)
    for name in (args.only.split(",") if args.only else CONFIGS):
        run(name, CONFIGS[name])


if __name__ == "__main__":
    main()
