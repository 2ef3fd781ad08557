"""Cost of the attention-pool head at ViT-B/16 dims, bf16, batch 256, README schedule: vit_base_patch16_siglip_224 ('map')
against the same trunk with global_pool='avg' and no pool.  Device events around batches of forwards, the variants interleaved
round by round on one device (`profiles/attnpool_ab.txt`).

    python tools/attnpool_cost.py > profiles/attnpool_ab.txt
"""
import dataclasses, os, sys, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "rajni-vit_amd"), ROOT):
    sys.path.insert(0, p)
import torch
import rajni_amd
from rajni_amd import ops, timm_shaped as ts
from rajni_amd.run import README_SCHEDULE

DEV, B, ITERS, ROUNDS = "cuda", 256, 20, 7
cfg = ts.config_of("vit_base_patch16_siglip_224")
avg = dataclasses.replace(cfg, global_pool="avg", fc_norm=False)
wm = rajni_amd.RAJNIViTWrapper(ts.create_model(cfg, seed=1), README_SCHEDULE).to(DEV).to(torch.bfloat16).eval()
wa = rajni_amd.RAJNIViTWrapper(ts.create_model(avg, seed=1), README_SCHEDULE).to(DEV).to(torch.bfloat16).eval()
x = torch.randn(B, 3, 224, 224, device=DEV, dtype=torch.bfloat16)
wm(x); n_last = wm.get_last_stats()["token_counts"][-1]
kv = torch.randn(B, n_last, 2 * cfg.embed_dim, device=DEV, dtype=torch.bfloat16)
q = torch.randn(cfg.num_heads, cfg.head_dim, device=DEV, dtype=torch.float32) * cfg.head_dim ** -0.5
variants = {
    "map forward": lambda: wm(x),
    "avg forward": lambda: wa(x),
    "map forward_features (trunk + final norm, no pool)": lambda: wm.forward_features(x),
    "avg forward_features (trunk + final norm, no pool)": lambda: wa.forward_features(x),
    "attention pool kernel alone": lambda: ops.attention_pool(kv, q),
}
for f in variants.values():          # warm every shape
    for _ in range(3):
        f()
torch.cuda.synchronize()
times = {k: [] for k in variants}
for r in range(ROUNDS):
    for k, f in variants.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ITERS):
            f()
        e1.record()
        torch.cuda.synchronize()
        times[k].append(e0.elapsed_time(e1) / ITERS)
print(f"vit_base_patch16_siglip_224 dims (C 768, 12 heads of 64, depth 12, MLP 3072), bf16, B = {B}, README schedule "
      f"{README_SCHEDULE}; token counts {wm.get_last_stats()['token_counts']}, {n_last} tokens reach the head")
print(f"{ROUNDS} rounds of {ITERS} calls per variant, variants interleaved; ms per call: median (min .. max)")
med = {}
for k, v in times.items():
    med[k] = statistics.median(v)
    print(f"  {k:52s} {med[k]:8.4f}  ({min(v):.4f} .. {max(v):.4f})")
tm = med["map forward"] - med["map forward_features (trunk + final norm, no pool)"]
ta = med["avg forward"] - med["avg forward_features (trunk + final norm, no pool)"]
print(f"  map: forward - forward_features = {tm:+.4f} ms  (kv GEMM + pool kernel + proj / LayerNorm / MLP on B rows + head GEMM)")
print(f"  avg: forward - forward_features = {ta:+.4f} ms  (the fused norm + mean kernel and the head GEMM, MINUS the all-rows final norm it replaces)")
print(f"  map forward / avg forward = {med['map forward'] / med['avg forward']:.4f}")
