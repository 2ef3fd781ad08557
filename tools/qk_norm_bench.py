"""q/k-norm (csrc/variants.hip) alone on the ViT-B forward's stage shapes (B = 256; 197 / 152 / 87 tokens; H = 12, D = 64; bf16):
microseconds and algorithmic TB/s (the q and k thirds, read + written), next to rajni_layernorm on the same number of rows in the
same process; then the price of the feature in the whole forward: the q/k-norm ViT-B against the same weights with q_norm /
k_norm replaced by Identity, through evaluate_model, A B B A.  GPU box only: python tools/qk_norm_bench.py [batch]"""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rajni-vit_amd"))
import torch
import torch.nn as nn
import rajni_amd
from rajni_amd import ops, timm_shaped as ts

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
H, D, C = 12, 64, 768


def timed(fn, reps=30):
    for _ in range(3): fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


w = [torch.ones(D, device="cuda"), torch.zeros(D, device="cuda"), torch.ones(D, device="cuda"), torch.zeros(D, device="cuda")]
for tokens in (197, 152, 87):
    rows = B * tokens
    qkv = torch.randn(rows, 3 * C, device="cuda").to(torch.bfloat16)
    us = timed(lambda: ops.qk_norm(qkv, H, w[0], w[1], w[2], w[3], 1e-6))
    x = torch.randn(rows, C, device="cuda"); lw = torch.ones(C, device="cuda"); lb = torch.zeros(C, device="cuda")
    ln = timed(lambda: ops.layernorm(x, lw, lb, 1e-6))
    print(f"rows {rows} ({tokens} tokens): qk_norm {us:.1f} us  {rows * 2 * C * 4 / us / 1e6:.2f} TB/s (q, k read + written)   |   "
          f"layernorm fp32 -> bf16 {ln:.1f} us  {rows * C * 6 / ln / 1e6:.2f} TB/s", flush=True)

sched = {3: {"keep_ratio": 0.88, "update": True}, 4: {"keep_ratio": 0.88, "update": True}, 7: {"keep_ratio": 0.80, "update": True},
         8: {"keep_ratio": 0.72, "update": True}}
cfg = ts.CONFIGS["vit_base_patch16_qknorm_224"]
g = torch.Generator().manual_seed(0)
loader = [(torch.randn(B, 3, 224, 224, generator=g), torch.randint(0, 1000, (B,), generator=g)) for _ in range(2)]


def model(with_norm):
    m = ts.create_model(cfg, seed=0)
    if not with_norm:
        for blk in m.blocks:
            blk.attn.q_norm, blk.attn.k_norm = nn.Identity(), nn.Identity()
    return rajni_amd.RAJNIViTWrapper(m.to(torch.bfloat16), sched).eval()


models = {True: model(True), False: model(False)}
rates = {True: [], False: []}
for with_norm in (True, False, False, True):
    _, thr = rajni_amd.evaluate_model(models[with_norm], loader * 10, device="cuda", max_batches=20, warmup=5)
    rates[with_norm].append(thr)
for k, name in ((True, "q/k-norm"), (False, "Identity")):
    print(f"ViT-B/16 B={B} README schedule, {name}: {rates[k][0]:.0f} / {rates[k][1]:.0f} img/s  ({B / (sum(rates[k]) / 2) * 1e3:.3f} ms per forward)")
a, b = sum(rates[True]) / 2, sum(rates[False]) / 2
print(f"price of q/k-norm as one in-place pass per block: {(B / a - B / b) * 1e6:.0f} us per forward, {100 * (b / a - 1):.2f} % of the forward")
