#!/usr/bin/env python
"""What rotary position embeddings cost on the device (include/rajni_hip_rope.h): ViT-B/16 dimensions, bf16, batch 256, the README
schedule.

1. The kernel alone, at every block's token count: microseconds per rajni_rope_qk launch (device events around 50 back-to-back
   launches after 5 warm-up launches, the median of 5 such windows), the bytes it moves - it reads and writes the q and k thirds
   of the patch rows, 4 * B * (N - P) * C * 2 bytes, and reads one table row per token - and the rate, with and without a
   source map, and with one table per head (the mixed form: 2H table rows per token, each loaded behind the head in front).
   Beside it the LayerNorm kernel of the same run on the same rows (fp32 stream in, bf16 out, 6 bytes per element):
   the project's reference point for a row kernel bound by memory.
2. The whole forward with and without `rope` for the same trunk (vit_base_patch16_rope_224 and the same config with
   rope="none"): host clock around sync -> call -> sync, the median of 60 calls per mode, modes alternated A B B A.
Neither measurement has a pass mark.

    python tools/rope_cost.py [--out FILE (appended to)] [--batch 256] [--calls 60]
"""
import argparse
import dataclasses
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rajni-vit_amd"))

import rajni_amd  # noqa: E402
from rajni_amd import _native as nat  # noqa: E402
from rajni_amd import timm_shaped as ts  # noqa: E402

SCHED = {3: {"keep_ratio": 0.88, "update": True}, 4: {"keep_ratio": 0.88, "update": True},
         7: {"keep_ratio": 0.80, "update": True}, 8: {"keep_ratio": 0.72, "update": True}}


def window_us(call, launches=50, warm=5, windows=5):
    for _ in range(warm):
        call()
    out = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            call()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / launches * 1e3)
    return statistics.median(out), min(out), max(out)


def kernel_lines(B, counts, P, H, D, half):
    C = H * D
    lib, s = nat.lib(), nat.stream_ptr(torch.device("cuda"))
    g = torch.Generator(device="cuda").manual_seed(0)
    n0 = counts[0]
    cos = torch.rand((n0 - P, D), generator=g, device="cuda") * 2 - 1
    sin = torch.rand((n0 - P, D), generator=g, device="cuda") * 2 - 1
    cosh = torch.rand((H, n0 - P, D), generator=g, device="cuda") * 2 - 1
    sinh = torch.rand((H, n0 - P, D), generator=g, device="cuda") * 2 - 1
    w, b = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    lines = [f"{'tokens':>6s} {'rope us':>9s} {'[min, max]':>16s} {'MB':>7s} {'TB/s':>6s} | {'mapped us':>9s} {'TB/s':>6s} | {'per-head us':>11s} {'TB/s':>6s} | "
             f"{'LayerNorm us':>12s} {'MB':>7s} {'TB/s':>6s} | rope / LN rate"]
    for N in sorted(set(counts), reverse=True):
        qkv = torch.randn((B, N, 3 * C), generator=g, device="cuda").to(torch.bfloat16)
        # a sub-selection of the grid in ascending order per image, as the forward's map is
        src = torch.cat([torch.arange(P, device="cuda").expand(B, P),
                         P + torch.rand((B, n0 - P), generator=g, device="cuda").argsort(1)[:, :N - P].sort(1).values], 1).to(torch.int32).contiguous()
        x = torch.randn((B * N, C), generator=g, device="cuda")
        y = torch.empty((B * N, C), dtype=torch.bfloat16, device="cuda")
        rope = lambda m: nat.check(lib.rajni_rope_qk(qkv.data_ptr(), m, cos.data_ptr(), sin.data_ptr(), 0, B, N, P, H, D, int(half),
                                                     nat.RAJNI_BF16, s), "rajni_rope_qk")
        roph = lambda: nat.check(lib.rajni_rope_qk(qkv.data_ptr(), None, cosh.data_ptr(), sinh.data_ptr(), (n0 - P) * D, B, N, P, H, D,
                                                   int(half), nat.RAJNI_BF16, s), "rajni_rope_qk")
        ln = lambda: nat.check(lib.rajni_layernorm(x.data_ptr(), C, w.data_ptr(), b.data_ptr(), y.data_ptr(), B * N, C, 1e-6,
                                                   nat.RAJNI_BF16, 1, s), "rajni_layernorm")
        r, rlo, rhi = window_us(lambda: rope(None))
        m, _, _ = window_us(lambda: rope(src.data_ptr()))
        ph, _, _ = window_us(roph)
        l, _, _ = window_us(ln)
        rb = 4.0 * B * (N - P) * C * 2 + 8.0 * B * (N - P) * D
        lb = 6.0 * B * N * C
        pb = 4.0 * B * (N - P) * C * 2 + 8.0 * B * (N - P) * C      # a table row pair per (token, head), read for q and for k from cache
        lines.append(f"{N:6d} {r:9.1f} {f'[{rlo:.1f}, {rhi:.1f}]':>16s} {rb / 1e6:7.1f} {rb / r / 1e6:6.2f} | {m:9.1f} {(rb + 4.0 * B * N) / m / 1e6:6.2f} | {ph:11.1f} {pb / ph / 1e6:6.2f} | "
                     f"{l:12.1f} {lb / 1e6:7.1f} {lb / l / 1e6:6.2f} | {(rb / r) / (lb / l):.2f}")
        torch.cuda.synchronize()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--calls", type=int, default=60)
    args = ap.parse_args()
    nat.check(nat.lib().rajni_device_check(), "device check")
    B = args.batch
    cfg = ts.config_of("vit_base_patch16_rope_224")
    x = torch.randn((B, 3, cfg.img_size, cfg.img_size), generator=torch.Generator(device="cuda").manual_seed(1), device="cuda").to(torch.bfloat16)
    models = {}
    for label, c in (("rope", cfg), ("none", dataclasses.replace(cfg, rope="none"))):
        w = rajni_amd.RAJNIViTWrapper(ts.create_model(c, seed=0).to(torch.bfloat16), SCHED).to("cuda").eval()
        models[label] = w
        for _ in range(5):
            w(x)
    torch.cuda.synchronize()
    counts = models["rope"].get_last_stats()["token_counts"]
    assert counts == models["none"].get_last_stats()["token_counts"]
    lines = [f"# tools/rope_cost.py: ViT-B/16 dimensions (12 heads of 64), bf16, batch {B}, README schedule; token counts {counts}",
             "# 1. rajni_rope_qk alone (axial table shared by all heads, interleaved pairs) against rajni_layernorm on the same rows: "
             "medians of 5 windows of 50 launches"]
    lines += kernel_lines(B, counts, cfg.num_prefix_tokens, cfg.num_heads, cfg.head_dim, cfg.rope_half)
    ms = {m: [] for m in models}
    per = max(1, args.calls // 4)      # every mode runs in four segments: A B | B A | B A | A B
    for order in (("rope", "none"), ("none", "rope"), ("none", "rope"), ("rope", "none")):
        for m in order:
            for _ in range(per):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                models[m](x)
                torch.cuda.synchronize()
                ms[m].append((time.perf_counter() - t0) * 1e3)
    lines.append(f"# 2. the whole forward, host clock around sync -> call -> sync, medians of {len(ms['rope'])} calls per mode, A B B A")
    for m, v in ms.items():
        med = statistics.median(v)
        lines.append(f"forward rope={m:5s}: {med:8.3f} ms [{min(v):.3f}, {max(v):.3f}]  {B / med * 1000:8.0f} img/s")
    r, n = statistics.median(ms["rope"]), statistics.median(ms["none"])
    lines.append(f"rope - none = {(r - n) * 1e3:+.1f} us = {(r - n) / cfg.depth * 1e3:.1f} us per block; rope / none = {r / n:.4f}")
    print("\n".join(lines), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
