#!/usr/bin/env python
"""What the mean importance query and a model without a class token cost on the device (include/rajni_hip_query.h).

  (a) the score + select launch at ViT-B's shapes (B 256, N 197 and 173, H 12, D 64, bf16, keep = 88 % of the patch tokens):
      RAJNI_QUERY_CLS against RAJNI_QUERY_MEAN on the same qkv, through rajni_score_select_query, as one workgroup per image
      and with the tiled path forced.  The mean query re-reads the Q third: 3/3 of qkv instead of 2/3.
  (b) the whole forward (evaluate_model's sync -> forward -> sync) of the vit_medium_patch16_gap_256 dimensions (no class token,
      mean query) against its class-token twin with the class query and with the mean query, README schedule, batch 256, bf16.

Modes alternate A B B A inside one process (so a drifting clock falls on both alike); every figure is the MEDIAN over the
rounds of a device-event time around CALLS back-to-back enqueues after WARM warm-up calls.  Neither measurement has a pass mark.

    python tools/noclass_cost.py [--out profiles/noclass_ab.txt] [--rounds 6]
"""
import argparse
import dataclasses
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rajni-vit_amd"))

import rajni_amd  # noqa: E402
from rajni_amd import _native as nat  # noqa: E402
from rajni_amd import timm_shaped as ts  # noqa: E402
from rajni_amd.run import README_SCHEDULE  # noqa: E402

WARM, CALLS = 10, 50


def abba(modes, rounds, fn):
    """{mode: median of fn(mode)} over `rounds` rounds, the modes in order A B .. and back .. B A within a round"""
    times = {m: [] for m in modes}
    for _ in range(rounds):
        for m in list(modes) + list(reversed(modes)):
            times[m].append(fn(m))
    return {m: statistics.median(v) for m, v in times.items()}, {m: (min(v), max(v)) for m, v in times.items()}


def timed(call, calls=CALLS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / calls      # us per call


def score_launch(B, N, H, D, tiled, rounds, say):
    lib = nat.lib()
    g = torch.Generator(device="cuda").manual_seed(N * H + D)
    qkv = torch.randn((B, N, 3 * H * D), generator=g, device="cuda").to(torch.bfloat16)
    keep = max(1, int(0.88 * (N - 1)))
    scores = torch.empty((B, N), dtype=torch.bfloat16, device="cuda")
    idx = torch.empty((B, keep + 1), dtype=torch.int32, device="cuda")
    nxt = torch.empty((B, keep + 1), dtype=torch.bfloat16, device="cuda")
    lib.rajni_debug_force_score_tiled(int(tiled))
    try:
        nbytes = {q: lib.rajni_score_select_query_workspace_bytes(B, N, H, D, nat.RAJNI_BF16, q) for q in (nat.QUERY_CLS, nat.QUERY_MEAN)}
        ws = torch.empty(max(nbytes.values()), dtype=torch.uint8, device="cuda") if tiled else None

        def call(q):
            nat.check(lib.rajni_score_select_query(qkv.data_ptr(), B, N, H, D, 1e-6, 1, keep, q, scores.data_ptr(), idx.data_ptr(),
                                                   nxt.data_ptr(), nat.RAJNI_BF16, nat.ptr(ws), nbytes[q], nat.stream_ptr()),
                      "rajni_score_select_query")
        for q in nbytes:
            for _ in range(WARM):
                call(q)
        torch.cuda.synchronize()
        med, span = abba([nat.QUERY_CLS, nat.QUERY_MEAN], rounds, lambda q: timed(lambda: call(q)))
    finally:
        lib.rajni_debug_force_score_tiled(0)
    c, m = med[nat.QUERY_CLS], med[nat.QUERY_MEAN]
    say(f"score launch B={B} N={N} H={H} D={D} bf16 {'tiled (forced)' if tiled else 'one workgroup'}: cls {c:8.2f} us "
        f"[{span[nat.QUERY_CLS][0]:.2f}, {span[nat.QUERY_CLS][1]:.2f}]   mean {m:8.2f} us [{span[nat.QUERY_MEAN][0]:.2f}, "
        f"{span[nat.QUERY_MEAN][1]:.2f}]   mean / cls {m / c:.3f}")


def whole_forward(batch, rounds, say):
    cfg = ts.config_of("vit_medium_patch16_gap_256")
    twin = dataclasses.replace(cfg, class_token=True)
    sched = {k: v for k, v in README_SCHEDULE.items() if k < cfg.depth}
    x = torch.randn((batch, 3, cfg.img_size, cfg.img_size), generator=torch.Generator(device="cuda").manual_seed(0), device="cuda").to(torch.bfloat16)
    models = {}
    for label, c, query in (("no class token, mean query", cfg, "mean"), ("class-token twin, class query", twin, "cls"),
                            ("class-token twin, mean query", twin, "mean")):
        w = rajni_amd.RAJNIViTWrapper(ts.create_model(c, seed=0).to(torch.bfloat16), sched).to("cuda").eval()
        models[label] = w.set_importance_query(query)
        for _ in range(3):
            w(x)
    torch.cuda.synchronize()

    def one(label):        # sync -> forward -> sync, as evaluate_model times it: ms per forward
        return timed(lambda: models[label](x), calls=10) / 1000.0
    med, span = abba(list(models), rounds, one)
    base = med["class-token twin, class query"]
    for label in models:
        say(f"forward {cfg.embed_dim} wide x {cfg.depth} blocks at {cfg.img_size} px, batch {batch}, bf16, {label:30s}: {med[label]:7.3f} ms "
            f"[{span[label][0]:.3f}, {span[label][1]:.3f}]  {batch / med[label] * 1000:9.0f} img/s  x{med[label] / base:.4f} "
            f"(token counts {models[label].get_last_stats()['token_counts']})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--batch", type=int, default=256)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    nat.check(nat.lib().rajni_device_check(), "device check")
    say(f"# tools/noclass_cost.py: medians over {args.rounds} A B B A rounds of {CALLS} calls (whole forward: 10), [min, max] beside")
    for N in (197, 173):
        for tiled in (False, True):
            score_launch(256, N, 12, 64, tiled, args.rounds, say)
    whole_forward(args.batch, args.rounds, say)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
