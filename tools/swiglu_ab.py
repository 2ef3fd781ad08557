"""The gated FC1 (RAJNI_EPI_BIAS_SWIGLU) against what the library could do without it, one process, on the FC1 shapes of the DINOv2
giant ViTs (C 1536, hidden 4096, 1374 tokens at 518 px with 4 registers):
  A  fused:    one rajni_linear launch, [M, 1536] x [8192, 1536]^T -> silu(gate) * value, [M, 4096]
  B  unfused:  rajni_linear with RAJNI_EPI_BIAS into [M, 8192], then F.silu(a) * b in torch
alternated A B B A ..., device-event times, and the outputs compared (one rounding apart: B rounds gate and value to bf16
first).  Beside them G, the GELU FC1 of the same [8192, 1536] W (output [M, 8192]), for the achieved TFLOP/s - all three
multiply by the same W, 2 * M * 8192 * 1536 flop.  Rows: every token count of a three-stage schedule, times the batch.
`forward`: the whole forward of vit_giant_patch14_reg4_dinov2's dims against the stock PyTorch forward of the same module.
usage: python tools/swiglu_ab.py [batch=8] [forward [batch=4] [depth=40]]"""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rajni-vit_amd"))
import dataclasses
import torch, rajni_amd
import torch.nn.functional as F
from rajni_amd import ops, _native as nat, timm_shaped as ts
from rajni_amd.wrapper.model import plan_token_counts

SCHED = {10: {"keep_ratio": 0.88, "update": True}, 20: {"keep_ratio": 0.80, "update": True}, 30: {"keep_ratio": 0.72, "update": True}}
C_, HID, P = 1536, 4096, 5
DEV = "cuda"


def timed(fn, reps=5, inner=20):
    """median over `reps` of the device-event time of `inner` calls, us per call"""
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        t.append(a.elapsed_time(b) / inner * 1e3)
    return sorted(t)[len(t) // 2]


def fc1_ab(B):
    counts = sorted(set(plan_token_counts(1369 + P, 40, SCHED, P)), reverse=True)
    print(f"giant FC1 shapes: C {C_}, hidden {HID}, batch {B}, token counts {counts}; bf16; median of 5 x 20 launches per line, "
          f"5 warm-up launches, device events")
    torch.manual_seed(0)
    w = ops.pack_weight((torch.randn(2 * HID, C_, device=DEV) * 0.03), torch.bfloat16)
    b = torch.randn(2 * HID, device=DEV) * 0.1
    for n in counts:
        M = n * B
        x = torch.randn(M, C_, device=DEV).to(torch.bfloat16)
        yA = torch.empty((M, HID), dtype=torch.bfloat16, device=DEV)
        yB = torch.empty((M, 2 * HID), dtype=torch.bfloat16, device=DEV)
        fused = lambda: ops.linear(x, w, HID, b, nat.EPI_BIAS_SWIGLU, out=yA)
        def unfused():
            ops.linear(x, w, 2 * HID, b, nat.EPI_BIAS, out=yB)
            return F.silu(yB[:, :HID]) * yB[:, HID:]
        gelu = lambda: ops.linear(x, w, 2 * HID, b, nat.EPI_BIAS_GELU, out=yB)
        for f in (fused, unfused, gelu):
            for _ in range(5):
                f()
        res = {"A": [], "B": [], "G": []}
        for tag in "ABBAGABBAG":
            res[tag].append(timed({"A": fused, "B": unfused, "G": gelu}[tag]))
        ref = unfused().float()
        err = float((fused().float() - ref).abs().max() / ref.abs().max())
        mean = lambda v: sum(v) / len(v)
        a, bb, g = mean(res["A"]), mean(res["B"]), mean(res["G"])
        flop = 2.0 * M * 2 * HID * C_
        print(f"M {M:6d} ({n} tokens): fused {a:8.1f} us (spread {max(res['A']) - min(res['A']):.1f}, {flop / a / 1e6:.0f} TFLOP/s)  "
              f"unfused {bb:8.1f} us (spread {max(res['B']) - min(res['B']):.1f})  fused {100 * (a - bb) / bb:+.1f} %  |  "
              f"GELU FC1 [M, 8192] {g:8.1f} us ({flop / g / 1e6:.0f} TFLOP/s)  |  max |fused - unfused| / max |.| {err:.2e}")


def forward_ab(B, depth):
    cfg = dataclasses.replace(ts.config_of("vit_giant_patch14_reg4_dinov2"), depth=depth)
    sched = {k: v for k, v in SCHED.items() if k < depth}
    base = ts.create_model(cfg, seed=0).to(torch.bfloat16).to(DEV).eval()
    x = torch.randn(B, 3, cfg.img_size, cfg.img_size, device=DEV).to(torch.bfloat16)

    def stock():
        with torch.no_grad():
            return base(x)
    t_stock = []
    for _ in range(3):
        stock()
    for _ in range(3):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(3):
            stock()
        torch.cuda.synchronize(); t_stock.append((time.perf_counter() - t0) / 3 * 1e3)
    want = stock().float()
    for name, sc in (("unpruned", {}), ("three-stage schedule", sched)):
        m = rajni_amd.RAJNIViTWrapper(base, sc).eval()
        for _ in range(3):
            m(x)
        t = []
        for _ in range(3):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(3):
                m(x)
            torch.cuda.synchronize(); t.append((time.perf_counter() - t0) / 3 * 1e3)
        got = m(x).float()
        extra = f"max |dlogit| vs stock {float((got - want).abs().max()):.4g} (scale {float(want.abs().max()):.4g})" if not sc else \
            f"token counts {sorted(set(m.get_last_stats()['token_counts']), reverse=True)}"
        print(f"giant reg4 dims, depth {depth}, 518 px, bf16, B={B}, {name}: native {sorted(t)[1]:.2f} ms  "
              f"stock PyTorch (unpruned) {sorted(t_stock)[1]:.2f} ms;  {extra}")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "forward":
        forward_ab(int(sys.argv[2]) if len(sys.argv) > 2 else 4, int(sys.argv[3]) if len(sys.argv) > 3 else 40)
    else:
        fc1_ab(int(sys.argv[1]) if len(sys.argv) > 1 else 8)
