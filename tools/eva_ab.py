"""What the norm inside the MLP costs: eva02_base_patch14_224's dims (bf16, batch 256, the README 4-stage schedule) with and
without mlp.norm, one process:
  A  the model as it is: every block issues rajni_hidden_norm between FC1 and FC2
  B  the same weights with every mlp.norm replaced by nn.Identity
alternated A B B A, each a median over sync -> forward -> sync.  Then the kernel alone on the hidden rows of the widest launch
(256 x 257 rows of 2048 bf16), device events, beside rajni_layernorm on the same row count at C = 768: bytes read plus bytes
written per second.  The yardstick is the LayerNorm kernel's rate in README.md, 5.5 TB/s.
Writes profiles/eva_ab.txt.
usage: python tools/eva_ab.py [batch=256] [model=eva02_base_patch14_224]"""
import copy, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rajni-vit_amd"))
import torch, torch.nn as nn, rajni_amd
from rajni_amd import ops, timm_shaped as ts

SCHED = {3: {"keep_ratio": 0.88, "update": True}, 4: {"keep_ratio": 0.88, "update": True},
         7: {"keep_ratio": 0.80, "update": True}, 8: {"keep_ratio": 0.72, "update": True}}
DEV = "cuda"
README_LN_TBS = 5.5
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def forward_ms(m, x, reps=7, inner=3):
    t = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(inner):
            m(x)
        torch.cuda.synchronize(); t.append((time.perf_counter() - t0) / inner * 1e3)
    return sorted(t)[len(t) // 2]


def event_us(fn, reps=5, inner=20):
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


def main(B, name):
    cfg = ts.config_of(name)
    base = ts.create_model(cfg, seed=0).to(torch.bfloat16).to(DEV).eval()
    bare = copy.deepcopy(base)
    for blk in bare.blocks:
        blk.mlp.norm = nn.Identity()
    x = torch.randn(B, 3, cfg.img_size, cfg.img_size, device=DEV).to(torch.bfloat16)
    models = {"A": rajni_amd.RAJNIViTWrapper(base, SCHED).eval(), "B": rajni_amd.RAJNIViTWrapper(bare, SCHED).eval()}
    for m in models.values():
        for _ in range(3):
            m(x)
    res = {"A": [], "B": []}
    for tag in "ABBA":
        res[tag].append(forward_ms(models[tag], x))
    counts = models["A"].get_last_stats()["token_counts"]
    a, b = sum(res["A"]) / 2, sum(res["B"]) / 2
    say(f"{name} dims (C {cfg.embed_dim}, hidden {cfg.hidden_dim}, depth {cfg.depth}), bf16, batch {B}, README 4-stage schedule, "
        f"token counts {sorted(set(counts), reverse=True)}; A B B A, medians of 7 x 3 forwards, sync -> forward -> sync")
    say(f"  A with mlp.norm     {res['A'][0]:.3f} / {res['A'][1]:.3f} ms   {B / a * 1e3:.0f} images/s")
    say(f"  B without           {res['B'][0]:.3f} / {res['B'][1]:.3f} ms   {B / b * 1e3:.0f} images/s")
    say(f"  the norm costs {100 * (a - b) / b:+.2f} % of the forward ({(a - b) * 1e3 / cfg.depth:.1f} us per block)")
    n, ld = cfg.hidden_dim, (cfg.hidden_dim + 63) // 64 * 64
    for tokens in sorted(set(counts), reverse=True)[:1] + sorted(set(counts))[:1]:
        rows = B * tokens
        h = torch.zeros((rows, ld), dtype=torch.bfloat16, device=DEV)
        h[:, :n] = torch.randn(rows, n, device=DEV)
        w, bias = torch.ones(n, device=DEV), torch.zeros(n, device=DEV)
        t = event_us(lambda: ops.hidden_norm(h, w, bias, 1e-6, n=n))
        xs = torch.randn(rows, cfg.embed_dim, device=DEV)
        lw, lb = torch.ones(cfg.embed_dim, device=DEV), torch.zeros(cfg.embed_dim, device=DEV)
        tl = event_us(lambda: ops.layernorm(xs, lw, lb, 1e-6))
        say(f"  rajni_hidden_norm, {rows} rows x {n} bf16 in place: {t:.1f} us, {2 * 2 * rows * n / t / 1e6:.2f} TB/s   |   "
            f"rajni_layernorm, {rows} rows x {cfg.embed_dim} fp32 -> bf16, same run: {tl:.1f} us, "
            f"{6 * rows * cfg.embed_dim / tl / 1e6:.2f} TB/s   (README's LayerNorm rate: {README_LN_TBS} TB/s)")
    with open(os.path.join(ROOT, "profiles", "eva_ab.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 256, sys.argv[2] if len(sys.argv) > 2 else "eva02_base_patch14_224")
