#!/usr/bin/env python3
"""bf16 model against fp16 model, one process: the same ViT-B/16 weights (README schedule) wrapped twice - once .to(bfloat16),
once .to(float16) - timed A/B/A/B with the sync -> forward -> sync metric, then the per-class breakdown (HIP events,
rajni_profile_*) of each and the fp16 / bf16 ratio per class.  Last, the numerics of both on the 256-image agreement
fixture (tests/golden/base224_agree256, the reference's own selections injected): max |dlogit| against the reference fp32
run, relative to its logit scale, and top-1 agreement.
    python tools/ab_dtype.py [batch] [rounds]        -> one summary line per dtype, the class table, and a JSON line"""
import copy, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rajni-vit_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import rajni_amd
from rajni_amd import timm_shaped as ts, _native as nat

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 6
ITERS = 10
SCHED = {3: {"keep_ratio": 0.88, "update": True}, 4: {"keep_ratio": 0.88, "update": True},
         7: {"keep_ratio": 0.80, "update": True}, 8: {"keep_ratio": 0.72, "update": True}}
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}

cfg = ts.CONFIGS["vit_base_patch16_224"]
base = ts.create_model(cfg, seed=0)
models = {k: rajni_amd.RAJNIViTWrapper(copy.deepcopy(base).to(dt).cuda(), SCHED).eval() for k, dt in DTYPES.items()}
x32 = torch.randn(B, 3, cfg.img_size, cfg.img_size, device="cuda")
xs = {k: x32.to(dt) for k, dt in DTYPES.items()}
for k in DTYPES:
    for _ in range(5):
        models[k](xs[k])

times = {k: [] for k in DTYPES}
for r in range(ROUNDS):                      # A/B/A/B: clock and thermal drift hit both alike
    order = list(DTYPES) if r % 2 == 0 else list(DTYPES)[::-1]
    for k in order:
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(ITERS):
            models[k](xs[k])
        torch.cuda.synchronize(); times[k].append((time.perf_counter() - t0) / ITERS * 1e3)

classes = {}
for k in DTYPES:
    nat.profile_reset(); nat.profile_enable((1 << 17) - 1)
    for _ in range(5):
        models[k](xs[k])
    torch.cuda.synchronize(); nat.profile_enable(0)
    classes[k] = {c: v["ms"] / 5 * 1e3 for c, v in nat.profile_collect().items() if v["launches"]}

res = {"batch": B, "rounds": ROUNDS, "iters": ITERS}
for k in DTYPES:
    t = sorted(times[k])
    res[k] = {"ms_min": round(t[0], 4), "ms_median": round(t[len(t) // 2], 4), "img_per_s": round(B / t[0] * 1e3, 1)}
    print(f"{k}: min {t[0]:.3f} ms  median {t[len(t) // 2]:.3f} ms per forward  ({B / t[0] * 1e3:.0f} img/s)")
res["fp16_over_bf16_min"] = round(res["fp16"]["ms_min"] / res["bf16"]["ms_min"], 4)
res["fp16_over_bf16_median"] = round(res["fp16"]["ms_median"] / res["bf16"]["ms_median"], 4)
print(f"fp16 / bf16: {res['fp16_over_bf16_min']:.4f} (min)  {res['fp16_over_bf16_median']:.4f} (median)")
print(f"{'class':36s} {'bf16 us':>9s} {'fp16 us':>9s} {'ratio':>7s}")
res["classes_us"] = {}
for c in sorted(set(classes["bf16"]) | set(classes["fp16"]), key=lambda c: -classes["bf16"].get(c, 0.0)):
    a, b = classes["bf16"].get(c, 0.0), classes["fp16"].get(c, 0.0)
    print(f"{c:36s} {a:9.1f} {b:9.1f} {b / a if a else float('nan'):7.3f}")
    res["classes_us"][c] = {"bf16": round(a, 2), "fp16": round(b, 2)}

# numerics on the agreement fixture (the reference's own selections injected)
from helpers import load_case, case_images, pruned_blocks  # noqa: E402
meta, data = load_case("base224_agree256")
imgs = torch.from_numpy(case_images(meta, data)).cuda()
ref = data["logits"].astype(np.float64)
scale = float(np.abs(ref).max())
res["numerics_agree256"] = {"logit_scale": round(scale, 4)}
for k, dt in DTYPES.items():
    mcfg = ts.CONFIGS[meta["cfg_name"]]
    model = ts.create_model(mcfg, seed=meta["seed"], std=meta["std"], bias_std=meta["bias_std"], round_bf16=True)
    w = rajni_amd.RAJNIViTWrapper(model, meta["schedule"]).cuda().to(dt).eval()
    w.force_keep_idx({i: torch.from_numpy(data[f"blk{i}.keep_idx"]).cuda() for i in pruned_blocks(meta)})
    lg = w(imgs).double().cpu().numpy()
    err = float(np.abs(lg - ref).max())
    agree = int((lg.argmax(1) == ref.argmax(1)).sum())
    res["numerics_agree256"][k] = {"max_abs_dlogit": round(err, 5), "rel": round(err / scale, 5), "top1_agree": agree}
    print(f"{k}: max |dlogit| {err:.4g} = {err / scale:.3g} of the logit scale; top-1 agreement {agree}/{len(ref)}")
print(json.dumps(res))
