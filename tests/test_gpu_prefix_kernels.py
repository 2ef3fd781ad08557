"""The kernels that know about prefix tokens (CLS + register tokens), through the *_prefix entry points of the C ABI: selection
(select-only and fused), patch embed with prefix rows, and the 'avg' pool behind them.  GPU box only (`-m gpu`).

Selections are compared BIT-EXACTLY with the restated rule (tests/numerics_prefix.py::select_tokens): only scores[:, P:] are
ranked, larger first, then lower index, NaN = +inf, -0 = +0; slots 0..P-1 of keep_idx hold 0..P-1; next_scores is the gather.
Patch counts sit on the edges of the 8 / 4 / 2 / 1 lanes-per-token regimes of the rank loop at 1024 threads (128|129, 256|257,
512|513) and at the smallest legal sizes (1, 2, 3 patches), where the packed-key image is larger than the logits' region."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import numerics as nm
import numerics_prefix as npx
import numerics_variants as nv
from oracle import rajni_oracle as orc
from rajni_amd import ops, _native as nat

DEV = "cuda"
TORCH = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
PREFIXES = [1, 2, 4, 5]
PATCHES = [1, 2, 3, 16, 128, 129, 196, 256, 257, 512, 513, 576]


def keeps(n):
    return sorted({1, max(1, n // 2), n})


def stream():
    return nat.stream_ptr()


def host(t):
    return t.float().cpu().numpy()


def check_selection(idx, nxt, scores, keep, P, what):
    """idx / nxt device tensors against the rule on `scores` (a device tensor of the I/O dtype)"""
    s = host(scores)
    want = npx.select_tokens(s, keep, P)
    got = idx.cpu().numpy()
    np.testing.assert_array_equal(got, want, err_msg=what)
    assert np.array_equal(host(nxt), np.take_along_axis(s, want, axis=1), equal_nan=True), what


def tied_scores(B, N, dt, seed):
    """positive scores on a coarse grid (many exact ties), one row all equal, one row of signed values"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    s = (torch.rand((B, N), generator=g, device=DEV) * 64).floor() / 64
    s[1] = 0.25
    if B > 2:
        s[2] = torch.randn(N, generator=g, device=DEV)
    return s.to(TORCH[dt])


@pytest.mark.parametrize("P", PREFIXES)
@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_select_prefix_bit_exact(dt, P):
    for n in PATCHES:
        N = P + n
        s = tied_scores(3, N, dt, seed=N * 7 + P)
        for keep in keeps(n):
            idx, nxt = ops.select_topk(s, keep, num_prefix=P)
            assert tuple(idx.shape) == tuple(nxt.shape) == (3, P + keep)
            check_selection(idx, nxt, s, keep, P, f"select P={P} n={n} keep={keep} {dt}")


@pytest.mark.parametrize("two_pass", [0, 1], ids=["merged", "two_pass"])
@pytest.mark.parametrize("H,D", [(1, 8), (2, 8), (1, 64), (2, 64)])
@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_score_select_prefix_fused(dt, H, D, two_pass):
    """the fused kernel: scores do not depend on P (bit-equal to rajni_importance), the selection is the rule applied to them.
    N = P + 1, P + 2 with D = 8, H = 1 are the sizes at which the packed-key image decides the size of its LDS region."""
    B = 2
    nat.lib().rajni_debug_force_score_two_pass(two_pass)
    try:
        for P in PREFIXES:
            for n in PATCHES:
                N = P + n
                g = torch.Generator(device=DEV).manual_seed(N * 131 + H * 17 + D)
                qkv = torch.randn((B, N, 3 * H * D), generator=g, device=DEV).to(TORCH[dt])
                only = ops.importance(qkv, H)
                for keep in keeps(n):
                    what = f"score_select P={P} n={n} keep={keep} H={H} D={D} {dt} two_pass={two_pass}"
                    scores, idx, nxt = ops.score_select(qkv, H, keep, num_prefix=P)
                    assert torch.equal(scores.view(torch.uint8), only.view(torch.uint8)), what
                    check_selection(idx, nxt, scores, keep, P, what)
    finally:
        nat.lib().rajni_debug_force_score_two_pass(0)


@pytest.mark.parametrize("P", [2, 4, 5])
@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_special_values_at_the_prefix_patch_boundary(dt, P):
    """indices P-1 (the last register), P, P+1 (the first patches) and N-1: a register holding the largest score, +inf or NaN
    takes no rank slot and appears exactly once; equal scores across the boundary; zeros of both signs"""
    inf, nan = np.inf, np.nan
    for n in (2, 3, 16, 129, 257, 513):
        N = P + n
        base = np.random.default_rng(N).standard_normal((1, N)).astype(np.float32)
        rows = []
        for reg, first, second, last in ((9.0, 1.0, 2.0, 3.0), (inf, 1.0, inf, 0.5), (nan, nan, 1.0, nan), (nan, inf, inf, nan),
                                         (0.5, 0.5, 0.5, 0.5), (-0.0, 0.0, -0.0, 0.0), (0.0, -0.0, 0.0, -0.0), (-inf, -inf, 1.0, -inf),
                                         (7.0, 7.0, -7.0, 7.0)):
            r = base.copy()
            r[0, P - 1], r[0, P], r[0, P + 1], r[0, N - 1] = reg, first, second, last
            rows.append(r)
            z = np.where(np.arange(N) % 2 == 0, np.float32(0.0), np.float32(-0.0))[None].astype(np.float32)     # only zeros
            z[0, P - 1], z[0, P] = reg, first
            rows.append(z)
            e = np.full((1, N), np.float32(first))                                   # everything equals the first patch
            e[0, :P] = reg
            rows.append(e)
        s = torch.from_numpy(np.concatenate(rows)).to(DEV).to(TORCH[dt])
        for keep in keeps(n):
            idx, nxt = ops.select_topk(s, keep, num_prefix=P)
            what = f"special values P={P} n={n} keep={keep} {dt}"
            check_selection(idx, nxt, s, keep, P, what)
            got = idx.cpu().numpy()
            assert (got[:, :P] == np.arange(P)).all() and (got[:, P:] >= P).all(), what
            assert ((got == P - 1).sum(axis=1) == 1).all(), what
            assert (np.diff(got, axis=1) > 0).all(), what


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_num_prefix_1_is_the_old_entry_point_bit_for_bit(dt):
    """select, fused score/select, patch embed and pool: the *_prefix entry point with num_prefix = 1 against its namesake"""
    lib, T, code = nat.lib(), TORCH[dt], nat.dtype_code(TORCH[dt])
    same = lambda a, b: torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    for N in (2, 3, 17, 130, 197, 258, 577):
        s = tied_scores(3, N, dt, seed=N)
        for keep in keeps(N - 1):
            old = ops.select_topk(s, keep)
            idx = torch.full((3, keep + 1), -1, dtype=torch.int32, device=DEV)
            nxt = torch.empty((3, keep + 1), dtype=T, device=DEV)
            nat.check(lib.rajni_select_topk_prefix(s.data_ptr(), 3, N, 1, keep, idx.data_ptr(), nxt.data_ptr(), code, stream()), "select")
            assert torch.equal(idx, old[0]) and same(nxt, old[1]), (N, keep)
        H, D = (2, 64) if N > 3 else (1, 8)
        g = torch.Generator(device=DEV).manual_seed(N)
        qkv = torch.randn((2, N, 3 * H * D), generator=g, device=DEV).to(T)
        keep = max(1, (N - 1) // 2)
        old = ops.score_select(qkv, H, keep)
        sc = torch.empty((2, N), dtype=T, device=DEV)
        idx = torch.full((2, keep + 1), -1, dtype=torch.int32, device=DEV)
        nxt = torch.empty((2, keep + 1), dtype=T, device=DEV)
        nat.check(lib.rajni_score_select_prefix(qkv.data_ptr(), 2, N, H, D, 1e-6, 1, keep, sc.data_ptr(), idx.data_ptr(), nxt.data_ptr(),
                                                code, stream()), "score_select")
        assert same(sc, old[0]) and torch.equal(idx, old[1]) and same(nxt, old[2]), N
    # patch embed (fused loader and materialised columns; both streams), reg = NULL
    for S, Pz in ((64, 16), (56, 14)):
        for out_f32 in ((False, True) if dt != "fp32" else (False,)):
            img, w, b, cls, _, pos = embed_case(3, S, Pz, 128, 0, True, dt)
            old = ops.patch_embed(img, w, b, cls, pos, True, Pz, 128, out_f32=out_f32)
            x = torch.empty_like(old)
            nbytes = lib.rajni_patch_embed_workspace_bytes(3, 3, S, Pz, code)
            ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)
            nat.check(lib.rajni_patch_embed_prefix(img.data_ptr(), w.data_ptr(), b.data_ptr(), cls.data_ptr(), None, 1, pos.data_ptr(), 1,
                                                   x.data_ptr(), int(out_f32), 3, 3, S, Pz, 128, code, ws.data_ptr() if nbytes else None,
                                                   nbytes, stream()), "patch_embed")
            assert same(x, old), (S, Pz, out_f32)
    # pooled rows
    xs = torch.randn((3, 21, 128), generator=torch.Generator(device=DEV).manual_seed(5), device=DEV).to(T)
    nw, nb = torch.rand(128, device=DEV) + 0.5, torch.randn(128, device=DEV)
    for pool in ("avg", "token"):
        old = ops.pool_norm(xs, pool, (nw, nb, 1e-6), (nb.abs() + 0.5, nw, 1e-5), out_dtype=T)
        new = torch.empty_like(old)
        fw = nb.abs() + 0.5
        nat.check(lib.rajni_pool_norm_prefix(xs.data_ptr(), 3, 21, 1, 128, nat.POOL_AVG if pool == "avg" else nat.POOL_TOKEN, nw.data_ptr(),
                                             nb.data_ptr(), 1e-6, fw.data_ptr(), nw.data_ptr(), 1e-5, new.data_ptr(), code, 0, stream()), "pool")
        assert same(new, old), pool


# ---------------------------------------------------------------------------------------------------------------
# patch embed with prefix rows
# ---------------------------------------------------------------------------------------------------------------

def embed_case(B, S, Pz, Cc, R, pos_has_prefix, dt, seed=0):
    """device tensors (images, packed weight, fp32 bias, cls [C], reg [R, C] or None, pos) of dtype dt"""
    g = torch.Generator(device=DEV).manual_seed(seed + S + Cc + R)
    T = TORCH[dt]
    rn = lambda *shape, s=1.0: (torch.randn(shape, generator=g, device=DEV) * s).to(T)
    img, w = rn(B, 3, S, S), rn(Cc, 3, Pz, Pz, s=0.05)
    b = rn(Cc, s=0.1).float()
    cls = rn(Cc)
    reg = rn(R, Cc) if R else None
    n = (S // Pz) ** 2
    pos = rn(n + (1 + R if pos_has_prefix else 0), Cc)
    wp = ops.pack_weight(w, T, k_multiple=64)
    wp.w_plain = w
    return img, wp, b, cls, reg, pos


@pytest.mark.parametrize("pos_has_prefix", [True, False], ids=["pos_with_prefix_rows", "no_embed_class"])
@pytest.mark.parametrize("S,Pz", [(64, 16), (56, 14)], ids=["patch16_fused", "patch14_columns"])
@pytest.mark.parametrize("fmt", ["bf16", "bf16_to_f32", "fp16", "fp16_to_f32", "fp32"])
def test_patch_embed_with_prefix_rows(fmt, S, Pz, pos_has_prefix):
    """against a torch fp64 restatement at tests/test_gpu_kernels.py::test_patch_embed's tolerances (1e-2 of the scale into a
    16-bit stream, 1e-5 into fp32); the prefix rows are a copy or ONE fp32 add, rounded once into a 16-bit stream: exact"""
    dt = fmt.split("_")[0]
    out_f32 = fmt.endswith("_to_f32")
    Cc = 128
    for R in (1, 4):
        for B in (1, 3):
            img, wp, b, cls, reg, pos = embed_case(B, S, Pz, Cc, R, pos_has_prefix, dt)
            P, n = 1 + R, (S // Pz) ** 2
            x = ops.patch_embed(img, wp, b, cls, pos, pos_has_prefix, Pz, Cc, out_f32=out_f32, reg=reg)
            what = f"patch embed {fmt} S={S} patch={Pz} R={R} B={B} pos_has_prefix={pos_has_prefix}"
            assert tuple(x.shape) == (B, P + n, Cc) and x.dtype == (torch.float32 if out_f32 or dt == "fp32" else TORCH[dt]), what
            tok = torch.nn.functional.conv2d(img.double(), wp.w_plain.double(), b.double(), stride=Pz).flatten(2).transpose(1, 2)
            off = P if pos_has_prefix else 0
            want = tok + pos.double()[off:][None]
            got = x[:, P:].double()
            scale = float(want.abs().max())
            err = float((got - want).abs().max())
            assert err <= (1e-5 if x.dtype == torch.float32 else 1e-2) * scale, f"{what}: patch rows off by {err:.4g} (scale {scale:.4g})"
            pre = torch.cat([cls[None], reg]).float()
            if pos_has_prefix:
                pre = pre + pos[:P].float()                                   # one fp32 add
            pre = pre.to(x.dtype)                                             # one rounding into a 16-bit stream
            for bi in range(B):
                assert torch.equal(x[bi, :P].view(torch.uint8), pre.view(torch.uint8)), f"{what}: prefix rows of image {bi}"


# ---------------------------------------------------------------------------------------------------------------
# 'avg' pool behind the prefix rows
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stream_dt,out_dt", [("fp32", "fp32"), ("fp32", "bf16"), ("fp32", "fp16"), ("bf16", "bf16"), ("fp16", "fp16")])
@pytest.mark.parametrize("P", [2, 5])
def test_pool_norm_averages_rows_behind_the_prefix(P, stream_dt, out_dt):
    """mean over rows P..N-1 in the kernel's fixed order, against fp64 within tests/numerics_variants.py::pool_norm_budget (the
    budget of tests/test_gpu_variants_kernels.py::test_pool_norm_stress_tokens, evaluated on the rows that are pooled)"""
    B, C = 3, 192
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(nm.TORCH[dt]).to(DEV)
    for N in (P + 1, P + 2, 21, 201):
        x, (nw, nb), (fw, fb) = nv.pool_case(B, N, C, stream_dt, seed=P)
        xd = dev(x, stream_dt)
        for pool, use_norm, use_fc in (("avg", False, True), ("avg", True, True), ("avg", True, False), ("avg", False, False),
                                       ("token", True, True)):
            norm = (nw, nb, 1e-6) if use_norm else None
            fc = (fw, fb, 1e-5) if use_fc else None
            # the budget's 'avg' drops ONE leading row: hand it the rows from P - 1 on ('token' reads row 0)
            want, bud = nv.pool_norm_budget(x[:, P - 1:] if pool == "avg" else x, pool, norm, fc, out_dt)
            dn = (dev(nw, "fp32"), dev(nb, "fp32"), 1e-6) if use_norm else None
            df = (dev(fw, "fp32"), dev(fb, "fp32"), 1e-5) if use_fc else None
            y = ops.pool_norm(xd, pool, dn, df, out_dtype=nm.TORCH[out_dt], num_prefix=P)
            what = f"pool_norm P={P} N={N} {stream_dt}->{out_dt} {pool} norm={use_norm} fc_norm={use_fc}"
            nm.assert_within(host(y), want, bud, what)
            one = ops.pool_norm(xd[1:2].clone(), pool, dn, df, out_dtype=nm.TORCH[out_dt], num_prefix=P)
            assert torch.equal(one.view(torch.uint8), y[1:2].view(torch.uint8)), what
            if pool == "avg":      # the same bits as the old entry point on the tensor without its first P - 1 rows
                old = ops.pool_norm(xd[:, P - 1:].contiguous(), pool, dn, df, out_dtype=nm.TORCH[out_dt])
                assert torch.equal(old.view(torch.uint8), y.view(torch.uint8)), what
    with pytest.raises(nat.NativeError, match="patch token"):
        ops.pool_norm(torch.zeros((1, P, C), device=DEV), "avg", num_prefix=P, out_dtype=torch.float32)
