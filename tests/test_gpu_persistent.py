"""The persistent kernels with several tiles or items per workgroup.  GPU box only (`-m gpu`).

gemm_bf16_tn_stream (256x256 and 256x128; bf16, fp16, fp8 weights), gemm_f8_tn_stream, gemm_f8_tn_wide and
attn_bf16_d64_stream walk their tiles / items in a hand-pipelined loop: the DMA is retargeted to the next tile NS steps
early, the previous tile's stores are still in flight at the next tile's first counted wait, K/V of item i+1 and the
keep_idx entries of item i+2 are in flight while item i is computed.  At the shapes of the other kernel tests every
workgroup runs ONE tile or item.  Here rajni_debug_set_persistent_workgroups(n) caps the grid and nothing else, so the few
tiles of a small shape go through one, two, three ... workgroups; every case asserts

  (a) for each cap the output equals the uncapped launch's BIT FOR BIT (same tiles, same K order, same epilogue; at these
      shapes the uncapped launch runs one tile or item per workgroup - the regime tests/test_gpu_numerics.py holds to fp64),
      both into fresh NaN-filled buffers with no NaN left;
  (b) the capped output itself stays inside the per-element budget of tests/numerics.py (fp8 x fp8 and e4m3 outputs: the
      rule of tests/numerics_fp8.py) - tests/test_persistent_cpu.py shows that a tile or item built from another one's
      operands would not, and that the caps reach every kind of step between tiles;
  (c) every hook is reset by the fixture below.

The last tests run the production grid without the hook, sized from the device's CU count.
Every check prints its worst err / budget ratio (`pytest -s`)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import numerics as nm
import numerics_fp8 as n8
import numerics_persistent as pz
from rajni_amd import ops, _native as nat

DEV = "cuda"
NBLK_DEFAULT = 1600 * 1024
# bit patterns no kernel output holds: NaNs (e4m3: the NaN code)
NAN_BYTE = 0x7F


@pytest.fixture(autouse=True)
def hooks_reset():
    yield
    lib = nat.lib()
    lib.rajni_debug_set_persistent_workgroups(0)
    lib.rajni_debug_force_gemm_tiling(0)
    lib.rajni_debug_force_f8_tiling(0)
    lib.rajni_debug_set_gemm_nblock_bytes(NBLK_DEFAULT)
    lib.rajni_debug_set_resid_stagger(1)


def cap(n):
    nat.lib().rajni_debug_set_persistent_workgroups(n)


def dev(a, dt):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
    return t if dt == "fp32" else t.to(nm.TORCH[dt])


def raw(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.float().cpu().numpy().astype(np.float64)


def bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def fresh(shape, dtype):
    """an output buffer no launch has written: NaN in every element (e4m3 bytes: the NaN code)"""
    if dtype == torch.uint8:
        return torch.full(shape, NAN_BYTE, dtype=torch.uint8, device=DEV)
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def no_nan(t):
    if t.dtype == torch.uint8:
        return not bool(((t & 0x7F) == 0x7F).any())
    return not bool(torch.isnan(t).any())


def same_bits(a, b):
    return torch.equal(bits(a.contiguous()), bits(b.contiguous()))


def report(got, want, budget, what):
    """the ratio line of nm.assert_within without the assertion (for bounds another module asserts)"""
    print(f"[numerics] {what}: worst err/budget {nm.worst_ratio(got, want, budget)[0]:.3f}")


def under_caps(run, caps, check, what, cols=slice(None)):
    """(a) and (b) for one launch form: run() launches into a fresh buffer and returns it; check(out, label) holds (b)"""
    cap(0)
    base = run()
    assert no_nan(base[..., cols]), f"{what}: the uncapped launch left NaN"
    for n in caps:
        cap(n)
        got = run()
        assert no_nan(got[..., cols]), f"{what}: cap {n} left NaN (a tile or item was skipped)"
        assert same_bits(got[..., cols], base[..., cols]), f"{what}: cap {n} differs from the uncapped launch"
        check(got, f"{what} cap {n}")
    cap(0)
    return base


# ---------------------------------------------------------------------------------------------------------------
# GEMM
# ---------------------------------------------------------------------------------------------------------------
COLS = slice(0, pz.N)


def resid_launcher(form, xd, wd, bd, K, kw):
    """gathered: a fresh output; in place: out = a fresh copy of the residual rows, as forward.hip calls fc2 - a tile
    visited twice would add twice"""
    gam = dev(form.gam, "fp32")
    idx = raw(form.idx) if form.gather else None
    r0 = dev(form.r, form.stream)
    r0[..., pz.N:] = float("nan")
    x3 = xd.reshape(pz.B_IMG, pz.NP, K)

    def run():
        if form.gather:
            out = fresh((pz.M, pz.LD), nm.TORCH[form.stream])
            ops.linear(x3, wd, pz.N, bd, nat.EPI_BIAS_RESID, gamma=gam, resid=r0, r_idx=idx, out=out, **kw)
            return out
        rd = r0.clone()
        ops.linear(x3, wd, pz.N, bd, nat.EPI_BIAS_RESID, gamma=gam, resid=rd, out=rd.reshape(pz.M, pz.LD), **kw)
        return rd.reshape(pz.M, pz.LD)
    return run


def stagger_and_nblock(run, base, form, nblock, what):
    lib = nat.lib()
    if form.epi == 2 and form.stream is not None:       # the residual stagger never changes a bit
        for units in (0, 2):
            lib.rajni_debug_set_resid_stagger(units)
            assert same_bits(run()[:, COLS], base[:, COLS]), f"{what}: stagger {units} differs from the default"
        lib.rajni_debug_set_resid_stagger(1)
    if nblock:                                          # N blocks of one and two column tiles under two workgroups
        cap(pz.NBLOCK_UNDER_CAP[0])
        for v in pz.NBLOCK_UNDER_CAP[1]:
            lib.rajni_debug_set_gemm_nblock_bytes(v)
            got = run()
            assert no_nan(got[:, COLS]) and same_bits(got[:, COLS], base[:, COLS]), f"{what}: N blocks {v} under a cap differ"
        lib.rajni_debug_set_gemm_nblock_bytes(NBLK_DEFAULT)
        cap(0)


@pytest.mark.parametrize("fmt,tiling,K", pz.GEMM16_CASES)
def test_gemm_16bit_under_caps(fmt, tiling, K):
    case = pz.gemm16_case(fmt, K)
    dt = case["dt"]
    xd, bd = dev(case["x"], dt), dev(case["b"], "fp32")
    if fmt == "w8":
        wd, kw = case["q"].to(DEV), dict(w_scale=case["s"].to(DEV))
    else:
        wd, kw = ops.pack_weight(dev(case["w"], dt), nm.TORCH[dt]), {}
    nat.lib().rajni_debug_force_gemm_tiling(tiling)
    for form in case["forms"]:
        what = f"persistent gemm16 {fmt} tiling {tiling} K {K} {form.name}"
        if form.epi == 2:
            run = resid_launcher(form, xd, wd, bd, K, kw)
        else:
            def run(form=form):
                out = fresh((pz.M, pz.LD), nm.TORCH[dt])
                ops.linear(xd, wd, pz.N, bd, form.epi, out=out, **kw)
                return out
        check = lambda got, label, form=form: nm.assert_within(host(got)[:, COLS], form.want, form.budget, label)
        base = under_caps(run, pz.GEMM_CAPS, check, what, COLS)
        # one epilogue per tiling also walks forced N blocks: GELU on the wide tiling, the in-place fp32-stream RESID on mid
        nblock = form.name == ("GELU" if tiling == 4 else "RESID fp32 in place")
        stagger_and_nblock(run, base, form, nblock, what)


@pytest.mark.parametrize("tiling,K", pz.F8_CASES)
def test_gemm_fp8_x_fp8_under_caps(tiling, K):
    case = pz.f8_case(K)
    xq, wp, bd = raw(case["xq"]), raw(case["wp"]), raw(case["b"])
    kw = dict(w_scale=raw(case["ws"]), x_scale=raw(case["xs"]))
    ys = raw(case["ys"])
    ld8 = (pz.N + 15) // 16 * 16
    nat.lib().rajni_debug_force_f8_tiling(tiling)
    for form in pz.f8_forms(case, tiling):
        what = f"persistent gemm fp8xfp8 tiling {tiling} K {K} {form.name}"
        if form.name == "BIAS":
            def run():
                out = fresh((pz.M, pz.LD), torch.bfloat16)
                ops.linear(xq, wp, pz.N, bd, nat.EPI_BIAS, out=out, **kw)
                return out

            def check(got, label):
                report(host(got)[:, COLS], form.want, form.budget, label)
                n8.check_bias(host(got)[:, COLS], form.want)
        elif form.name == "GELU8":
            def run():
                out = fresh((pz.M, ld8), torch.uint8)
                ops.linear(xq, wp, pz.N, bd, nat.EPI_BIAS_GELU, out=out, y_scale=ys, **kw)
                return out

            def check(got, label):
                deq = n8.e4m3_bytes_to_f64(got)[:, COLS] * case["ys"][:, None].astype(np.float64)
                report(deq, form.want, form.budget, label)
                n8.check_gelu8(deq, case["pre"], case["ys"])
                assert torch.equal(ys, raw(case["ys"])), "y_scale is an input of the GELU8 epilogue"
        else:
            run = resid_launcher(form, xq, wp, bd, K, kw)

            def check(got, label, form=form):
                g = host(got)[:, COLS]
                report(g, form.want, form.budget, label)
                if form.stream == "fp32":
                    n8.check_resid_f32(g, form.want)
                else:
                    assert (np.abs(g - form.want) <= form.budget).all(), label
        base = under_caps(run, pz.GEMM_CAPS, check, what, COLS)
        stagger_and_nblock(run, base, form, form.name == "BIAS", what)


@pytest.mark.parametrize("dt,out_f32,tiling,P", pz.PATCH_CASES)
def test_patch_embed_under_caps(dt, out_f32, tiling, P):
    case = pz.patch_case(dt, out_f32, P)
    img, cls, pos = dev(case["img"], dt), dev(case["cls"], dt), dev(case["pos"], dt)
    wd = ops.pack_weight(dev(case["w"], dt), nm.TORCH[dt], k_multiple=64)
    bd = dev(case["b"], "fp32")
    n, Cc = case["npatch"] + 1, pz.PATCH_C
    assert nat.lib().rajni_patch_embed_workspace_bytes(pz.PATCH_B, 3, pz.PATCH_S, P, nat.dtype_code(nm.TORCH[dt])) == 0   # fused loader
    nat.lib().rajni_debug_force_gemm_tiling(tiling)

    def run():
        x = fresh((pz.PATCH_B, n, Cc), nm.TORCH[case["out_dt"]])
        nat.check(nat.lib().rajni_patch_embed(img.data_ptr(), wd.data_ptr(), bd.data_ptr(), cls.data_ptr(), pos.data_ptr(), 1,
                                              x.data_ptr(), int(out_f32), pz.PATCH_B, 3, pz.PATCH_S, P, Cc,
                                              nat.dtype_code(nm.TORCH[dt]), None, 0, nat.stream_ptr(img.device)), "rajni_patch_embed")
        return x

    form = case["forms"][0]

    def check(got, label):
        g = host(got)
        nm.assert_within(g[:, 1:].reshape(-1, Cc), form.want, form.budget, label)
        nm.assert_within(g[:, 0], np.broadcast_to(case["cls_want"], (pz.PATCH_B, Cc)), case["cls_bud"], label + " CLS rows")
    under_caps(run, pz.PATCH_CAPS, check, f"persistent patch embed {dt} out_f32 {out_f32} tiling {tiling} P {P}")


# ---------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------
AB, AH, AD, AC = pz.ATTN_B, pz.ATTN_H, pz.ATTN_D, pz.ATTN_H * pz.ATTN_D


def attention_into(out, qkv, idx, n_kept, dtype, nq=None, Bq=AB):
    n_src = qkv.shape[1]
    a = (qkv.data_ptr(), nat.ptr(idx), out.data_ptr(), Bq, n_src, n_kept)
    b = (AH, AD, float(pz.ATTN_SCALE), nat.dtype_code(dtype), nat.stream_ptr(qkv.device))
    if nq is None:
        nat.check(nat.lib().rajni_attention(*a, *b), "rajni_attention")
    else:
        nat.check(nat.lib().rajni_debug_attention_rows(*a, nq, *b), "rajni_debug_attention_rows")
    return out


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("n_kept", pz.ATTN_NP)
def test_attention_under_caps(n_kept, dt):
    """15 items through 1, 2, 4 and 7 workgroups: cap 1 runs all of them through one workgroup's two LDS buffers"""
    for kind in pz.ATTN_KINDS:
        for gathered in (True, False):
            qkv, idx, want, bud = pz.attention_case(kind, n_kept, gathered, dt)
            qd, idd = dev(qkv, dt), (raw(idx) if gathered else None)
            run = lambda: attention_into(fresh((AB, n_kept, AC), nm.TORCH[dt]), qd, idd, n_kept, nm.TORCH[dt])
            check = lambda got, label: nm.assert_within(host(got), want, bud, label)
            under_caps(run, pz.ATTN_CAPS, check, f"persistent attention {dt} np {n_kept} {kind} {'gathered' if gathered else 'identity'}")


@pytest.mark.parametrize("n_kept", [n for n in pz.ATTN_NP if n <= 224])
def test_attention_fp8_output_under_caps(n_kept):
    """rajni_attention_fp8: e4m3 rows and row scales bit-equal to the uncapped call and within the e4m3 rule"""
    for kind in pz.ATTN_KINDS:
        for gathered in (True, False):
            qkv, idx, want, _ = pz.attention_case(kind, n_kept, gathered, "bf16")
            qd, idd = dev(qkv, "bf16"), (raw(idx) if gathered else None)
            scale = float(np.float32(np.abs(want).max() / 448.0))
            cap(0)
            ref = host(ops.attention(qd, idd, AH, pz.ATTN_SCALE))            # the bf16-output kernel: same products
            base = None
            for n in (0,) + pz.ATTN_CAPS:
                cap(n)
                out, rs = fresh((AB, n_kept, AC), torch.uint8), fresh((AB * n_kept,), torch.float32)
                nat.check(nat.lib().rajni_attention_fp8(qd.data_ptr(), nat.ptr(idd), out.data_ptr(), scale, rs.data_ptr(), AB,
                                                        qd.shape[1], n_kept, AH, AD, float(pz.ATTN_SCALE), nat.stream_ptr(qd.device)),
                          "rajni_attention_fp8")
                what = f"persistent attention e4m3 out np {n_kept} {kind} {'gathered' if gathered else 'identity'} cap {n}"
                assert no_nan(out) and no_nan(rs), what
                if base is None:
                    base = (out, rs)
                    continue
                assert torch.equal(out, base[0]) and same_bits(rs, base[1]), f"{what} differs from the uncapped call"
                report(n8.e4m3_bytes_to_f64(out) * np.float64(np.float32(scale)), ref, n8.attention_fp8_bound(ref, want, scale), what)
                n8.check_attention_fp8(out, rs, ref, want, scale)
            cap(0)


SENTINEL = {torch.bfloat16: 0x7FC1, torch.float16: 0x7E01}      # NaNs with a payload: no attention output holds them


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("n_kept", [87, 224])
def test_attention_rows_limited_under_caps(n_kept, dt):
    """rajni_debug_attention_rows (waves without queries take their own wait on the item pipeline): the rows written equal
    the all-rows call's, nothing past the 32-row tile that straddles nq is written"""
    dtype = nm.TORCH[dt]
    qkv, idx, want, bud = pz.attention_case("normal", n_kept, True, dt)
    qd, idd = dev(qkv, dt), raw(idx)
    cap(0)
    full = attention_into(fresh((AB, n_kept, AC), dtype), qd, idd, n_kept, dtype)
    assert no_nan(full)
    for nq in (1, 33):
        end = min(n_kept, (nq + 31) // 32 * 32)
        for n in (1, 4):
            cap(n)
            out = torch.empty((AB, n_kept, AC), dtype=dtype, device=DEV)
            bits(out).fill_(SENTINEL[dtype])
            attention_into(out, qd, idd, n_kept, dtype, nq=nq)
            what = f"persistent attention rows {dt} np {n_kept} nq {nq} cap {n}"
            assert same_bits(out[:, :end], full[:, :end]), f"{what}: a written row differs from the all-rows call"
            assert bool((bits(out[:, end:].contiguous()) == SENTINEL[dtype]).all()), f"{what}: rows past the straddling tile were written"
            nm.assert_within(host(out[:, :end]), want[:, :end], bud[:, :end], what)
    cap(0)


# ---------------------------------------------------------------------------------------------------------------
# the production grid, without the hook: 2 CUs + 5 tiles, 6 CUs + 5 items
# ---------------------------------------------------------------------------------------------------------------

def cu_count():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def production_shape(bn):
    """(M, N) of 2 * CUs + 5 tiles of 256 x bn, the last row tile (37 rows) and the last column tile (68 columns) ragged"""
    tiles_m, tiles_n = pz.factor_tiles(2 * cu_count() + 5)
    return (tiles_m - 1) * pz.BM + 37, (tiles_n - 1) * bn + 68, tiles_m


def row_slices(M, tiles_m):
    """(first X row, first row owned, end) of every row tile: a ragged last tile starts at M - 256"""
    return [(pz.plain_m0(i, M), i * pz.BM, min(M, i * pz.BM + pz.BM)) for i in range(tiles_m)]


def test_production_grid_wide_gelu_bf16():
    M, N, tiles_m = production_shape(256)
    K, ld = pz.K_MIN[4], (N + 7) // 8 * 8
    g = torch.Generator(device=DEV).manual_seed(M + N)
    x = torch.randn(M, K, generator=g, device=DEV).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g, device=DEV) * 0.05).to(torch.bfloat16)
    b = torch.randn(N, generator=g, device=DEV).to(torch.bfloat16).float()
    wd = ops.pack_weight(w)
    nat.lib().rajni_debug_force_gemm_tiling(4)
    out = fresh((M, ld), torch.bfloat16)
    ops.linear(x, wd, N, b, nat.EPI_BIAS_GELU, out=out)
    assert no_nan(out[:, :N])
    pre, S, gg = pz.gemm_pre_t(x, w, b)
    ratio = pz.worst_ratio_t(out[:, :N], pz.gelu_t(pre), pz.budget_gelu_t(pre, S, gg, "bf16", nm.A_GELU_16))
    print(f"[numerics] production gemm16 wide GELU bf16 {M}x{N}x{K} ({2 * cu_count() + 5} tiles on {cu_count()} CUs): worst err/budget {ratio:.3f}")
    assert ratio <= 1.0
    for m0, r0, r1 in row_slices(M, tiles_m):                   # one launch per 256-row slice: one tile per workgroup
        o = fresh((pz.BM, ld), torch.bfloat16)
        ops.linear(x[m0:m0 + pz.BM], wd, N, b, nat.EPI_BIAS_GELU, out=o)
        assert same_bits(o[r0 - m0:r1 - m0, :N], out[r0:r1, :N]), f"rows {r0}..{r1} differ from their own launch"


def test_production_grid_mid_resid_fp32_stream_in_place():
    M, N, tiles_m = production_shape(128)
    K, ld = pz.K_MIN[5], (N + 7) // 8 * 8
    g = torch.Generator(device=DEV).manual_seed(M + N)
    x = torch.randn(M, K, generator=g, device=DEV).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g, device=DEV) * 0.05).to(torch.bfloat16)
    b = torch.randn(N, generator=g, device=DEV).to(torch.bfloat16).float()
    gam = torch.randn(N, generator=g, device=DEV).to(torch.bfloat16).float()
    resid = torch.randn(1, M, ld, generator=g, device=DEV)
    wd = ops.pack_weight(w)
    nat.lib().rajni_debug_force_gemm_tiling(5)
    rd = resid.clone()
    ops.linear(x.reshape(1, M, K), wd, N, b, nat.EPI_BIAS_RESID, gamma=gam, resid=rd, out=rd.reshape(M, ld))
    out = rd.reshape(M, ld)
    assert no_nan(out[:, :N])
    pre, S, gg = pz.gemm_pre_t(x, w, b)
    want, bud = pz.budget_resid_t(pre, S, gg, resid[0, :, :N].double(), gam.double(), "fp32")
    ratio = pz.worst_ratio_t(out[:, :N], want, bud)
    print(f"[numerics] production gemm16 mid RESID fp32 in place {M}x{N}x{K} ({2 * cu_count() + 5} tiles on {cu_count()} CUs): worst err/budget {ratio:.3f}")
    assert ratio <= 1.0
    for m0, r0, r1 in row_slices(M, tiles_m):
        rs = resid[:, m0:m0 + pz.BM].clone()
        ops.linear(x[m0:m0 + pz.BM].reshape(1, pz.BM, K), wd, N, b, nat.EPI_BIAS_RESID, gamma=gam, resid=rs, out=rs.reshape(pz.BM, ld))
        assert same_bits(rs[0, r0 - m0:r1 - m0, :N], out[r0:r1, :N]), f"rows {r0}..{r1} differ from their own launch"


def test_production_grid_fp8_wide_gelu8():
    M, N, _ = production_shape(256)
    K = 512
    rng = np.random.default_rng([M, N, K])
    xq, xs, wp, ws, xd, wd = n8.f8_operands(rng, M, N, K)
    b = rng.standard_normal(N).astype(np.float32)
    pre = (raw(xd) @ raw(wd).T + raw(b).double()).cpu().numpy()              # fp64 on the device
    ys = n8.gelu8_row_scales(rng, pre)
    ysd = raw(ys)
    nat.lib().rajni_debug_force_f8_tiling(2)
    out = fresh((M, (N + 15) // 16 * 16), torch.uint8)
    ops.linear(raw(xq), raw(wp), N, raw(b), nat.EPI_BIAS_GELU, out=out, w_scale=raw(ws), x_scale=raw(xs), y_scale=ysd)
    assert no_nan(out[:, :N]) and torch.equal(ysd, raw(ys))
    deq = n8.e4m3_bytes_to_f64(out)[:, :N] * ys[:, None].astype(np.float64)
    h = pz.orc.gelu(pre)
    report(deq, h, n8.gelu8_bound(h, ys), f"production gemm fp8xfp8 wide GELU8 {M}x{N}x{K}")
    n8.check_gelu8(deq, pre, ys)


@pytest.mark.parametrize("n_kept", [87, 224])
def test_production_grid_attention(n_kept):
    """H * B >= 6 CUs + 5 items: every workgroup runs at least three, with a remainder"""
    Bq = -(-(6 * cu_count() + 5) // AH)
    n_src = n_kept + pz.ATTN_EXTRA
    g = torch.Generator(device=DEV).manual_seed(n_kept)
    qkv = torch.randn(Bq, n_src, 3 * AC, generator=g, device=DEV).to(torch.bfloat16)
    idx = torch.rand(Bq, n_src, generator=g, device=DEV).argsort(dim=1)[:, :n_kept].sort(dim=1).values.to(torch.int32).contiguous()
    out = attention_into(fresh((Bq, n_kept, AC), torch.bfloat16), qkv, idx, n_kept, torch.bfloat16, Bq=Bq)
    assert no_nan(out)
    gathered = qkv.gather(1, idx.long()[:, :, None].expand(-1, -1, 3 * AC))
    want, bud = pz.attention_budget_t(gathered, AH, pz.ATTN_SCALE, "bf16")
    ratio = pz.worst_ratio_t(out, want, bud)
    print(f"[numerics] production attention bf16 np {n_kept} ({Bq * AH} items on {cu_count()} CUs): worst err/budget {ratio:.3f}")
    assert ratio <= 1.0
    each = fresh((Bq, n_kept, AC), torch.bfloat16)
    for i in range(Bq):                                                      # one launch per image: one item per workgroup
        attention_into(each[i:i + 1], qkv[i:i + 1], idx[i:i + 1], n_kept, torch.bfloat16, Bq=1)
    assert no_nan(each) and same_bits(each, out)
