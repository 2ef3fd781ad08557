"""Host-side arithmetic behind the large-offset tests, no GPU: workspace sizes beyond 2^32 and 2^35 bytes against a Python
big-int restatement of the layouts, and the refusals that protect the 32-bit quantities the kernels keep (include/rajni_hip.h,
"addressing limits").  Every refusal here is reached with NULL buffers: the limits are checked before the pointers, so
nothing can be launched by these calls, with or without a device."""
import ctypes as C

import pytest

import numerics_tiled as nt
from rajni_amd import _native as nat

T31, T32, T35 = 1 << 31, 1 << 32, 1 << 35
F32, BF16, F16 = nat.RAJNI_F32, nat.RAJNI_BF16, nat.RAJNI_F16


def lib():
    return nat.lib()


def last_error():
    return lib().rajni_last_error().decode()


# ---------------------------------------------------------------------------------------------------------------
# workspace sizes
# ---------------------------------------------------------------------------------------------------------------

def align256(v):
    return (v + 255) // 256 * 256


def patch_ws(B, Cin, S, patch, dtype):
    """rajni_patch_embed_workspace_bytes: 0 where the im2col is fused into the loads (power-of-two patch >= 8, S % 8 == 0,
    Cin * patch^2 % 64 == 0), else the zero-padded column matrix [B * (S / patch)^2, ceil64(Cin * patch^2)]"""
    k = Cin * patch * patch
    if patch >= 8 and patch & (patch - 1) == 0 and S % 8 == 0 and k % 64 == 0:
        return 0
    return B * (S // patch) ** 2 * ((k + 63) // 64 * 64) * (4 if dtype == F32 else 2)


def score_ws(B, N, H, D):
    """rajni_score_select_workspace_bytes: 0 where one workgroup's 160 KiB of LDS hold the shape, else the tiled layout"""
    if nt.single_workgroup_lds_bytes(N, H, D) <= 160 * 1024 or N > nt.MAX_N:
        return 0
    return nt.workspace_bytes(B, N, H, D)


def vit_ws(B, S, patch, Cc, H, hidden, dtype, resid_bf16, act_fp8, P, Cin=3):
    """the regions of carve() in csrc/forward.hip, each rounded up to 256 bytes: xa, xb (residual stream, fp32 unless
    resid_bf16), xn, qkv, att, hid, cls rows, carried scores, patch columns, two act_fp8 scale vectors, score scratch"""
    n0 = (S // patch) ** 2 + P
    rows = B * n0
    es = 4 if dtype == F32 else 2
    xs = 4 if (dtype == F32 or not resid_bf16) else 2
    regions = [rows * Cc * xs, rows * Cc * xs, rows * Cc * es, rows * 3 * Cc * es, rows * Cc * es, rows * hidden * es, B * Cc * es,
               rows * es, patch_ws(B, Cin, S, patch, dtype), rows * 4 if act_fp8 else 0, rows * 4 if act_fp8 else 0,
               score_ws(B, n0, H, Cc // H)]
    return sum(align256(r) for r in regions)


def plan(B, S, patch, Cc, H, hidden, dtype, resid_bf16, act_fp8):
    p = nat.VitPlan()
    p.dtype, p.B, p.in_chans, p.img_size, p.patch_size = dtype, B, 3, S, patch
    p.C, p.H, p.D, p.depth, p.hidden, p.num_classes = Cc, H, Cc // H, 1, hidden, 1000
    p.resid_bf16, p.act_fp8 = int(resid_bf16), int(act_fp8)
    return p


def native_ws(B, S, patch, Cc, H, hidden, dtype, resid_bf16, act_fp8, P):
    p = plan(B, S, patch, Cc, H, hidden, dtype, resid_bf16, act_fp8)
    if P == 1:
        return lib().rajni_vit_workspace_bytes(C.byref(p))
    reg = (C.c_char * 16)()                      # only its address is looked at (non-NULL with num_prefix > 1)
    pre = nat.VitPrefix(P, C.cast(reg, C.c_void_p))
    return lib().rajni_vit_workspace_bytes_prefix(C.byref(p), C.byref(pre))


# (name, S, patch, C, H, hidden, B): totals beyond 2^32 bytes (all) and, with the fp32 residual stream, 2^35 bytes (the first two)
BIG_PLANS = [("vit_large_patch14_518", 518, 14, 1024, 16, 4096, 1024),
             ("vit_base_patch16_2048", 2048, 16, 768, 12, 3072, 256),
             ("vit_huge_patch14_224", 224, 14, 1280, 16, 5120, 4096)]


@pytest.mark.parametrize("P", [1, 5])
@pytest.mark.parametrize("dtype,resid_bf16,act_fp8", [(BF16, 0, 0), (BF16, 0, 1), (BF16, 1, 0), (BF16, 1, 1), (F16, 0, 0), (F32, 0, 0)])
@pytest.mark.parametrize("name,S,patch,Cc,H,hidden,B", BIG_PLANS, ids=[p[0] for p in BIG_PLANS])
def test_vit_workspace_bytes_beyond_2_32_and_2_35(name, S, patch, Cc, H, hidden, B, dtype, resid_bf16, act_fp8, P):
    want = vit_ws(B, S, patch, Cc, H, hidden, dtype, resid_bf16, act_fp8, P)
    assert want > T32
    if not resid_bf16 and name != "vit_huge_patch14_224":
        assert want > T35
    assert native_ws(B, S, patch, Cc, H, hidden, dtype, resid_bf16, act_fp8, P) == want
    # strictly monotone in B, through the sizes at which totals pass 2^31, 2^32 and 2^35
    sizes = [native_ws(b, S, patch, Cc, H, hidden, dtype, resid_bf16, act_fp8, P) for b in (1, 2, 3, 64, 65, B // 2, B - 1, B, B + 1, 4 * B)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    assert sizes[-1] == vit_ws(4 * B, S, patch, Cc, H, hidden, dtype, resid_bf16, act_fp8, P)


def test_every_region_of_a_large_plan_is_sized_in_64_bits():
    """ViT-L/14 at 518 px, B = 1024: the hidden buffer alone holds 5.7e9 elements, qkv 4.3e9 - each region's own size is past
    2^32, so a 32-bit product anywhere in carve() changes the total"""
    name, S, patch, Cc, H, hidden, B = BIG_PLANS[0]
    rows = B * ((S // patch) ** 2 + 1)
    assert rows * hidden > T32 and rows * 3 * Cc > T32 and rows * Cc * 4 > T32
    assert native_ws(B, S, patch, Cc, H, hidden, BF16, 0, 0, 1) == vit_ws(B, S, patch, Cc, H, hidden, BF16, 0, 0, 1)


@pytest.mark.parametrize("B,N,H,D", [(256, 16385, 12, 64), (688, 16384, 1, 64), (1024, 1370, 16, 64), (65535, 16416, 16, 64),
                                     (4096, 257, 16, 80), (19400, 577, 1, 64)])
def test_score_select_workspace_bytes_at_large_batches(B, N, H, D):
    want = score_ws(B, N, H, D)
    assert lib().rajni_score_select_workspace_bytes(B, N, H, D, BF16) == want
    if want:
        assert lib().rajni_score_select_workspace_bytes(B + 1, N, H, D, F32) > want
    assert (want == 0) == (N < 600)
    if B == 65535:
        assert want > T35


@pytest.mark.parametrize("B,S,patch,dtype", [(14300, 224, 14, BF16), (14300, 224, 16, BF16), (4096, 518, 14, F32), (256, 2048, 16, BF16),
                                             (65535, 224, 14, F32), (3, 70, 10, F16)])
def test_patch_embed_workspace_bytes_at_large_batches(B, S, patch, dtype):
    want = patch_ws(B, 3, S, patch, dtype)
    assert lib().rajni_patch_embed_workspace_bytes(B, 3, S, patch, dtype) == want
    assert (want == 0) == (patch == 16)
    if want:
        assert lib().rajni_patch_embed_workspace_bytes(B + 1, 3, S, patch, dtype) > want
    if B >= 4096 and patch == 14:
        assert want > T32


# ---------------------------------------------------------------------------------------------------------------
# refusals before any launch
# ---------------------------------------------------------------------------------------------------------------
QK_MAX_GROUPS = T31 - 1024        # RAJNI_QK_NORM_MAX_GROUPS: rows * 2 * H must stay below it
GRID_YZ = 65535                   # RAJNI_MAX_GRID_YZ


def qk_norm_null(rows, H, D=64):
    return lib().rajni_qk_norm(None, None, None, None, None, rows, H, D, 1e-6, BF16, None)


@pytest.mark.parametrize("H", [1, 16])
def test_qk_norm_refuses_at_its_group_limit_and_not_one_row_below(H):
    rows = QK_MAX_GROUPS // (2 * H)
    assert rows * 2 * H == QK_MAX_GROUPS
    assert qk_norm_null(rows, H) == 2
    assert str(QK_MAX_GROUPS - 1) in last_error() and str(QK_MAX_GROUPS) in last_error(), last_error()
    assert qk_norm_null(rows + 7, H) == 2
    # one row fewer is inside the limit: the call gets as far as its pointer check (and nowhere near a launch)
    assert qk_norm_null(rows - 1, H) == 1
    assert "null pointer" in last_error()


def attention_null(B, n_src, n_p, H, D, dtype=BF16):
    return lib().rajni_attention(None, None, None, B, n_src, n_p, H, D, 0.125, dtype, None)


def attention_fp8_null(B, n_src, n_p, H):
    return lib().rajni_attention_fp8(None, None, None, 1.0, None, B, n_src, n_p, H, 64, 0.125, None)


@pytest.mark.parametrize("dtype", [BF16, F16, F32])
def test_attention_refuses_more_images_or_heads_than_a_grid_axis_takes(dtype):
    for B, H in ((GRID_YZ + 1, 1), (1, GRID_YZ + 1), (1 << 20, 12)):
        assert attention_null(B, 197, 197, H, 64, dtype) == 2
        assert str(GRID_YZ) in last_error(), last_error()
    assert attention_null(GRID_YZ, 197, 197, 1, 64, dtype) == 1 and "null pointer" in last_error()
    assert attention_null(1, 16, 16, GRID_YZ, 64, dtype) == 1 and "null pointer" in last_error()
    assert attention_fp8_null(GRID_YZ + 1, 197, 197, 12) == 2 and str(GRID_YZ) in last_error()
    assert attention_fp8_null(GRID_YZ, 197, 197, 12) == 1


def test_attention_refuses_an_image_beyond_its_32_bit_row_offsets():
    """the persistent kernel (head dim 64, 16-bit, up to 256 kept tokens) and its e4m3-output form address rows inside one
    image with a 32-bit byte offset, so n_src * 3 * H * 64 * 2 bytes per image must stay below 2^32.  16416 tokens (the score
    path's cap) fit at every head count up to 340."""
    H = 12
    row_bytes = 3 * H * 64 * 2
    n_ok = (T32 - 1) // row_bytes
    assert n_ok > 16416 * 50
    assert attention_null(2, n_ok + 1, 197, H, 64) == 2 and "2^32" in last_error()
    assert attention_null(2, n_ok, 197, H, 64) == 1 and "null pointer" in last_error()
    assert attention_fp8_null(2, n_ok + 1, 197, H) == 2 and "2^32" in last_error()
    assert attention_fp8_null(2, n_ok, 197, H) == 1
    assert attention_null(2, n_ok + 1, 256, H, 64, F16) == 2
    # the online (more than 256 kept tokens), fp32 and general head dim kernels form 64-bit offsets: no such limit
    assert attention_null(2, n_ok + 1, 257, H, 64) == 1
    assert attention_null(2, n_ok + 1, 197, H, 64, F32) == 1
    assert attention_null(2, n_ok + 1, 197, H, 80) == 1


def score_ws_null(B, N, H=1, D=64, dtype=BF16):
    return lib().rajni_score_select_ws(None, B, N, H, D, 1e-6, 1, N // 2, None, None, None, dtype, None, 0, None)


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_tiled_score_path_refuses_more_images_than_its_grid_takes(dtype):
    """the tiled launch is dim3(token tiles, B): B <= 65535.  The single-workgroup launch is dim3(B) and has no such limit."""
    assert score_ws_null(GRID_YZ + 1, 16384, dtype=dtype) == 2
    assert str(GRID_YZ) in last_error() and "tiled" in last_error(), last_error()
    assert score_ws_null(GRID_YZ, 16384, dtype=dtype) == 1 and "qkv is null" in last_error()
    assert score_ws_null(GRID_YZ + 1, 197, dtype=dtype) == 1 and "qkv is null" in last_error()


def test_forward_refuses_more_images_than_its_attention_launches_take():
    """every block's attention is launched on grid (q tiles, H, B): the forward checks B <= 65535 with the rest of the plan,
    before its first kernel, instead of meeting the attention refusal after patch embed, norm1 and qkv have run.  The plan
    here has no weights and no workspace, and images / logits are host bytes nothing reads: only the order of the checks lets
    the call return 2 (and, one image below the limit, 1 for the missing weights)."""
    p = plan(GRID_YZ + 1, 224, 16, 768, 12, 3072, BF16, 0, 0)
    blocks = (nat.Block * 1)()
    p.blocks = blocks
    host = (C.c_char * 16)()
    addr = C.cast(host, C.c_void_p)
    assert lib().rajni_vit_forward(C.byref(p), addr, addr, None) == 2
    assert str(GRID_YZ) in last_error() and "rajni_vit_forward" in last_error(), last_error()
    p.B = GRID_YZ
    assert lib().rajni_vit_forward(C.byref(p), addr, addr, None) == 1
    assert "null weight pointer" in last_error(), last_error()


# ---------------------------------------------------------------------------------------------------------------
# tests/bigmem.py itself (on the CPU, small sizes)
# ---------------------------------------------------------------------------------------------------------------

def _big(free_gib=100, **kw):
    import bigmem as bm
    return bm.Big("cpu", mem_get_info=lambda: (free_gib << 30, 256 << 30), **kw)


def test_bigmem_periodic_fill_and_check_find_one_changed_element():
    import torch
    import bigmem as bm
    b = _big()
    for dtype in (torch.bfloat16, torch.float32, torch.uint8):
        x = b.dense((1000, 8), dtype)
        block = (torch.arange(37 * 8).reshape(37, 8) % 251).to(dtype)
        bm.periodic_fill(x, block)
        assert torch.equal(x[37 * 5 + 3], block[3]) and torch.equal(x[999], block[999 % 37])
        for chunk in (1, 5, 64):
            bm.assert_periodic(x, 37, periods_per_chunk=chunk)
        for row in (37, 500, 999):
            y = x.clone()
            y[row, 7] += 1
            with pytest.raises(AssertionError, match=f"row {row} differs from row {row % 37}"):
                bm.assert_periodic(y, 37, periods_per_chunk=5)
    nan = torch.full((80, 4), float("nan"))
    bm.assert_periodic(nan, 7)                       # bit-for-bit: NaN rows are equal to themselves
    z = torch.zeros((80, 4))
    z[50, 1] = -0.0
    with pytest.raises(AssertionError, match="row 50"):
        bm.assert_periodic(z, 7)                     # ... and -0 is not +0


def test_bigmem_strided_rows_tail_slices_and_thresholds():
    import torch
    import bigmem as bm
    b = _big()
    v = b.rows(5, 3, 100, torch.float32)
    assert v.shape == (5, 3) and v.stride() == (100, 1) and b.held == (4 * 100 + 3) * 4
    assert bm.row_offset_bytes(v, 4) == 1600
    t = torch.arange(60.0).reshape(6, 10)
    s = bm.tail_slice(t, 4)
    assert s.shape == (2, 10) and s.data_ptr() == t.data_ptr() + 160 and float(s[0, 0]) == 40.0
    ld = (1 << 21) + 64
    assert bm.first_row_past(ld, bm.T31) == 1024 and 1023 * ld < bm.T31 <= 1024 * ld
    assert bm.crossings(1099 * ld + 256, 2) == {"2^31 bytes": True, "2^32 bytes": True, "2^31 elements": True}
    assert bm.crossings(16000 * 173 * 768, 2) == {"2^31 bytes": True, "2^32 bytes": False, "2^31 elements": False}
    with pytest.raises(AssertionError, match="does not cross"):
        bm.assert_crosses_all(16000 * 173 * 768, 2, "dst")
    a, c = torch.tensor([1.0, float("nan")]), torch.tensor([1.0, float("nan")])
    bm.assert_bit_equal(a, c, "same bits")
    with pytest.raises(AssertionError, match="1 of 2 elements differ"):
        bm.assert_bit_equal(a, torch.tensor([1.0, 2.0]), "different bits")


def test_bigmem_cap_and_skip_with_the_numbers():
    import torch
    import bigmem as bm
    b = _big(cap=1 << 20)
    b.empty(600 << 10)
    with pytest.raises(AssertionError, match="the cap is"):
        b.empty(600 << 10)
    b.close()
    assert b.held == 0
    assert bm.CAP_BYTES == 24 * bm.GIB
    with bm.big_empty(1000, torch.float32, device="cpu", mem_get_info=lambda: (8 << 30, 8 << 30)) as t:
        assert t.shape == (250,) and t.dtype == torch.float32
    short = _big(free_gib=5)
    with pytest.raises(pytest.skip.Exception, match=r"needs 4\.00 GiB .* 5\.00 GiB are free"):
        short.reserve(4 * bm.GIB)                    # 4 GiB + 2 GiB headroom > 5 GiB free
    assert short.held == 0
    short.reserve(2 * bm.GIB)
