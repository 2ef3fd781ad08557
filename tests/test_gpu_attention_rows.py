"""Attention limited to the first query rows (rajni_debug_attention_rows, include/rajni_hip_debug.h) against the all-rows
launch: the limited launch runs the same kernel and instantiation with the query tiles that hold none of the wanted rows
switched off (head dim 64 on 16-bit operands) or not launched (grid.x of the other kernels), so the rows it writes must be
the all-rows launch's rows BIT FOR BIT, and it must write nothing past the tile that holds the last wanted row.

The last block of the forward relies on this with nq = 1 (the head reads x[:, 0] only)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rajni_amd import _native as nat
from rajni_amd import ops

DEV = "cuda"
B = 3
# (id, dtype, H, D, np, n_src (None: identity selection), rows of the first query tile)
#   persistent head-dim-64 kernel: one wave = 32 query rows; NSUB = ceil(np / 32) picks the instantiation
#   chunked head-dim-64 kernel (np > 256): 128-row workgroups of four 32-row waves, the waves past nq are switched off
#   general head dims: 128 query rows per workgroup;  fp32: 64 query rows per workgroup
CASES = [
    ("persistent_nsub1", torch.bfloat16, 2, 64, 17, None, 32),
    ("persistent_nsub3", torch.bfloat16, 3, 64, 87, None, 32),
    ("persistent_nsub7", torch.bfloat16, 2, 64, 197, None, 32),
    ("persistent_nsub8", torch.bfloat16, 2, 64, 256, None, 32),
    ("persistent_fp16", torch.float16, 2, 64, 87, None, 32),
    ("persistent_gathered", torch.bfloat16, 3, 64, 87, 121, 32),
    ("chunked", torch.bfloat16, 2, 64, 300, None, 32),
    ("dgen_d80", torch.bfloat16, 2, 80, 70, None, 128),
    ("fp32_d64", torch.float32, 2, 64, 70, None, 64),
    ("fp32_dgen_d32", torch.float32, 3, 32, 70, None, 64),
]
# bit patterns no attention output holds: NaNs with a payload (positive as int16 / int32)
SENTINEL = {torch.bfloat16: 0x7FC1, torch.float16: 0x7E01, torch.float32: 0x7FC00001}


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("name,dtype,H,D,n_kept,n_src,tile", CASES, ids=[c[0] for c in CASES])
def test_first_query_rows_equal_the_all_rows_launch(name, dtype, H, D, n_kept, n_src, tile):
    gen = torch.Generator(device=DEV).manual_seed(n_kept * 131 + D)
    C = H * D
    src = n_src or n_kept
    qkv = torch.randn(B, src, 3 * C, generator=gen, device=DEV).to(dtype)
    idx = None
    if n_src is not None:   # CLS first, then ascending patch rows - what a pruning stage selects
        rows = [torch.cat([torch.zeros(1, dtype=torch.long, device=DEV),
                           1 + torch.randperm(src - 1, generator=gen, device=DEV)[:n_kept - 1].sort().values]) for _ in range(B)]
        idx = torch.stack(rows).to(torch.int32).contiguous()
    scale = D ** -0.5
    full = ops.attention(qkv, idx, H, scale)
    assert torch.isfinite(full.float()).all()
    out = torch.empty_like(full)
    _bits(out).fill_(SENTINEL[dtype])
    nat.check(nat.lib().rajni_debug_attention_rows(qkv.data_ptr(), nat.ptr(idx), out.data_ptr(), B, src, n_kept, 1, H, D,
                                                   float(scale), nat.dtype_code(dtype), nat.stream_ptr(qkv.device)),
              "rajni_debug_attention_rows")
    torch.cuda.synchronize()
    got = _bits(out).reshape(B, n_kept, H, D)
    want = _bits(full).reshape(B, n_kept, H, D)
    row_untouched = (got == SENTINEL[dtype]).all(dim=-1)       # [B, np, H]: this (image, row, head) slice was not written
    row_equal = (got == want).all(dim=-1)
    assert (row_untouched | row_equal).all(), f"{name}: a written row differs from the all-rows launch"
    assert row_equal[:, 0, :].all(), f"{name}: row 0 of some (image, head) is missing or differs"
    assert row_untouched[:, tile:, :].all(), f"{name}: rows past the first query tile ({tile} rows) were written"
    # the whole first tile is computed and stored (the rows of it that exist)
    assert row_equal[:, :min(tile, n_kept), :].all()


def test_the_row_limit_is_checked_and_np_rows_is_the_plain_launch():
    H, D, n = 2, 64, 40
    qkv = torch.randn(2, n, 3 * H * D, device=DEV).to(torch.bfloat16)
    full = ops.attention(qkv, None, H, 0.125)
    out = torch.zeros_like(full)
    call = lambda nq: nat.lib().rajni_debug_attention_rows(qkv.data_ptr(), None, out.data_ptr(), 2, n, n, nq, H, D, 0.125,
                                                           nat.RAJNI_BF16, nat.stream_ptr(qkv.device))
    for bad in (0, -1, n + 1):
        assert call(bad) != 0 and b"nq" in nat.lib().rajni_last_error()
    assert call(n) == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(full))
    assert not np.isnan(out.float().cpu().numpy()).any()
