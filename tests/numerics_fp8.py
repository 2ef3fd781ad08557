"""References and bounds of the fp8 kernels (fp8 x fp8 GEMM epilogues, e4m3 attention output), shared by
tests/test_gpu_fp8_mfma.py and tests/test_gpu_persistent.py so that both hold a kernel to the SAME rule.  Pure numpy /
torch-CPU.  Every reference is fp64 numpy on the DEQUANTISED operands (e4m3 code x fp32 row scale)."""
import numpy as np
import torch

from oracle import rajni_oracle as orc


def e4m3_bytes_to_f64(q: torch.Tensor) -> np.ndarray:
    return q.cpu().view(torch.float8_e4m3fn).to(torch.float32).numpy().astype(np.float64)


def random_e4m3(rng, shape):
    """uniform random e4m3 codes without the two NaN patterns (0x7F, 0xFF)"""
    b = rng.integers(0, 256, size=shape, dtype=np.uint8)
    b[(b & 0x7F) == 0x7F] = 0x38
    return b


def f8_operands(rng, M, N, K):
    """(x codes [M,K], x scales, W codes zero padded to whole 256-row tiles, W scales, dequantised x, dequantised W)"""
    xq, wq = random_e4m3(rng, (M, K)), random_e4m3(rng, (N, K))
    # keep products tame: scales so that dequantised entries are O(1)
    xs = (rng.uniform(0.5, 2.0, size=M) / 64.0).astype(np.float32)
    ws = (rng.uniform(0.5, 2.0, size=N) / 64.0).astype(np.float32)
    npad = (N + 255) // 256 * 256
    wp = np.zeros((npad, K), np.uint8)
    wp[:N] = wq
    xd = e4m3_bytes_to_f64(torch.from_numpy(xq)) * xs[:, None]
    wd = e4m3_bytes_to_f64(torch.from_numpy(wq)) * ws[:, None]
    return xq, xs, wp, ws, xd, wd


def gelu8_row_scales(rng, pre):
    """per-row output scale of the GELU8 epilogue: a bound on the row, not its maximum"""
    return (np.abs(pre).max(axis=1) * rng.uniform(1.0, 8.0, size=pre.shape[0]) / 448.0).astype(np.float32)


# ---- bounds: |got - want| <= bound, element by element (a scalar bound holds for every element) ----------------

def bias_bound(want):
    """EPI_BIAS, bf16 output"""
    return 2.0 ** -8 * np.abs(want).max() + 1e-3


def resid_f32_bound(want):
    """EPI_RESID on the fp32 stream: fp32 accumulation over K <= 3072 wide-range terms"""
    return 1e-4 * np.abs(want).max()


def gelu8_bound(h, ys):
    """e4m3 output of gelu(pre) with row scale ys: half an ulp = 2^-4 relative in the normal range, scale * 2^-10 below it"""
    return np.maximum(np.abs(h) * 2.0 ** -4, ys[:, None] * 2.0 ** -10) * 1.01 + 2e-4 * np.abs(h).max()


GELU8_RULE_MISMATCH = 5e-3      # fp32 accumulation order + the 4e-5 GELU polynomial near boundaries


def check_bias(got, want):
    assert np.abs(got - want).max() <= bias_bound(want)


def check_resid_f32(got, want):
    assert np.abs(got - want).max() <= resid_f32_bound(want)


def check_gelu8(deq, pre, ys):
    """deq = the stored e4m3 values x ys; pre = the fp64 pre-activation"""
    h = orc.gelu(pre)
    assert (np.abs(deq - h) <= gelu8_bound(h, ys)).all()
    want = orc.quantize_rows_e4m3(h, ys)
    assert np.mean(want != deq) < GELU8_RULE_MISMATCH


def attention_fp8_bound(ref, want, scale):
    """rajni_attention_fp8 against `ref`, the 16-bit-output kernel's result on the same inputs (same products).
    e4m3: half an ulp = 2^-4 relative in the normal range, scale * 2^-10 absolute below it; on top, what separates the two
    kernels' own roundings of the same fp32 value (bf16 output: 2^-9 relative)"""
    return np.maximum(np.abs(ref) * 2.0 ** -4, scale * 2.0 ** -10) * 1.001 + np.abs(ref) * 2.0 ** -8 + 1e-6 * np.abs(want).max()


def check_attention_fp8(out, rs, ref, want, scale):
    """out uint8 [B, Np, C], rs fp32 row scales (device tensors), ref = the bf16-output kernel (fp64 numpy), want = fp64
    attention, scale = the out_scale passed in"""
    assert (rs.cpu().numpy() == np.float32(scale)).all()
    deq = e4m3_bytes_to_f64(out) * np.float64(np.float32(scale))
    bound = attention_fp8_bound(ref, want, scale)
    assert (np.abs(deq - ref) <= bound).all(), float((np.abs(deq - ref) - bound).max())
    assert np.abs(deq - want).max() <= (2.0 ** -4 + 1.5e-2) * np.abs(want).max()
    # byte for byte the stated rule applied to the bf16 kernel's output, except where that output sits within its own
    # rounding of an e4m3 boundary
    rule = orc.quantize_rows_e4m3(ref, np.float32(scale))
    assert np.mean(rule != deq) < 0.08
