#!/usr/bin/env python3
"""Coefficients of the packed-FMA GELU in csrc/gemm.hip: h(x) = 0.5*erf(x/sqrt2) ~= xc*P(xc^2)."""
import numpy as np
from scipy.special import erf
zmax, n = 3.0, 9
u = (np.cos(np.pi * (np.arange(4000) + 0.5) / 4000) + 1) / 2 * zmax ** 2
z = np.sqrt(u)
f = np.where(z > 1e-8, erf(z) / np.maximum(z, 1e-30), 2 / np.sqrt(np.pi))
V = np.vander(u, n, increasing=True)
w = z + 1e-3
a, *_ = np.linalg.lstsq(V * w[:, None], f * w, rcond=None)
c = [0.5 / np.sqrt(2) * a[i] / 2 ** i for i in range(n)]
print("X0 =", zmax * np.sqrt(2))
print(", ".join("%.9ef" % v for v in c))
# the kernel's own evaluation order in fp32 (gelu_pk): fused multiply-adds, and the LOWER-clamped x as the final multiplier
# (with the unclamped x the residual 0.5 + h(-X0) = 2.8e-6 would scale with |x|: -2.8e-2 at x = -1e4)
f32 = np.float32
X0 = f32(zmax * np.sqrt(2))


def fma(a, b, k):
    return (a.astype(np.float64) * b.astype(np.float64) + np.float64(k)).astype(f32)


def gelu_pk(x):
    xl = np.maximum(x.astype(f32), -X0)
    xc = np.minimum(xl, X0)
    u = xc * xc
    acc = np.full_like(xl, f32(c[-1]))
    for v in c[-2::-1]:
        acc = fma(acc, u, f32(v))
    return fma(xl, xc * acc, xl * f32(0.5))


def gelu64(x):
    x = x.astype(np.float64)
    return 0.5 * x * (1 + erf(x / np.sqrt(2)))


x = np.linspace(-8, 8, 400001).astype(f32)
x = np.concatenate([x, [np.nextafter(X0, f32(0)), X0, np.nextafter(X0, f32(9))]]).astype(f32)
x = np.concatenate([x, -x])
print("max |gelu err| on [-8, 8] (fp32 fma Horner) = %.3e" % np.abs(gelu_pk(x) - gelu64(x)).max())
t = -(2.0 ** np.arange(3, 17)).astype(f32)
print("max |gelu err| for x = -2^3 .. -2^16        = %.3e" % np.abs(gelu_pk(t) - gelu64(t)).max())
