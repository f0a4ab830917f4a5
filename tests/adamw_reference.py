"""The referee of the AdamW tests: torch.optim.AdamW's update evaluated in float64, per-element error bounds for an fp32
implementation of it, and the adversarial optimiser state both are checked on.  Plain torch, any device.

    p  <- p (1 - lr wd)
    m' = b1 m + (1 - b1) g
    v' = b2 v + (1 - b2) g^2
    den = sqrt(v') / sqrt(1 - b2^step) + eps
    p' = p - lr / (1 - b1^step) m' / den

The hyper-parameters are rounded to float32 first and widened to double then: that is what arrives through the library's c_float ABI
and what its host-side scalar set-up (adam_hyper) sees.  An fp32 optimiser under test gets the same rounded values (`f32`).

Bounds, u = 2^-24 (the unit roundoff of fp32), from counting roundings -- derived, not tuned:

    |dm| <= 4 u (|m| + |g|) + FLT_MIN                        3 roundings + the rounding of 1 - b1 to fp32
    |dv| <= 4 u (v + g^2) + FLT_MIN                          4 roundings
    |dp| <= 8 u (|p| + step_size (|m| + |g|) / den) + FLT_MIN    decay, rounded step size, division, square root, subtraction

p' inherits the absolute error of m', which is not small relative to m' where m + (1 - b1)(g - m) cancels: the scale is |m| + |g|, not
|m'|.  The FLT_MIN floor leaves the handling of denormal results open.  The bounds leave room for a division or square root 1-2 ulp off
correct rounding and none for another formula (tests/test_adamw_reference_cpu.py: ten wrong optimisers, each caught)."""
import math

import numpy as np
import torch

U = 2.0 ** -24
FLT_MIN = float(np.finfo(np.float32).tiny)

#: (lr, beta1, beta2, eps, weight_decay, step)
HYPER_SETS = (
    (3e-5, 0.9, 0.999, 1e-8, 0.01, 1),
    (3e-5, 0.9, 0.999, 1e-8, 0.01, 2),
    (1e-3, 0.8, 0.95, 1e-4, 0.1, 7),
    (1e-3, 0.9, 0.999, 1e-8, 0.01, 1000),
    (2e-2, 0.5, 0.9, 1e-6, 0.3, 100000),
    (1e-3, 0.9, 0.999, 1e-8, 0.0, 3),
    (1.0, 0.9, 0.999, 1e-8, 0.5, 1),
)


def f32(x):
    """A Python float rounded to float32 and widened again."""
    return float(np.float32(x))


def _scalars(lr, beta1, beta2, eps, wd, step):
    lr, beta1, beta2, eps, wd = (f32(x) for x in (lr, beta1, beta2, eps, wd))
    step = int(step)
    return lr, beta1, beta2, eps, wd, lr / (1.0 - beta1 ** step), math.sqrt(1.0 - beta2 ** step)


def reference(p, g, m, v, lr, beta1, beta2, eps, wd, step):
    """-> (p', m', v') in float64."""
    lr, beta1, beta2, eps, wd, step_size, bc2_sqrt = _scalars(lr, beta1, beta2, eps, wd, step)
    p, g, m, v = (t.double() for t in (p, g, m, v))
    p = p * (1.0 - lr * wd)
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    den = v.sqrt() / bc2_sqrt + eps
    return p - step_size * m / den, m, v


def bounds(p, g, m, v, lr, beta1, beta2, eps, wd, step):
    """-> (bound on |dp|, on |dm|, on |dv|) per element, float64, for the state (p, g, m, v) BEFORE the step."""
    lr, beta1, beta2, eps, wd, step_size, bc2_sqrt = _scalars(lr, beta1, beta2, eps, wd, step)
    p, g, m, v = (t.double() for t in (p, g, m, v))
    v1 = beta2 * v + (1.0 - beta2) * g * g
    den = v1.sqrt() / bc2_sqrt + eps
    mg = m.abs() + g.abs()
    return (8.0 * U * (p.abs() + step_size * mg / den) + FLT_MIN, 4.0 * U * mg + FLT_MIN, 4.0 * U * (v + g * g) + FLT_MIN)


def worst_ratios(got, ref, bnd):
    """(p, m, v) triples of what a step gave, the reference and the bounds -> [max |d| / bound] per output; inf where `got` is not finite."""
    out = []
    for a, r, b in zip(got, ref, bnd):
        if a.numel() == 0:
            out.append(0.0)
            continue
        if not bool(torch.isfinite(a).all()):
            out.append(float("inf"))
            continue
        out.append(float(((a.double() - r).abs() / b).max()))
    return out


def adversarial_state(n, seed, device="cpu"):
    """-> (p, g, m, v) float32 [n] on `device` (drawn on the CPU: the same values everywhere).
    p ~ N(0, 1), every 7th exactly 1 (LayerNorm weights), every 11th exactly 0; g of random sign and log-uniform magnitude over
    1e-12 .. 1e2, every 13th exactly 0, every 17th 1e-20 (g^2 denormal); m = N(0, 1) |g| and v = U(0, 2) g^2, every 5th of both 0 (fresh
    state), every 19th m and every 23rd v of order 1 (moments unrelated to the gradient)."""
    gen = torch.Generator().manual_seed(seed)
    i = torch.arange(n)
    rn = lambda: torch.randn(n, generator=gen, dtype=torch.float64)
    ru = lambda: torch.rand(n, generator=gen, dtype=torch.float64)
    p = rn()
    p[i % 7 == 0] = 1.0
    p[i % 11 == 0] = 0.0
    g = torch.where(ru() < 0.5, -1.0, 1.0) * 10.0 ** (-12.0 + 14.0 * ru())
    g[i % 13 == 0] = 0.0
    g[i % 17 == 0] = 1e-20
    m = rn() * g.abs()
    v = 2.0 * ru() * g * g
    m19, v23 = rn(), 2.0 * ru()
    m = torch.where(i % 19 == 0, m19, m)
    v = torch.where(i % 23 == 0, v23, v)
    m[i % 5 == 0] = 0.0
    v[i % 5 == 0] = 0.0
    return tuple(t.float().to(device) for t in (p, g, m, v))
