"""Integrated gradients (ChromoformerBase.integrated_gradients): the quadrature table shared by the library call, its tests and users.

IG integrates the input gradient along the straight path from a baseline x' to the input x,
    attr = (x - x') * integral_0^1 dF(x' + a (x - x')) / dx da  ~  (x - x') * sum_k w_k g(x' + a_k (x - x')),
and satisfies completeness: the attributions of one gene sum to F(x) - F(x') up to the quadrature error.  The methods are Captum's
(IntegratedGradients(method=...)): Gauss-Legendre (default) and the four Riemann sums.  The trapezoid rule here is the composite one
on n equally spaced nodes including both ends (step 1 / (n - 1), half weights at the ends), so that every method's weights sum to 1.
"""
import numpy as np

METHODS = ("gausslegendre", "riemann_trapezoid", "riemann_middle", "riemann_left", "riemann_right")
INPUTS = ("promoter_feats", "pcre_feats", "interaction_freq")


def ig_quadrature64(method="gausslegendre", n_steps=50):
    """-> (alphas, weights), float64 [n_steps]: nodes and weights on [0, 1]."""
    if method not in METHODS:
        raise ValueError("integrated gradients: unknown method %r; choose from %s" % (method, METHODS))
    n = int(n_steps)
    if n != n_steps or n < 1:
        raise ValueError("integrated gradients: n_steps must be a positive integer, got %r" % (n_steps,))
    if method == "gausslegendre":
        x, w = np.polynomial.legendre.leggauss(n)
        return 0.5 * (x + 1.0), 0.5 * w
    if method == "riemann_trapezoid":
        if n < 2:
            raise ValueError("integrated gradients: riemann_trapezoid needs n_steps >= 2 (both ends of the path)")
        w = np.full(n, 1.0 / (n - 1))
        w[0] *= 0.5
        w[-1] *= 0.5
        return np.linspace(0.0, 1.0, n), w
    k = np.arange(n, dtype=np.float64)
    a = {"riemann_left": k / n, "riemann_middle": (k + 0.5) / n, "riemann_right": (k + 1.0) / n}[method]
    return a, np.full(n, 1.0 / n)


def ig_quadrature(method="gausslegendre", n_steps=50):
    """-> (alphas, weights), float32 [n_steps]: ig_quadrature64 cast to fp32 -- the table the library call uses."""
    a, w = ig_quadrature64(method, n_steps)
    return a.astype(np.float32), w.astype(np.float32)
