"""Integrated gradients without a GPU: the quadrature table (chromoformer_amd.attribution.ig_quadrature), the CPU oracle of
tests/ig_oracle.py against the reference's own IG (tests/golden/integrated_gradients.npz), and the C entry point and the predict CLI
options (declared, bound, parsed, refused)."""
import os
import re

import numpy as np
import pytest
import torch

from chromoformer_amd.attribution import METHODS, ig_quadrature, ig_quadrature64
from oracle import chromoformer_oracle as orc
from tests.helpers import GOLDEN
from tests.ig_oracle import oracle_ig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINS = (2000, 500, 100)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("n", [2, 7, 50, 300])
def test_weights_sum_to_one_and_nodes_lie_in_the_interval(method, n):
    a, w = ig_quadrature(method, n)
    assert a.dtype == np.float32 and w.dtype == np.float32 and a.shape == w.shape == (n,)
    assert abs(float(w.astype(np.float64).sum()) - 1.0) <= n * 2 ** -24
    assert (a >= 0).all() and (a <= 1).all() and (w > 0).all()
    assert (np.diff(a) > 0).all()


@pytest.mark.parametrize("n", [1, 2, 5, 16, 50])
def test_gauss_legendre_integrates_polynomials_exactly(n):
    a, w = ig_quadrature64("gausslegendre", n)
    for j in range(2 * n):
        assert abs(float((w * a ** j).sum()) - 1.0 / (j + 1)) < 1e-12, j


def test_riemann_nodes():
    for method, first, last in (("riemann_left", 0.0, 0.9), ("riemann_right", 0.1, 1.0), ("riemann_middle", 0.05, 0.95),
                                ("riemann_trapezoid", 0.0, 1.0)):
        a, _ = ig_quadrature64(method, 10 if method != "riemann_trapezoid" else 11)
        assert abs(a[0] - first) < 1e-15 and abs(a[-1] - last) < 1e-15, method
    _, w = ig_quadrature64("riemann_trapezoid", 11)
    assert np.allclose(w, [0.05] + [0.1] * 9 + [0.05])


def test_bad_quadrature_requests_raise():
    with pytest.raises(ValueError, match="unknown method"):
        ig_quadrature("simpson", 10)
    for n in (0, -3, 2.5):
        with pytest.raises(ValueError, match="n_steps"):
            ig_quadrature("gausslegendre", n)
    with pytest.raises(ValueError, match="riemann_trapezoid"):
        ig_quadrature("riemann_trapezoid", 1)
    assert ig_quadrature("riemann_left", 1)[1][0] == 1.0


@pytest.mark.parametrize("regression", [False, True], ids=["classifier", "regressor"])
def test_the_oracle_reproduces_the_reference_golden(regression):
    z = np.load(os.path.join(GOLDEN, "integrated_gradients.npz"))
    head, t = ("reg", 0) if regression else ("clf", 1)
    g = int(z["gene"])
    a, w = ig_quadrature("gausslegendre", int(z["n_steps"]))
    assert np.array_equal(a, z["alphas"]) and np.array_equal(w, z["weights"])
    batch = orc.synthetic_batch(8, seed=31, regime="realistic")
    one = {k: ({b: x[g:g + 1] for b, x in v.items()} if isinstance(v, dict) else v[g:g + 1]) for k, v in batch.items()}
    attr, lx, lb, delta = oracle_ig(orc.init_params(None, 42, regression), one, a, w, t)
    for k in ["promoter_feats.%d" % b for b in BINS] + ["pcre_feats.%d" % b for b in BINS] + ["interaction_freq"]:
        key, _, b = k.partition(".")
        got = (attr[key][int(b)] if b else attr[key])[0]
        ref = torch.from_numpy(z["%s.attr.%s" % (head, k)])
        assert got.shape == ref.shape, k
        assert (got - ref).norm().item() <= 1e-4 * ref.norm().item() + 1e-9, k
    assert (lx[0] - torch.from_numpy(z["%s.logits_x" % head])).abs().max().item() < 1e-6
    assert (lb[0] - torch.from_numpy(z["%s.logits_base" % head])).abs().max().item() < 1e-6
    assert abs(delta[0].item() - float(z["%s.delta" % head])) < 1e-5
    # completeness up to the quadrature error: delta is small against F(x) - F(xb)
    assert abs(delta[0].item()) < 0.1 * abs((lx[0, t] - lb[0, t]).item())


def test_the_entry_point_is_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "chromoformer_hip.h")).read()
    assert re.search(r"int\s+cf_integrated_gradients\s*\(\s*cf_handle\s*\*\s*h\s*,\s*const\s+cf_batch\s*\*\s*batch\s*,\s*const\s+cf_ig_opts\s*\*"
                     r"\s*opts\s*,\s*const\s+cf_input_grads\s*\*\s*out\s*,", hdr)
    from chromoformer_amd import _lib
    assert "cf_integrated_gradients" in _lib.SYMBOLS
    assert [f[0] for f in _lib.cf_ig_opts._fields_] == ["n_steps", "target", "interpolate", "alphas", "weights", "base_promoter_feats",
                                                       "base_pcre_feats", "base_interaction_freq", "base_broadcast"]
    from chromoformer_amd import ChromoformerRegressor
    from chromoformer_amd.net import Chromoformer
    assert Chromoformer.integrated_gradients is ChromoformerRegressor.integrated_gradients


def _cli(*extra):
    from chromoformer_amd import predict
    return predict.main(["-m", "meta.csv", "-d", "npy", "-o", "out.csv"] + list(extra))


@pytest.mark.parametrize("extra, msg", [
    (["--ig-steps", "10"], "need --ig-dir"),
    (["--ig-target", "1"], "need --ig-dir"),
    (["--ig-method", "riemann_left"], "need --ig-dir"),
    (["--ig-dir", "d", "--ig-steps", "0"], "at least 1"),
    (["--ig-dir", "d", "--ig-steps", "1", "--ig-method", "riemann_trapezoid"], "at least 2"),
    (["--ig-dir", "d", "--ig-target", "2"], r"\[0, 2\)"),
    (["--ig-dir", "d", "--ig-target", "1", "--regression"], r"\[0, 1\)"),
    (["--ig-dir", "d", "--ig-method", "simpson"], "invalid choice"),
])
def test_cli_refuses_bad_ig_options(extra, msg, capsys):
    with pytest.raises(SystemExit) as e:
        _cli(*extra)
    assert e.value.code == 2
    assert re.search(msg, capsys.readouterr().err)


def test_cli_parses_ig_options(monkeypatch):
    from chromoformer_amd import predict
    seen = {}

    def fake(*a, **k):
        seen.update(k)
        raise RuntimeError("stop")

    monkeypatch.setattr(predict, "predict", fake)
    with pytest.raises(RuntimeError, match="stop"):
        _cli("--ig-dir", "d", "--ig-steps", "20", "--ig-method", "riemann_middle", "--ig-target", "0")
    assert (seen["ig_dir"], seen["ig_steps"], seen["ig_method"], seen["ig_target"]) == ("d", 20, "riemann_middle", 0)
    with pytest.raises(RuntimeError, match="stop"):
        _cli("--ig-dir", "d")
    assert (seen["ig_steps"], seen["ig_method"], seen["ig_target"]) == (50, "gausslegendre", None)
    with pytest.raises(RuntimeError, match="stop"):
        _cli()
    assert seen["ig_dir"] is None
