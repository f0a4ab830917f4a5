"""The referee of the AdamW tests refereed (tests/adamw_reference.py), no GPU: torch.optim.AdamW in float32 lies inside the bounds of
the float64 reference on the adversarial state, and ten wrong optimisers evaluated in float64 -- rounding is not what is caught --
each leave them.  So the bounds admit an honest fp32 AdamW and nothing else the list below can think of."""
import math

import pytest
import torch

from tests.adamw_reference import HYPER_SETS, adversarial_state, bounds, f32, reference, worst_ratios

N = 1 << 16


@pytest.fixture(scope="module")
def state():
    return adversarial_state(N, 1234)


def test_adversarial_state_has_its_edge_cases(state):
    p, g, m, v = state
    i = torch.arange(N)
    assert all(t.dtype == torch.float32 and bool(torch.isfinite(t).all()) for t in state)
    assert bool((p[(i % 7 == 0) & (i % 11 != 0)] == 1).all()) and bool((p[i % 11 == 0] == 0).all())
    assert bool((g[(i % 13 == 0) & (i % 17 != 0)] == 0).all()) and bool((g[i % 17 == 0] == 1e-20).all())
    assert bool((m[i % 5 == 0] == 0).all()) and bool((v[i % 5 == 0] == 0).all()) and bool((v >= 0).all())
    sq = g[i % 17 == 0] * g[i % 17 == 0]
    assert bool((sq < torch.finfo(torch.float32).tiny).all())          # g^2 is denormal (or flushed)
    mag = g.abs()[g != 0]
    assert mag.min() < 1e-11 and mag.max() > 10.0
    far = (i % 19 == 0) & (i % 5 != 0)
    assert (m[far].abs() > 1e3 * g[far].abs()).float().mean() > 0.5     # moments unrelated to the gradient


def _torch_adamw(state, hp):
    """One step of torch.optim.AdamW(foreach=False) in float32 from the given state at step - 1, on the hyper-parameters as the library's
    ABI delivers them (rounded to float32)."""
    p, g, m, v = (t.clone() for t in state)
    lr, b1, b2, eps, wd, step = hp
    par = torch.nn.Parameter(p)
    opt = torch.optim.AdamW([par], lr=f32(lr), betas=(f32(b1), f32(b2)), eps=f32(eps), weight_decay=f32(wd), foreach=False)
    opt.state[par] = {"step": torch.tensor(float(step - 1)), "exp_avg": m, "exp_avg_sq": v}
    par.grad = g
    opt.step()
    st = opt.state[par]
    assert float(st["step"]) == step
    return par.detach(), st["exp_avg"], st["exp_avg_sq"]


@pytest.mark.parametrize("hp", HYPER_SETS, ids=[str(h) for h in HYPER_SETS])
def test_torch_adamw_in_fp32_lies_inside_the_bounds(state, hp):
    got = _torch_adamw(state, hp)
    worst = worst_ratios(got, reference(*state, *hp), bounds(*state, *hp))
    print("torch.optim.AdamW fp32 %s: worst |d| / bound  p %.3f  m %.3f  v %.3f" % (hp, *worst))
    assert max(worst) <= 1.0, (hp, worst)


def _mutant(kind, p, g, m, v, lr, b1, b2, eps, wd, step):
    """A wrong AdamW in float64 on the float32-rounded hyper-parameters; kind None: the right one."""
    lr, b1, b2, eps, wd = (f32(x) for x in (lr, b1, b2, eps, wd))
    p, g, m, v = (t.double() for t in (p, g, m, v))
    if kind == "step_off_by_one":
        step = step + 1
    if kind == "beta2_0.99":
        assert abs(b2 - 0.999) < 1e-6
        b2 = f32(0.99)
    if kind == "decay_in_gradient":
        g = g + wd * p
    elif kind == "decay_halved":
        p = p * (1.0 - 0.5 * lr * wd)
    elif kind != "decay_after_step":
        p = p * (1.0 - lr * wd)
    m1 = (1.0 - b1) * m + b1 * g if kind == "one_minus_beta1_on_m" else b1 * m + (1.0 - b1) * g
    v1 = b2 * v + (1.0 - b2) * (g.abs() if kind == "g_for_g_squared" else g * g)
    bc1 = 1.0 if kind == "no_bias_correction1" else 1.0 - b1 ** step
    bc2_sqrt = 1.0 if kind == "no_bias_correction2" else math.sqrt(1.0 - b2 ** step)
    den = (v1 + eps).sqrt() / bc2_sqrt if kind == "eps_inside_sqrt" else v1.sqrt() / bc2_sqrt + eps
    p1 = p - lr / bc1 * m1 / den
    if kind == "decay_after_step":
        p1 = p1 * (1.0 - lr * wd)
    return p1, m1, v1


MUTANTS = ("decay_halved", "decay_after_step", "decay_in_gradient", "eps_inside_sqrt", "no_bias_correction2", "no_bias_correction1",
           "step_off_by_one", "beta2_0.99", "one_minus_beta1_on_m", "g_for_g_squared")


def test_the_unmutated_formula_is_the_reference(state):
    for hp in HYPER_SETS:
        for a, b in zip(_mutant(None, *state, *hp), reference(*state, *hp)):
            assert torch.equal(a, b), hp


@pytest.mark.parametrize("kind", MUTANTS)
def test_every_wrong_optimiser_leaves_the_bounds(state, kind):
    killed = []
    for hp in HYPER_SETS:
        if kind == "beta2_0.99" and hp[2] != 0.999:
            continue
        worst = worst_ratios(_mutant(kind, *state, *hp), reference(*state, *hp), bounds(*state, *hp))
        if max(worst) > 1.0:
            killed.append((hp, ["%.3g" % w for w in worst]))
    print("mutant %s: outside the bounds on %d of %d sets: %s" % (kind, len(killed), len(HYPER_SETS), killed))
    assert killed, kind
