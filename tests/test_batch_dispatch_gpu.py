"""The kernel choices that follow from the number of genes in a batch, against the fp64 referee (cases: tests/batch_dispatch_cases.py).

Off the fused trunk the centre-row attention launch takes 1, 2, 4 or 8 regions per workgroup from N = B * i_max (k_attc1, k_attc2<., 2 / 4 / 8>,
forward and backward), a last workgroup with fewer regions than that runs guards of its own, and the weight-gradient tiles reduce
9B / 8B / B rows in stages of 32 with a partial last stage.  The other gradient tests sit at B <= 8 (one region per workgroup) or B = 64
(eight, no ragged tail, whole stages).  Here: two, four and eight regions per workgroup with and without a ragged last workgroup whose
regions are live (S1-S3, R1-R3), and the fused trunk at 1, 2, 17 and 33 genes (F*).

  * every case reaches the kernel it names (cf_attc_regions, launch counts);
  * logits, loss and all parameter gradients by helpers.assert_within_referee, unchanged;
  * per region -- one wrong region cannot hide in a tensor's norm -- the Pairwise output rows and d logits / d pcre_feats;
  * no dependence on max_batch or on a larger batch that ran before on the handle: bit-equal to a fresh handle;
  * the optimiser schedules (graph, fused AdamW, riders) bit-equal to the separate launches at 17 and 33 genes.

Measured on an MI355X, worst err(HIP) / err(fp32 oracle) against the fp64 oracle.  The bound is 2; per tensor the floors of
assert_within_referee (2e-5 of a tensor's norm) stand beside it, which is where the ratios above 2 come from -- gamma_f and fc_head.2.bias
gradients that both sides have to 1e-6 of their norm.  Forward launches: 4 on the fused trunk at every B, 11 (S*, R3) and 13 (R1, R2) off it.

  case   per tensor (worst tensor)                      per region: forward rows   d pcre_feats
  S1     3.04  regulation.100...layers.3...gamma_f      1.69                       1.27
  S2     1.80  fc_head.2.bias                           1.13                       1.22
  S3     3.14  regulation.500...layers.5...gamma_f      1.10                       1.15
  R1     1.98  regulation.500...layers.1...gamma_f      1.14                       1.11
  R2     2.48  regulation.500...layers.3...gamma_f      1.21                       1.84
  R3     1.50  regulation.100...layers.1...gamma_f      0.99                       1.17
  F1     3.68  fc_head.2.bias                           0.93                       1.18
  F2     2.13  regulation.500...layers.0...gamma_f      1.38                       1.04
  F17    1.97  fc_head.2.bias                           0.90                       1.30
  F33    1.89  regulation.2000...layers.0...gamma_f     0.77                       1.04

In absolute terms every live region's forward rows are within 2.1e-6 entry-wise (fp32 oracle: 1.7e-6) and every live [L, F] block of
d pcre_feats within 2.3e-6 of its norm (fp32 oracle: 3.2e-6).  All pairs of the max_batch test are bit-equal to a fresh handle, and all
schedules of the optimiser test bit-equal to the separate launches.  S3 runs on another seed than the rest: with seed 2024 one ReLU gate of
its batch sits within fp32 rounding of zero (batch_dispatch_cases.py has the figures)."""
import contextlib
import functools
import os

import pytest
import torch

from oracle import chromoformer_oracle as orc
from tests import batch_dispatch_cases as bd
from tests import helpers

pytestmark = pytest.mark.gpu
ALL = sorted(bd.CASES)


@contextlib.contextmanager
def _env(env):
    """Switches the library reads when a model is constructed (CF_TRUNK)."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _build(name, max_batch):
    c = bd.CASES[name]
    with _env(c.env):
        model = helpers.build_model(c.cfg, False, max_batch=max_batch)
        model.load_state_dict(bd.params(name))
    return model


@functools.lru_cache(maxsize=None)
def _model(name):
    return _build(name, bd.CASES[name].B)


def _forward_backward(model, batch):
    """helpers.referee_hip on a model that exists -> (logits, loss, {name: gradient}) on the CPU."""
    logits, loss = model.forward_backward(model.pack_batch(batch), batch["label"])
    torch.cuda.synchronize()
    model._publish_grads()
    return logits.cpu().clone(), float(loss), {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters() if p.grad is not None}


def _call(model, b, pcre_feats=None):
    return model(b["promoter_feats"], b["promoter_pad_masks"], pcre_feats or b["pcre_feats"], b["pcre_pad_masks"], b["interaction_masks"],
                 b["interaction_freq"])


def _forward_launches(model, b):
    with torch.no_grad():
        _call(model, b)
        _call(model, b)      # (the second pass: nothing that only the first pass after a bind does)
    torch.cuda.synchronize()
    return model.launch_counts()[0]


@functools.lru_cache(maxsize=None)
def _fused_forward_launches():
    return _forward_launches(_build("F2", 2), bd.batch("F2"))


@pytest.mark.parametrize("name", ALL)
def test_case_reaches_the_kernel_it_names(name):
    from chromoformer_amd import _lib
    c, S = bd.CASES[name], bd.config(name)["i_max"]
    model = _model(name)
    L = _lib.lib()
    n = _forward_launches(model, bd.batch(name))
    print("%s: %d forward launches (fused trunk, default configuration: %d)" % (name, n, _fused_forward_launches()))
    assert L.cf_attc_regions(model._handle, c.B) == 1
    if c.fused:      # one trunk launch whatever B is
        assert n == _fused_forward_launches()
        return
    assert L.cf_attc_regions(model._handle, c.B * S) == c.ag
    assert n > _fused_forward_launches()      # the stand-alone kernels: a chain of launches per layer


@pytest.mark.parametrize("name", ALL)
def test_all_gradients_against_the_fp64_referee(name):
    c = bd.CASES[name]
    b = bd.batch(name)
    with _env(c.env):
        got = helpers.referee_hip(functools.partial(helpers.build_model, c.cfg, False), b, bd.params(name))
    worst = helpers.assert_within_referee(got, bd.referee(name, torch.float32), bd.referee(name, torch.float64))
    print("%s: worst err(HIP) / err(fp32 oracle) against the fp64 referee: %.2f (%s)" % ((name,) + worst))


@pytest.mark.parametrize("name", ALL)
def test_every_live_region_forward_and_backward(name):
    c, cfg = bd.CASES[name], bd.config(name)
    b = bd.batch(name)
    S, T, d = cfg["i_max"], cfg["i_max"] + 1, cfg["d_emb"]
    model = _model(name)
    for p in model.parameters():
        p.grad = None
    cf = {bs: t.cuda().clone().requires_grad_(True) for bs, t in b["pcre_feats"].items()}
    logits = _call(model, b, cf)
    rows = {bs: model.debug_buffer("R%d.x0" % r).cpu().view(-1, T, d)[: c.B, 1:].clone() for r, bs in enumerate(cfg["binsizes"])}
    logits[:, 1].sum().backward()      # cf_backward_from_inputs: the attention backward with the batch's own regions per workgroup
    torch.cuda.synchronize()
    grads = {bs: t.grad.detach().cpu() for bs, t in cf.items()}
    assert (logits.detach().cpu().double() - bd.referee(name, torch.float64)[0]).abs().max().item() < 1e-4
    try:
        wf = bd.check_regions_forward(name, rows)
    finally:
        lv, r32, r64 = bd.live_slots(b), bd.regions(name, torch.float32), bd.regions(name, torch.float64)
        for bs in rows:      # the figures, whether or not a bound holds
            print("%s %d: forward rows err %.2e (fp32 oracle %.2e), d pcre_feats err %.2e (fp32 oracle %.2e)" % (
                name, bs, bd._forward_err(rows[bs], r64[0][bs], lv).max().item(), bd._forward_err(r32[0][bs], r64[0][bs], lv).max().item(),
                bd._backward_err(grads[bs], r64[1][bs], lv).max().item(), bd._backward_err(r32[1][bs], r64[1][bs], lv).max().item()))
    wb = bd.check_regions_backward(name, grads)
    print("%s: worst live region, err(HIP) / err(fp32 oracle): forward rows %.2f, d pcre_feats %.2f" % (name, wf, wb))


@pytest.mark.parametrize("first,second", [("R2", "R1"), ("S3", "S1"), ("F33", "F2")])
def test_no_dependence_on_max_batch_or_on_what_ran_before(first, second):
    """Every launch shape derives from B, not from max_batch, and no reduction reads rows a larger batch left behind: the second batch on
    a handle sized for (and used by) the first gives the bits of a fresh handle of its own size."""
    assert bd.CASES[first].cfg is bd.CASES[second].cfg and bd.CASES[first].env == bd.CASES[second].env
    model = _build(first, bd.CASES[first].B)
    _forward_backward(model, bd.batch(first))
    got = _forward_backward(model, bd.batch(second))
    fresh = _forward_backward(_build(second, bd.CASES[second].B), bd.batch(second))
    helpers.assert_within_referee(got, bd.referee(second, torch.float32), bd.referee(second, torch.float64))
    assert torch.equal(got[0], fresh[0]) and got[1] == fresh[1], (got[1], fresh[1], (got[0] - fresh[0]).abs().max().item())
    assert got[2].keys() == fresh[2].keys()
    for k in fresh[2]:
        assert torch.equal(got[2][k], fresh[2][k]), (k, (got[2][k] - fresh[2][k]).abs().max().item())


@pytest.mark.parametrize("B", [17, 33])
def test_optimiser_schedules_are_bit_equal_at_middle_batch_sizes(B):
    """test_config_variants_gpu.py::test_fused_optimiser_and_riders_equal_the_separate_launches at 17 and 33 genes, default configuration:
    the per-wave tiles of the riders, the tiles with the AdamW epilogue and the plain reduction side by side where the reduction spans
    several stages of 32 rows with a partial last one (M = 9B, 8B, B = 153 / 136 / 17 and 297 / 264 / 33)."""
    from chromoformer_amd import ChromoformerClassifier
    from chromoformer_amd.engine import Trainer
    batches = [orc.synthetic_batch(B, seed=21 + i, regime="realistic") for i in range(2)]

    def run(**kw):
        model = ChromoformerClassifier(seed=3, max_batch=B).cuda(0)
        tr = Trainer(model, lr=1e-3, **kw)
        slots = [tr.stage(b) for b in batches]
        losses = []
        for i in range(3):
            _, loss = tr.step(slots[i % 2])
            with torch.cuda.stream(tr.stream):
                losses.append(loss.clone())
        torch.cuda.synchronize()
        sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        sd["<exp_avg>"], sd["<exp_avg_sq>"] = model._mflat.cpu().clone(), model._vflat.cpu().clone()
        return sd, [float(x) for x in losses], tr

    ref, ref_loss, _ = run(use_graph=False, merge_opt=False)
    for kw in (dict(use_graph=True), dict(use_graph=False, rider_tiles=37), dict(use_graph=True, rider_tiles=100000), dict(use_graph=True, rider_tiles=0)):
        got, loss, tr = run(**kw)
        assert tr.fuse_opt, kw
        assert (tr.rider_tiles > 0) == (kw.get("rider_tiles", 512) > 0), (kw, tr.rider_tiles)      # the riders did ride where asked to
        assert loss == ref_loss, (B, kw)
        for k in ref:
            assert torch.equal(ref[k], got[k]), (B, kw, k)
