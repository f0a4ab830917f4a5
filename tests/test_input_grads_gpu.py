"""Gradients with respect to the float inputs (cf_backward_from_inputs): `x.grad` of promoter_feats[b], pcre_feats[b] and
interaction_freq after `model(...)[:, k].sum().backward()`, as the reference's autograd gives them (saliency maps).

  * oracle parity at bsz 8 in the realistic regime (padded promoters, dummy pCREs, masked interactions), judged by an fp64
    referee as in test_parity_holes_gpu.py, with exact zeros where the oracle has them;
  * the reference's own input gradients (tests/golden/input_grads.npz);
  * no side effects: logits and parameter gradients bit-identical with and without input gradients, each input alone equal to all
    together, run to run bit-identical;
  * a non-default Regulation shape (layer-by-layer k_attr), a non-default trunk width, embed.n_layers = 2 refused by name;
  * every element of every requested output written (NaN-prefilled buffers at the C ABI);
  * at bsz 64, sum_j dfeat_j f_j^T = W^T . lin_proj.weight.grad per resolution (ties the new outputs to the checked weight gradients)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import chromoformer_oracle as orc
from tests.helpers import GOLDEN, load_npz_batch

pytestmark = pytest.mark.gpu
BINS = (2000, 500, 100)
ALL = ("promoter_feats", "pcre_feats", "interaction_freq")


def _batch(B, seed, cfg=None):
    """Realistic regime plus promoter padding: the tail fifth of the bins of every other promoter is masked (centre bin kept)."""
    b = orc.synthetic_batch(B, cfg=cfg, seed=seed, regime="realistic")
    for bs, m in b["promoter_pad_masks"].items():
        L = m.shape[-1]
        m[0::2, ..., L - max(1, L // 5):] = True
    return b


def _params(cfg, regression, seed=42):
    P = orc.init_params(cfg, seed, regression)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for v in P.values():
            v.add_(0.02 * torch.randn(v.shape, generator=g))
    return P


def _model(cfg, regression, P, B):
    from chromoformer_amd import ChromoformerClassifier, ChromoformerRegressor
    cfg = orc._cfg(cfg)
    Model = ChromoformerRegressor if regression else ChromoformerClassifier
    m = Model(cfg["n_feats"], cfg["d_emb"], cfg["d_head"], cfg["embed"], cfg["pairwise_interaction"], cfg["regulation"],
              binsizes=cfg["binsizes"], seed=42, i_max=cfg["i_max"], w_max=cfg["w_max"], max_batch=B).cuda(0)
    m.load_state_dict(P)
    return m


def _leaves(batch, want, device, dtype=torch.float32):
    pf = {b: t.to(device, dtype).clone().requires_grad_("promoter_feats" in want) for b, t in batch["promoter_feats"].items()}
    cf = {b: t.to(device, dtype).clone().requires_grad_("pcre_feats" in want) for b, t in batch["pcre_feats"].items()}
    fr = batch["interaction_freq"].to(device, dtype).clone().requires_grad_("interaction_freq" in want)
    return pf, cf, fr


def _grads(pf, cf, fr):
    out = {}
    for b in pf:
        out["promoter_feats.%d" % b] = None if pf[b].grad is None else pf[b].grad.detach().cpu().clone()
        out["pcre_feats.%d" % b] = None if cf[b].grad is None else cf[b].grad.detach().cpu().clone()
    out["interaction_freq"] = None if fr.grad is None else fr.grad.detach().cpu().clone()
    return out


def _hip(model, batch, col, want=ALL, device="cuda"):
    pf, cf, fr = _leaves(batch, want, device)
    for p in model.parameters():
        p.grad = None
    logits = model(pf, batch["promoter_pad_masks"], cf, batch["pcre_pad_masks"], batch["interaction_masks"], fr)
    logits[:, col].sum().backward()
    torch.cuda.synchronize()
    pg = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters() if p.grad is not None}
    return logits.detach().cpu().clone(), _grads(pf, cf, fr), pg


def _oracle(P, batch, cfg, col, dtype):
    Pd = {k: v.detach().to(dtype) for k, v in P.items()}
    pf, cf, fr = _leaves(batch, ALL, "cpu", dtype)
    b2 = dict(batch, promoter_feats=pf, pcre_feats=cf, interaction_freq=fr)
    orc.forward(Pd, b2, cfg)[:, col].sum().backward()
    return _grads(pf, cf, fr)


def _check_referee(gh, g32, g64):
    for k, ref in g64.items():
        n = ref.norm().item()
        err_h, err_32 = (gh[k].double() - ref).norm().item(), (g32[k].double() - ref).norm().item()
        assert err_h <= max(2 * err_32, 2e-5 * n) + 1e-12, (k, err_h / max(n, 1e-30), err_32 / max(n, 1e-30))
        zero = g32[k] == 0
        assert bool((gh[k][zero] == 0).all()), (k, "non-zero where the oracle has exact zeros", int((gh[k][zero] != 0).sum()))


@pytest.mark.parametrize("regression", [False, True], ids=["classifier", "regressor"])
def test_input_grads_match_the_oracle_default_config(regression):
    B, col = 8, 0 if regression else 1
    batch = _batch(B, 77)
    masked = torch.stack([batch["interaction_masks"][b].view(B, 9, 9) for b in BINS]).all(0)
    assert bool(masked[:, 1:].all(-1).any()), "the batch must hold fully masked interaction rows"
    P = _params(None, regression)
    _, gh, _ = _hip(_model(None, regression, P, B), batch, col)
    _check_referee(gh, _oracle(P, batch, None, col, torch.float32), _oracle(P, batch, None, col, torch.float64))
    # dummy pCRE slots and masked interaction entries: exact zeros
    dummy = batch["pcre_pad_masks"][100][:, :, 0, 200].all(-1)
    assert bool(dummy.any())
    for b in BINS:
        assert bool((gh["pcre_feats.%d" % b][dummy] == 0).all())
    assert bool((gh["interaction_freq"][masked] == 0).all())


@pytest.mark.parametrize("regression", [False, True], ids=["classifier", "regressor"])
def test_input_grads_match_the_reference_golden(regression):
    z = np.load(GOLDEN + "/input_grads.npz")
    kat, _ = load_npz_batch("kat.npz")
    real = orc.synthetic_batch(8, seed=31, regime="realistic")
    head, col = ("reg", 0) if regression else ("clf", 1)
    for tag, batch in (("kat", kat), ("real", real)):
        gene = int(z["%s.gene" % tag])
        model = _model(None, regression, orc.init_params(None, 42, regression), 8)
        _, gh, _ = _hip(model, batch, col, device="cpu")      # CPU leaves: the gradient comes back through .to()
        for k, v in gh.items():
            ref = torch.from_numpy(z["%s.%s.grad.%s" % (tag, head, k)])
            got = v[gene]
            assert got.shape == ref.shape
            assert (got - ref).norm().item() <= 1e-4 * ref.norm().item() + 1e-7, (tag, k)


def test_no_side_effects_and_determinism():
    B = 8
    batch = _batch(B, 91)
    P = _params(None, False)
    model = _model(None, False, P, B)
    l0, g0, p0 = _hip(model, batch, 1, want=())
    assert all(v is None for v in g0.values())
    l1, g1, p1 = _hip(model, batch, 1)
    l2, g2, p2 = _hip(model, batch, 1)
    assert torch.equal(l0, l1) and set(p0) == set(p1)
    assert all(torch.equal(p0[k], p1[k]) for k in p0), "parameter gradients change when input gradients are requested"
    assert all(torch.equal(g1[k], g2[k]) for k in g1) and all(torch.equal(p1[k], p2[k]) for k in p1), "not run-to-run identical"
    for one in ALL:
        _, g, p = _hip(model, batch, 1, want=(one,))
        assert all(torch.equal(p0[k], p[k]) for k in p0)
        for k, v in g.items():
            if k.startswith(one):
                assert torch.equal(v, g1[k]), k
            else:
                assert v is None, k


_REG4 = dict(regulation=dict(n_layers=3, n_heads=4, d_model=256, d_ff=256))
_DEMB64 = dict(d_emb=64, embed=dict(n_layers=1, n_heads=1, d_model=64, d_ff=128), pairwise_interaction=dict(n_layers=3, n_heads=2, d_model=64, d_ff=256))


@pytest.mark.parametrize("name,variant", [("reg_4_heads", _REG4), ("d_emb_64_embed_1_head", _DEMB64)])
def test_input_grads_away_from_the_default_shapes(name, variant):
    B = 5
    cfg = orc._cfg(variant)
    batch = _batch(B, 13, cfg)
    P = _params(cfg, False, seed=3)
    _, gh, _ = _hip(_model(cfg, False, P, B), batch, 1)
    _check_referee(gh, _oracle(P, batch, cfg, 1, torch.float32), _oracle(P, batch, cfg, 1, torch.float64))


def test_embed_all_rows_path_is_refused_by_name():
    cfg = orc._cfg(dict(embed=dict(n_layers=2, n_heads=2, d_model=128, d_ff=128)))
    B = 3
    batch = _batch(B, 5, cfg)
    model = _model(cfg, False, orc.init_params(cfg, 42, False), B)
    with pytest.raises(RuntimeError, match="promoter_feats.*embed.n_layers"):
        _hip(model, batch, 1)


def test_every_requested_element_is_written():
    from chromoformer_amd import _lib
    B = 8
    batch = _batch(B, 17)
    model = _model(None, False, _params(None, False), B)
    bs, keep = model.pack_batch(batch)
    model._run_forward(bs, save=True)
    want = _lib.cf_input_grads()
    outs = []
    for r, b in enumerate(BINS):
        outs.append(torch.full(batch["promoter_feats"][b].shape, float("nan"), device="cuda"))
        want.promoter_feats[r] = outs[-1].data_ptr()
        outs.append(torch.full(batch["pcre_feats"][b].shape, float("nan"), device="cuda"))
        want.pcre_feats[r] = outs[-1].data_ptr()
    outs.append(torch.full(batch["interaction_freq"].shape, float("nan"), device="cuda"))
    want.interaction_freq = outs[-1].data_ptr()
    dl = torch.ones(B, 2, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.lib().cf_backward_from_inputs(model._handle, C.byref(bs), dl.data_ptr(), C.byref(want), st), "cf_backward_from_inputs")
    torch.cuda.synchronize()
    for o in outs:
        assert not bool(torch.isnan(o).any())


def test_feature_gradients_contract_to_the_weight_gradients_at_bsz64():
    B = 64
    batch = orc.synthetic_batch(B, seed=2024, regime="dense")
    P = _params(None, False)
    model = _model(None, False, P, B)
    _, gh, pg = _hip(model, batch, 1)
    for b in BINS:
        for name, key in (("promoter_feats", "embed.%d.lin_proj.weight" % b), ("pcre_feats", "pairwise_interaction.%d.lin_proj_pcre.weight" % b)):
            f = batch[name][b].double().reshape(-1, 7)
            d = gh["%s.%d" % (name, b)].double().reshape(-1, 7)
            lhs = d.t() @ f
            rhs = P[key].double().t() @ pg[key].double()
            assert (lhs - rhs).norm().item() <= 1e-4 * rhs.norm().item() + 1e-9, (name, b)
