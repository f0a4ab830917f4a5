"""Shared helpers for the tests: golden loading, batch plumbing and the fp64 referee (the oracle in float64 is the truth, the fp32
oracle and the HIP path are two fp32 evaluations of it)."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import chromoformer_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BATCH_KEYS = ("promoter_feats", "promoter_pad_masks", "pcre_feats", "pcre_pad_masks", "interaction_masks")


def load_npz_batch(name):
    """-> (batch dict in the reference layout, dict of the remaining arrays)."""
    z = np.load(os.path.join(GOLDEN, name), allow_pickle=False)
    batch = {k: {} for k in BATCH_KEYS}
    extra = {}
    for key in z.files:
        head, _, tail = key.partition(".")
        if head in BATCH_KEYS:
            batch[head][int(tail)] = torch.from_numpy(z[key])
        elif key in ("interaction_freq", "label"):
            batch[key] = torch.from_numpy(z[key])
        else:
            extra[key] = z[key]
    return batch, extra


def take(batch, idx):
    return {k: ({b: t[idx] for b, t in v.items()} if isinstance(v, dict) else v[idx]) for k, v in batch.items()}


def checksum(t):
    t = t.detach().double()
    return np.array([float(t.sum()), float(t.abs().sum()), float((t * t).sum())])


def build_model(cfg=None, regression=False, max_batch=8, seed=42):
    """The HIP model of an oracle configuration on cuda:0."""
    from chromoformer_amd import ChromoformerClassifier, ChromoformerRegressor
    c = orc._cfg(cfg)
    Model = ChromoformerRegressor if regression else ChromoformerClassifier
    return Model(c["n_feats"], c["d_emb"], c["d_head"], c["embed"], c["pairwise_interaction"], c["regulation"], binsizes=c["binsizes"],
                 seed=seed, i_max=c["i_max"], w_max=c["w_max"], max_batch=max_batch).cuda(0)


def referee_hip(Model, batch, P):
    """Fused forward + loss + backward of the HIP path -> (logits, loss, {name: gradient}) on the CPU.  Model: a model class, or
    functools.partial(build_model, cfg, regression) away from the default configuration."""
    model = Model(seed=42, max_batch=batch["interaction_freq"].shape[0]).cuda(0)
    model.load_state_dict(P)
    logits, loss = model.forward_backward(model.pack_batch(batch), batch["label"])
    torch.cuda.synchronize()
    model._publish_grads()
    return logits.cpu().clone(), float(loss), {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters() if p.grad is not None}


def referee_oracle(P, batch, regression, dtype, cfg=None):
    """The oracle's forward, loss and autograd in `dtype` -> (logits, loss, {name: gradient})."""
    Pr = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in P.items()}
    b = {k: ({kk: (vv.to(dtype) if vv.is_floating_point() else vv) for kk, vv in v.items()} if isinstance(v, dict) else v) for k, v in batch.items()}
    b["interaction_freq"] = batch["interaction_freq"].to(dtype)
    logits = orc.forward(Pr, b, cfg)
    if regression:
        loss = F.mse_loss(logits, batch["label"].view(-1, 1).to(dtype))
    else:
        loss = F.cross_entropy(logits, batch["label"].long())
    loss.backward()
    return logits.detach(), loss.item(), {k: v.grad for k, v in Pr.items() if v.grad is not None and not orc.never_trained(k)}


def perturbed_params(regression=False, cfg=None, seed=42):
    P = orc.init_params(cfg, seed, regression)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for v in P.values():
            v.add_(0.02 * torch.randn(v.shape, generator=g))
    return P


def assert_within_referee(got, o32, o64):
    """The criterion of test_parity_holes_gpu.py::test_bsz64_against_an_fp64_referee for (logits, loss, gradients) triples: `got`
    is not further from the fp64 truth than twice the fp32 oracle (floors: 2e-6 in the logits, 2e-5 of a tensor's norm), within 1e-4
    in the logits and 1e-3 of every tensor's norm, over the oracle's own gradient key set.  -> (worst err / err(fp32 oracle), name)."""
    (lh, lossh, gh), (l32, loss32, g32), (l64, loss64, g64) = got, o32, o64
    e32, eh = (l32.double() - l64).abs().max().item(), (lh.double() - l64).abs().max().item()
    assert eh < 1e-4 and eh <= max(2 * e32, 2e-6), ("logits", eh, e32)
    assert abs(lossh - loss64) <= max(2 * abs(loss32 - loss64), 2e-6 * max(1.0, abs(loss64))), ("loss", lossh, loss32, loss64)
    assert set(gh) == set(g64)
    worst = (0.0, None)
    for k, ref in g64.items():
        n = ref.norm().item()
        err_h, err_32 = (gh[k].double() - ref).norm().item(), (g32[k].double() - ref).norm().item()
        assert err_h <= max(2 * err_32, 2e-5 * n) + 1e-12, (k, err_h / max(n, 1e-30), err_32 / max(n, 1e-30))
        assert err_h <= 1e-3 * n + 1e-12, (k, err_h / max(n, 1e-30))
        worst = max(worst, (err_h / max(err_32, 1e-30), k))
    return worst
