"""The oracle of integrated gradients (ChromoformerBase.integrated_gradients): the contract's definition run with orc.forward and
torch autograd on the CPU, one backward per quadrature node.  Used by the IG tests and by tests/golden/make_ig_goldens.py.

    x_k  = xb + a_k (x - xb)            g_k = d(w_k logits[:, t]) / d x_k
    attr = (x - xb) * sum_k g_k         delta = sum(attr) - (F(x)[t] - F(xb)[t])     per gene
"""
import torch

from oracle import chromoformer_oracle as orc

KEYS = ("promoter_feats", "pcre_feats", "interaction_freq")


def oracle_ig(P, batch, alphas, weights, target, inputs=KEYS, baselines=None, cfg=None, dtype=torch.float32):
    """-> (attr, logits_x, logits_b, delta): attr mirrors the inputs ({binsize: tensor} for the features, a tensor for the
    frequencies), the rest [B, n_out], [B, n_out], [B].  dtype float64 runs the whole definition (parameters included) in fp64."""
    P = {k: v.detach().to(dtype) for k, v in P.items()}
    bins = list(batch["promoter_feats"])

    def cast(t):
        return t.to(dtype) if t.is_floating_point() else t

    b0 = {k: ({b: cast(t) for b, t in v.items()} if isinstance(v, dict) else cast(v)) for k, v in batch.items()}
    base = {}
    for key in inputs:
        x = b0[key]
        given = None if baselines is None else baselines.get(key)
        if isinstance(x, dict):
            base[key] = {b: (torch.zeros_like(x[b]) if given is None else cast(given[b]).expand_as(x[b])) for b in bins}
        else:
            base[key] = torch.zeros_like(x) if given is None else cast(given).expand_as(x)

    def run(vals, grad):
        b2 = dict(b0)
        leaves = {}
        for key in inputs:
            if isinstance(vals[key], dict):
                leaves[key] = {b: vals[key][b].detach().clone().requires_grad_(grad) for b in bins}
            else:
                leaves[key] = vals[key].detach().clone().requires_grad_(grad)
            b2[key] = leaves[key]
        return orc.forward(P, b2, cfg), leaves

    with torch.no_grad():
        lx = orc.forward(P, b0, cfg)
        b_base = dict(b0, **base)
        lb = orc.forward(P, b_base, cfg)
    acc = None
    for a, w in zip(alphas, weights):
        a, w = float(a), float(w)
        vals = {}
        for key in inputs:
            x, xb = b0[key], base[key]
            vals[key] = {b: xb[b] + a * (x[b] - xb[b]) for b in bins} if isinstance(x, dict) else xb + a * (x - xb)
        logits, leaves = run(vals, True)
        (logits[:, target] * w).sum().backward()
        g = {key: ({b: leaves[key][b].grad for b in bins} if isinstance(leaves[key], dict) else leaves[key].grad) for key in inputs}
        if acc is None:
            acc = g
        else:
            acc = {key: ({b: acc[key][b] + g[key][b] for b in bins} if isinstance(g[key], dict) else acc[key] + g[key]) for key in inputs}
    attr = {}
    total = torch.zeros(lx.shape[0], dtype=dtype)
    for key in inputs:
        x, xb = b0[key], base[key]
        if isinstance(x, dict):
            attr[key] = {b: (x[b] - xb[b]) * acc[key][b] for b in bins}
            for b in bins:
                total = total + attr[key][b].reshape(lx.shape[0], -1).sum(1)
        else:
            attr[key] = (x - xb) * acc[key]
            total = total + attr[key].reshape(lx.shape[0], -1).sum(1)
    delta = total - (lx[:, target] - lb[:, target])
    return attr, lx, lb, delta
