"""Oracles of integrated gradients in raw-signal space (cf_integrated_gradients_raw, attribution.raw_integrated_gradients), on the CPU
with orc.forward and torch autograd, in any dtype.

  * oracle_ig_signal: the tensor level.  The features are u = log(1 + m); the path is a * m from m = 0.  Per node the leaf is the bin
    mean a_k * m itself, the features log1p(leaf), and autograd runs back to the leaf:
        attr = m * sum_k d(w_k logits[:, t]) / d(a_k m)       coeff = (1 + m) * the same sum
    interaction_freq, when named, takes the straight path of tests/ig_oracle.py from its baseline.
  * oracle_ig_from_raw: the definition itself.  Per node the leaf is the raw signal a_k * x of every region of a gene, binned by
    chromoformer_amd.data.bin_log1p + centred (the dataset's own code), autograd back to the raw leaf, then x * sum_k grad_k.  It
    never forms a bin mean: the identity between the two is what the tests check."""
import numpy as np
import torch

from oracle import chromoformer_oracle as orc

FEATS = ("promoter_feats", "pcre_feats")


def oracle_ig_signal(P, batch, alphas, weights, target, inputs=FEATS, freq_baseline=None, cfg=None, dtype=torch.float32):
    """-> (attr, coeff, logits_x, logits_b, delta).  attr mirrors `inputs` ({binsize: tensor} for the features, a tensor for
    interaction_freq), coeff the feature inputs among them; delta [B] = sum(attr) - (F(x) - F(base))[:, target]."""
    P = {k: v.detach().to(dtype) for k, v in P.items()}
    bins = list(batch["promoter_feats"])

    def cast(t):
        return t.to(dtype) if t.is_floating_point() else t

    b0 = {k: ({b: cast(t) for b, t in v.items()} if isinstance(v, dict) else cast(v)) for k, v in batch.items()}
    feats = [k for k in FEATS if k in inputs]
    mean = {k: {b: torch.expm1(b0[k][b]) for b in bins} for k in feats}
    with_freq = "interaction_freq" in inputs
    if with_freq:
        fx = b0["interaction_freq"]
        fb = torch.zeros_like(fx) if freq_baseline is None else cast(freq_baseline).expand_as(fx)
    base = dict(b0, **{k: {b: torch.zeros_like(b0[k][b]) for b in bins} for k in feats})
    if with_freq:
        base["interaction_freq"] = fb
    with torch.no_grad():
        lx = orc.forward(P, b0, cfg)
        lb = orc.forward(P, base, cfg)
    acc = {k: {b: torch.zeros_like(mean[k][b]) for b in bins} for k in feats}
    facc = torch.zeros_like(fx) if with_freq else None
    for a, w in zip(alphas, weights):
        a, w = float(a), float(w)
        leaves = {k: {b: (a * mean[k][b]).detach().requires_grad_(True) for b in bins} for k in feats}
        cur = dict(b0, **{k: {b: torch.log1p(leaves[k][b]) for b in bins} for k in feats})
        if with_freq:
            fl = (fb + a * (fx - fb)).detach().requires_grad_(True)
            cur["interaction_freq"] = fl
        (orc.forward(P, cur, cfg)[:, target] * w).sum().backward()
        for k in feats:
            for b in bins:
                acc[k][b] = acc[k][b] + leaves[k][b].grad
        if with_freq:
            facc = facc + fl.grad
    attr = {k: {b: mean[k][b] * acc[k][b] for b in bins} for k in feats}
    coeff = {k: {b: (1 + mean[k][b]) * acc[k][b] for b in bins} for k in feats}
    B = lx.shape[0]
    total = torch.zeros(B, dtype=dtype)
    for k in feats:
        for b in bins:
            total = total + attr[k][b].reshape(B, -1).sum(1)
    if with_freq:
        attr["interaction_freq"] = (fx - fb) * facc
        total = total + attr["interaction_freq"].reshape(B, -1).sum(1)
    return attr, coeff, lx, lb, total - (lx[:, target] - lb[:, target])


def batch_from_raw(ds, gene_ids, dtype, scale=1.0, grad=False):
    """The model's inputs of `gene_ids` binned from the raw .npy regions times `scale` in `dtype`, by the dataset's own bin_log1p +
    centred -> (batch, raw), raw[(gene, slot)] the [F, len] leaf (slot -1: the promoter file) -- one leaf per (gene, region), so a
    region two genes share gets each gene's own gradient.  Follows _oracle_raw_grads of tests/test_raw_gradients_gpu.py."""
    F, S = ds.n_feats, ds.i_max
    items = [ds[ds.target_genes.index(g)] for g in gene_ids]                               # masks, frequencies (fp32 loader)
    raw, regs = {}, []
    keep = ds._load
    try:
        for g in gene_ids:
            chrom, tss, _ = ds.genes[g]["tss"]
            slots = {(chrom, tss - 20000, tss + 20000): -1}
            slots.update({tuple(p): s for s, p in enumerate(ds.genes[g]["pcres"])})

            def load(chrom, start, end, g=g, slots=slots):
                key = (g, slots[chrom, start, end])
                if key not in raw:
                    a = np.load("%s/%s:%d-%d.npy" % (ds.npy_dir, chrom, start, end))
                    raw[key] = (scale * torch.from_numpy(a.astype(np.float64))).to(dtype).requires_grad_(grad)
                return raw[key]

            ds._load = load
            regs.append(ds.regions(g, dtype=dtype))
    finally:
        ds._load = keep
    batch = {k: {} for k in ("promoter_feats", "promoter_pad_masks", "pcre_feats", "pcre_pad_masks", "interaction_masks")}
    for b in ds.binsizes:
        L = ds.w_max // b
        pfs, cfs = [], []
        for reg in regs:
            p, _, _, pcs = reg[b]
            pfs.append(p.t().unsqueeze(0))
            cfs.append(torch.stack([x.t() for x, _, _ in pcs] + [torch.zeros(L, F, dtype=dtype)] * (S - len(pcs))))
        batch["promoter_feats"][b], batch["pcre_feats"][b] = torch.stack(pfs), torch.stack(cfs)
        for k in ("promoter_pad_masks", "pcre_pad_masks", "interaction_masks"):
            batch[k][b] = torch.stack([it[k][b] for it in items])
    batch["interaction_freq"] = torch.stack([it["interaction_freq"] for it in items]).to(dtype)
    return batch, raw


def oracle_ig_from_raw(ds, P, gene_ids, alphas, weights, target, dtype=torch.float32):
    """-> (tracks, logits_x, logits_b): tracks[(gene, slot)] = x * sum_k d(w_k logits[gene, target]) / d(a_k x), [F, len] over the whole
    region file (the samples outside the window the dataset bins get exact zeros)."""
    Pd = {k: v.detach().to(dtype) for k, v in P.items()}
    with torch.no_grad():
        bx, x = batch_from_raw(ds, gene_ids, dtype)
        lx = orc.forward(Pd, bx, None)
        lb = orc.forward(Pd, batch_from_raw(ds, gene_ids, dtype, scale=0.0)[0], None)
    acc = {k: torch.zeros_like(v) for k, v in x.items()}
    for a, w in zip(alphas, weights):
        bk, leaves = batch_from_raw(ds, gene_ids, dtype, scale=float(a), grad=True)
        (orc.forward(Pd, bk, None)[:, target] * float(w)).sum().backward()
        for k in acc:
            acc[k] = acc[k] + leaves[k].grad
    return {k: x[k] * acc[k] for k in acc}, lx, lb
