"""Oracles of integrated gradients in raw-signal space against a donor cell type (cf_integrated_gradients_raw_donor,
cf_bin_spread_difference, attribution.raw_integrated_gradients(donor_dataset=...)), on the CPU with orc.forward and torch autograd, in
any dtype.

  * oracle_ig_signal_donor: the tensor level, tests.raw_ig_oracle.oracle_ig_signal extended to a donor.  The features are
    u = log(1 + m) and ud = log(1 + md); per node the leaf is the bin mean md + a_k (m - md) itself, the features log1p(leaf), and
    autograd runs back to the leaf:
        attr = (m - md) * sum_k d(w_k logits[:, t]) / d(leaf_k)       cmean = the same sum
    F(xd) is the donor's features under the batch's masks and frequencies.  interaction_freq, when named, takes the straight path of
    tests/ig_oracle.py from its baseline.
  * oracle_ig_from_raw_donor: the definition itself.  Per node the leaf is the raw signal xd + a_k (x - xd) of every region of a gene
    (x from the dataset's files, xd from the donor dataset's files of the same names), binned by the dataset's own bin_log1p +
    centred, autograd back to the raw leaf, then (x - xd) * sum_k grad_k.  It never forms a bin mean.
  * spread_reference: the formula of cf_bin_spread_difference in numpy float64, with the magnitude |x - xd| sum_r |C_r| / cnt_r its
    rounding bound is stated in."""
import os

import numpy as np
import torch

from oracle import chromoformer_oracle as orc
from tests.raw_ig_oracle import FEATS


def oracle_ig_signal_donor(P, batch, donor, alphas, weights, target, inputs=FEATS, freq_baseline=None, cfg=None, dtype=torch.float32):
    """-> (attr, cmean, logits_x, logits_b, delta).  donor: a batch dict whose promoter_feats / pcre_feats are read.  attr mirrors
    `inputs`, cmean the feature inputs among them; delta [B] = sum(attr) - (F(x) - F(base))[:, target]."""
    P = {k: v.detach().to(dtype) for k, v in P.items()}
    bins = list(batch["promoter_feats"])

    def cast(t):
        return t.to(dtype) if t.is_floating_point() else t

    b0 = {k: ({b: cast(t) for b, t in v.items()} if isinstance(v, dict) else cast(v)) for k, v in batch.items()}
    feats = [k for k in FEATS if k in inputs]
    mean = {k: {b: torch.expm1(b0[k][b]) for b in bins} for k in feats}
    ud = {k: {b: cast(donor[k][b]).reshape(b0[k][b].shape) for b in bins} for k in feats}
    dmean = {k: {b: torch.expm1(ud[k][b]) for b in bins} for k in feats}
    diff = {k: {b: mean[k][b] - dmean[k][b] for b in bins} for k in feats}
    with_freq = "interaction_freq" in inputs
    if with_freq:
        fx = b0["interaction_freq"]
        fb = torch.zeros_like(fx) if freq_baseline is None else cast(freq_baseline).expand_as(fx)
    base = dict(b0, **{k: ud[k] for k in feats})
    if with_freq:
        base["interaction_freq"] = fb
    with torch.no_grad():
        lx = orc.forward(P, b0, cfg)
        lb = orc.forward(P, base, cfg)
    acc = {k: {b: torch.zeros_like(mean[k][b]) for b in bins} for k in feats}
    facc = torch.zeros_like(fx) if with_freq else None
    for a, w in zip(alphas, weights):
        a, w = float(a), float(w)
        leaves = {k: {b: (dmean[k][b] + a * diff[k][b]).detach().requires_grad_(True) for b in bins} for k in feats}
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
    attr = {k: {b: diff[k][b] * acc[k][b] for b in bins} for k in feats}
    B = lx.shape[0]
    total = torch.zeros(B, dtype=dtype)
    for k in feats:
        for b in bins:
            total = total + attr[k][b].reshape(B, -1).sum(1)
    if with_freq:
        attr["interaction_freq"] = (fx - fb) * facc
        total = total + attr["interaction_freq"].reshape(B, -1).sum(1)
    return attr, acc, lx, lb, total - (lx[:, target] - lb[:, target])


def batch_on_raw_path(ds, donor_dir, gene_ids, dtype, a=1.0, grad=False):
    """The model's inputs of `gene_ids` binned from the raw regions xd + a (x - xd) in `dtype` (x: the dataset's .npy files, xd: the
    files of the same names in `donor_dir`) by the dataset's own bin_log1p + centred, under the dataset's masks and frequencies ->
    (batch, leaves, x, xd), each keyed (gene, slot) (slot -1: the promoter file), one leaf per (gene, region).  a = 1 is the gene's
    batch, a = 0 the donor's signal under the gene's masks."""
    F, S = ds.n_feats, ds.i_max
    items = [ds[ds.target_genes.index(g)] for g in gene_ids]                               # masks, frequencies (fp32 loader)
    leaves, xs, xds, regs = {}, {}, {}, []
    keep = ds._load
    try:
        for g in gene_ids:
            chrom, tss, _ = ds.genes[g]["tss"]
            slots = {(chrom, tss - 20000, tss + 20000): -1}
            slots.update({tuple(p): s for s, p in enumerate(ds.genes[g]["pcres"])})

            def load(chrom, start, end, g=g, slots=slots):
                key = (g, slots[chrom, start, end])
                if key not in leaves:
                    name = "%s:%d-%d.npy" % (chrom, start, end)
                    x = torch.from_numpy(np.load(os.path.join(ds.npy_dir, name)).astype(np.float64)).to(dtype)
                    xd = torch.from_numpy(np.load(os.path.join(donor_dir, name)).astype(np.float64)).to(dtype)
                    assert x.shape == xd.shape
                    xs[key], xds[key] = x, xd
                    leaves[key] = (xd + float(a) * (x - xd)).requires_grad_(grad)
                return leaves[key]

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
    return batch, leaves, xs, xds


def oracle_ig_from_raw_donor(ds, donor_dir, P, gene_ids, alphas, weights, target, dtype=torch.float32):
    """-> (tracks, logits_x, logits_b): tracks[(gene, slot)] = (x - xd) * sum_k d(w_k logits[gene, target]) / d(xd + a_k (x - xd)),
    [F, len] over the whole region file (the samples outside the window the dataset bins get exact zeros)."""
    Pd = {k: v.detach().to(dtype) for k, v in P.items()}
    with torch.no_grad():
        bx, _, x, xd = batch_on_raw_path(ds, donor_dir, gene_ids, dtype, 1.0)
        lx = orc.forward(Pd, bx, None)
        lb = orc.forward(Pd, batch_on_raw_path(ds, donor_dir, gene_ids, dtype, 0.0)[0], None)
    acc = {k: torch.zeros_like(v) for k, v in x.items()}
    for a, w in zip(alphas, weights):
        bk, leaves, _, _ = batch_on_raw_path(ds, donor_dir, gene_ids, dtype, float(a), grad=True)
        (orc.forward(Pd, bk, None)[:, target] * float(w)).sum().backward()
        for k in acc:
            acc[k] = acc[k] + leaves[k].grad
    return {k: (x[k] - xd[k]) * acc[k] for k in acc}, lx, lb


def spread_reference(x, xd, col0, ncols, flip, binsizes, n_bins, cmean):
    """The formula of cf_bin_spread_difference in float64 -> (draw [F, ncols], magnitude [F, ncols]).  x, xd: [F, ld] (xd None: the zero
    signal); binsizes / n_bins / cmean ([L_r, F] arrays or None) per resolution in any order -- the sum runs coarsest first;
    magnitude = |x - xd| * sum_r |C_r| / cnt_r, the size of the partial results the fp32 roundings act on."""
    xw = np.asarray(x, dtype=np.float64)[:, col0:col0 + ncols]
    dw = np.zeros_like(xw) if xd is None else np.asarray(xd, dtype=np.float64)[:, col0:col0 + ncols]
    F = xw.shape[0]
    total, mag = np.zeros((F, ncols)), np.zeros((F, ncols))
    for r in sorted(range(len(binsizes)), key=lambda r: -binsizes[r]):
        b, L, c = int(binsizes[r]), int(n_bins[r]), cmean[r]
        if c is None:
            continue
        c = np.asarray(c, dtype=np.float64)
        n = min(-(-ncols // b), L)
        left = -(-(L - n) // 2)
        for g in range(n):
            lo, hi = g * b, min((g + 1) * b, ncols)
            p = L - 1 - (left + g) if flip else left + g
            total[:, lo:hi] += (c[p] / (hi - lo))[:, None]
            mag[:, lo:hi] += (np.abs(c[p]) / (hi - lo))[:, None]
    return (xw - dw) * total, np.abs(xw - dw) * mag
