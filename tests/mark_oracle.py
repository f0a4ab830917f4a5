"""Oracles of the histone-mark coalitions (cf_mark_coalitions, model.mark_coalitions / mark_shapley / mark_epistasis), on the CPU in
any dtype.

  * gone_words / mark_rows / oracle_mark_coalitions: the rule of include/chromoformer_hip.h evaluated with torch on a batch dict.
    Player p is (marks_p, regions_p); for coalition word m (bit p set: present) and region rho, gone(rho) is the OR of marks_p over
    the absent players whose regions_p has bit rho; every element of region rho whose mark is in gone(rho) becomes
    tests.scan_oracle.rule(u, s) = log1p(s expm1(u)), at every resolution and in every row.  Logits by orc.forward on those rows.
  * batch_from_scaled_regions: the definition itself.  The dataset's _load is patched so that the samples of the chosen marks are
    multiplied by s over the WHOLE raw region, which is then binned by the dataset's own code (as scan_oracle.batch_from_scaled_raw
    does for a window).  It never forms a bin mean: the identity between the two is what the tests check."""
import numpy as np
import torch

from oracle import chromoformer_oracle as orc
from tests import scan_oracle as so


def gone_words(marks, regions, m, T):
    """-> [T] ints: gone(rho) for coalition word m."""
    out = [0] * T
    for p, (pm, pr) in enumerate(zip(marks, regions)):
        if not int(m) >> p & 1:
            for rho in range(T):
                if int(pr) >> rho & 1:
                    out[rho] |= int(pm)
    return out


def mark_rows(batch, players, keep, scale=0.0, dtype=torch.float32):
    """-> the batch dict of the B * n_coal rows, gene-major.  players: (marks, regions) words (attribution.mark_players)."""
    marks, regions = players[0], players[1]
    bins = list(batch["promoter_feats"])
    B = batch["interaction_freq"].shape[0]
    S = batch["pcre_feats"][bins[0]].shape[1]
    F = batch["promoter_feats"][bins[0]].shape[-1]
    keep = [int(m) for m in keep]
    nc = len(keep)

    def rep(t):
        t = t.to(dtype) if t.is_floating_point() else t
        return t[:, None].expand(B, nc, *t.shape[1:]).reshape(B * nc, *t.shape[1:]).clone()

    rows = {k: ({b: rep(t) for b, t in v.items()} if isinstance(v, dict) else rep(v)) for k, v in batch.items() if k in so.KEYS}
    for b in bins:
        L = batch["promoter_feats"][b].shape[-2]
        pf = rows["promoter_feats"][b].reshape(B, nc, L, F)
        cf = rows["pcre_feats"][b].reshape(B, nc, S, L, F)
        for c, m in enumerate(keep):
            gone = gone_words(marks, regions, m, S + 1)
            for f in range(F):
                if gone[0] >> f & 1:
                    pf[:, c, :, f] = so.rule(pf[:, c, :, f], scale)
                for j in range(S):
                    if gone[1 + j] >> f & 1:
                        cf[:, c, j, :, f] = so.rule(cf[:, c, j, :, f], scale)
        rows["promoter_feats"][b] = pf.reshape(B * nc, 1, L, F)
        rows["pcre_feats"][b] = cf.reshape(B * nc, S, L, F)
    return rows


def oracle_mark_coalitions(P, batch, players, keep, scale=0.0, cfg=None, dtype=torch.float32):
    """-> logits [B, n_coal, n_out] of mark_rows(batch, players, keep, scale) by orc.forward in `dtype`."""
    rows = mark_rows(batch, players, keep, scale, dtype)
    Pd = {k: v.detach().to(dtype) for k, v in P.items()}
    B = batch["interaction_freq"].shape[0]
    with torch.no_grad():
        lg = orc.forward(Pd, rows, cfg)
    return lg.reshape(B, -1, lg.shape[-1])


def batch_from_scaled_regions(ds, gene_ids, gone, scale, dtype=torch.float32):
    """The model's inputs of `gene_ids` binned by the dataset's own code from raw regions in which the samples of the marks of
    gone[rho] (a word per region: 0 the promoter, 1 + j pCRE slot j) are multiplied by `scale` over the whole region -> batch dict."""
    F, S = ds.n_feats, ds.i_max
    items = [ds[ds.target_genes.index(gid)] for gid in gene_ids]                               # masks, frequencies (fp32 loader)
    regs = []
    keep = ds._load
    try:
        for gid in gene_ids:
            chrom, tss, _ = ds.genes[gid]["tss"]
            slots = {(chrom, tss - 20000, tss + 20000): 0}
            slots.update({tuple(p): 1 + s for s, p in enumerate(ds.genes[gid]["pcres"])})

            def load(chrom, start, end, slots=slots):
                a = np.load("%s/%s:%d-%d.npy" % (ds.npy_dir, chrom, start, end)).astype(np.float64)
                marks = [f for f in range(F) if int(gone[slots[chrom, start, end]]) >> f & 1]
                if marks:
                    a[marks] *= scale
                return torch.from_numpy(a).to(dtype)

            ds._load = load
            regs.append(ds.regions(gid, dtype=dtype))
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
    return batch
