"""Oracles of the histone-mark coalitions against a donor cell type (cf_mark_donor_coalitions, model.mark_donor_coalitions /
mark_donor_shapley / mark_donor_epistasis), on the CPU in any dtype.

  * donor_dataset: a second "cell type" for a tests.scan_oracle.scan_dataset directory: the same regions, other signals.
  * donor_rows / oracle_donor_coalitions: the rule of include/chromoformer_hip.h evaluated with torch on two batch dicts.  Players,
    words and gone(rho) are those of tests.mark_oracle; every element of region rho whose mark is in gone(rho) is COPIED from the
    donor's batch, at every resolution and in every row.  Logits by orc.forward on those rows.
  * batch_from_replaced_regions: the definition itself.  The dataset's _load is patched so that the rows of the chosen marks of a raw
    region come from the donor's file of the same name, which is then binned by the dataset's own code.  Binning works per mark, so
    the two agree bit for bit: that identity is what the tests check."""
import os
import shutil

import numpy as np
import torch

from oracle import chromoformer_oracle as orc
from tests import mark_oracle as mo
from tests import scan_oracle as so

DONOR_SEED = 5


def donor_dataset(src_dir, out_dir, seed=DONOR_SEED, w_prom=39000):
    """For every region .npy of `src_dir` (a scan_oracle.scan_dataset directory) a file of the same name and shape in `out_dir`: fp16,
    non-negative counts drawn per file from (seed, the file's rank by name), every mark of every region different from the source
    somewhere; meta.csv copied -> ChromoformerDataset on out_dir at `w_prom`."""
    import pandas as pd

    from chromoformer_amd.data import ChromoformerDataset
    os.makedirs(out_dir, exist_ok=True)
    names = sorted(n for n in os.listdir(src_dir) if n.endswith(".npy"))
    assert names
    for rank, name in enumerate(names):
        a = np.load(os.path.join(src_dir, name))
        rng = np.random.default_rng([int(seed), rank])
        level = rng.uniform(0.5, 6.0, size=(a.shape[0], 1))
        base = np.abs(np.cumsum(rng.normal(0, 0.05, size=a.shape), axis=1)) * level
        d = rng.poisson(base).astype(np.float16)
        d[:, rng.random(a.shape[1]) < 0.2] = 0
        for f in range(a.shape[0]):      # (never needed with these seeds; the assertion below is the check)
            if np.array_equal(d[f], a[f]):
                d[f, 0] = a[f, 0] + np.float16(1)
        assert d.shape == a.shape and d.dtype == np.float16 and (d >= 0).all() and np.isfinite(d).all()
        assert all((d[f] != a[f]).any() for f in range(a.shape[0])), name
        np.save(os.path.join(out_dir, name), d)
    shutil.copy(os.path.join(src_dir, "meta.csv"), os.path.join(out_dir, "meta.csv"))
    meta = os.path.join(out_dir, "meta.csv")
    return ChromoformerDataset(meta, out_dir, pd.read_csv(meta).gene_id.tolist(), w_prom=w_prom)


def donor_rows(batch, donor, players, keep, dtype=torch.float32):
    """-> the batch dict of the B * n_coal rows, gene-major.  players: (marks, regions) words (attribution.mark_players); donor: a
    batch dict whose promoter_feats / pcre_feats are read (the rest is ignored)."""
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
        dp = donor["promoter_feats"][b].to(dtype).reshape(B, L, F)
        dc = donor["pcre_feats"][b].to(dtype).reshape(B, S, L, F)
        for c, m in enumerate(keep):
            gone = mo.gone_words(marks, regions, m, S + 1)
            for f in range(F):
                if gone[0] >> f & 1:
                    pf[:, c, :, f] = dp[:, :, f]
                for j in range(S):
                    if gone[1 + j] >> f & 1:
                        cf[:, c, j, :, f] = dc[:, j, :, f]
        rows["promoter_feats"][b] = pf.reshape(B * nc, 1, L, F)
        rows["pcre_feats"][b] = cf.reshape(B * nc, S, L, F)
    return rows


def oracle_donor_coalitions(P, batch, donor, players, keep, cfg=None, dtype=torch.float32):
    """-> logits [B, n_coal, n_out] of donor_rows(batch, donor, players, keep) by orc.forward in `dtype`."""
    rows = donor_rows(batch, donor, players, keep, dtype)
    Pd = {k: v.detach().to(dtype) for k, v in P.items()}
    B = batch["interaction_freq"].shape[0]
    with torch.no_grad():
        lg = orc.forward(Pd, rows, cfg)
    return lg.reshape(B, -1, lg.shape[-1])


def batch_from_replaced_regions(ds, donor_dir, gene_ids, gone, dtype=torch.float32):
    """The model's inputs of `gene_ids` binned by the dataset's own code from raw regions in which the rows of the marks of gone[rho]
    (a word per region: 0 the promoter, 1 + j pCRE slot j) are those of the file of the same name in `donor_dir` -> batch dict."""
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
                name = "%s:%d-%d.npy" % (chrom, start, end)
                a = np.load(os.path.join(ds.npy_dir, name)).copy()
                marks = [f for f in range(F) if int(gone[slots[chrom, start, end]]) >> f & 1]
                if marks:
                    d = np.load(os.path.join(donor_dir, name))
                    assert d.shape == a.shape and d.dtype == a.dtype
                    a[marks] = d[marks]
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
