"""Oracles of the window game (cf_mark_window_coalitions, model.mark_window_*), on the CPU in any dtype.

  * gone_table: gone(rho, g) of include/chromoformer_hip.h in plain Python -- the OR of marks_p over the absent players with bit rho in
    regions_p and lo_p <= g < hi_p.
  * edited_batch: the batch dict a coalition's row reads, by torch edits built from tests/scan_oracle.py's extent, covered_rows and rule:
    per region, resolution and coarse bin g with gone(rho, g) != 0 the rows window g (width 1) covers, the marks of the word scaled, or
    taken from the donor.
  * player builders restated without chromoformer_amd.attribution, and batch_from_edited_raw: the definition itself -- the dataset's
    _load patched so that, inside the windows of the absent players, the samples of their marks are multiplied by s (or replaced by the
    donor's raw samples) in the RAW region, which the dataset's own code then bins."""
import numpy as np
import torch

from tests import scan_oracle as so


def windows(W, width):
    return [(g, min(g + width, W)) for g in range(0, W, width)]


def players_promoter(F, W, width=1):
    return [(tuple(range(F)), (0,), w) for w in windows(W, width)]


def players_promoter_cells(F, W, width=1):
    return [((f,), (0,), w) for w in windows(W, width) for f in range(F)]


def players_regions(F, S, W, width=1):
    return [(tuple(range(F)), (rho,), w) for rho in range(S + 1) for w in windows(W, width)]


def full_word(P):
    return (1 << P) - 1


def gone_table(players, word, T, W):
    """players: (marks, regions, (lo, hi)) triples of index iterables; word: a Python int, bit p set = player p present ->
    [[set of marks gone in region rho at coarse bin g] for g] for rho]."""
    table = [[set() for _ in range(W)] for _ in range(T)]
    for p, (ms, rs, (lo, hi)) in enumerate(players):
        if word >> p & 1:
            continue
        for rho in rs:
            for g in range(lo, hi):
                table[rho][g] |= set(ms)
    return table


def edited_batch(batch, players, word, scale=0.0, donor=None, flip=None, dtype=torch.float32):
    """The batch with coalition `word` of `players` applied -> batch dict (feature tensors are new, the rest is shared).  donor: a batch
    dict whose features an absent player's elements take (None: the scale rule)."""
    bins = list(batch["promoter_feats"])
    n_bins = {b: batch["promoter_feats"][b].shape[-2] for b in bins}
    F = batch["promoter_feats"][bins[0]].shape[-1]
    B = batch["interaction_freq"].shape[0]
    S = batch["pcre_feats"][bins[0]].shape[1]
    bc = min(bins, key=lambda b: n_bins[b])
    W = n_bins[bc]
    flip = [False] * B if flip is None else [bool(f) for f in flip]
    table = gone_table(players, word, S + 1, W)
    out = dict(batch)
    out["promoter_feats"], out["pcre_feats"] = {}, {}
    for b in bins:
        L = n_bins[b]
        pf = batch["promoter_feats"][b].to(dtype).clone()
        cf = batch["pcre_feats"][b].to(dtype).clone()
        pv, cv = pf.view(B, L, F), cf.view(B, S, L, F)
        if donor is not None:
            dpv, dcv = donor["promoter_feats"][b].to(dtype).reshape(B, L, F), donor["pcre_feats"][b].to(dtype).reshape(B, S, L, F)
        pm, pmc = so.centre_row(batch["promoter_pad_masks"][b], B, L), so.centre_row(batch["promoter_pad_masks"][bc], B, W)
        cm = so.centre_row(batch["pcre_pad_masks"][b], B * S, L).reshape(B, S, L)
        cmc = so.centre_row(batch["pcre_pad_masks"][bc], B * S, W).reshape(B, S, W)
        for i in range(B):
            for rho in range(S + 1):
                q, n = so.extent(pm[i] if rho == 0 else cm[i, rho - 1])
                _, n_c = so.extent(pmc[i] if rho == 0 else cmc[i, rho - 1])
                dst = pv[i] if rho == 0 else cv[i, rho - 1]
                for g in range(W):
                    if not table[rho][g]:
                        continue
                    r0, r1 = so.covered_rows(q, n, n_c, L // W, g, 1, flip[i] and rho == 0)
                    for f in table[rho][g]:
                        if donor is None:
                            dst[r0:r1, f] = so.rule(dst[r0:r1, f], scale)
                        else:
                            dst[r0:r1, f] = (dpv[i] if rho == 0 else dcv[i, rho - 1])[r0:r1, f]
        out["promoter_feats"][b], out["pcre_feats"][b] = pf, cf
    return out


def batch_from_edited_raw(ds, gene_ids, players, word, scale=0.0, donor_dir=None, dtype=torch.float32):
    """The model's inputs of `gene_ids` binned by the dataset's own code from raw regions in which, inside the windows of the absent
    players of `word`, the samples of their marks are multiplied by `scale` -- or, with `donor_dir`, replaced by the samples of the
    file of the same name there -> batch dict.  Each sample is edited once however many absent players cover it."""
    F, S = ds.n_feats, ds.i_max
    bc = max(int(b) for b in ds.binsizes)
    W = ds.w_max // bc
    table = gone_table(players, word, S + 1, W)
    items = [ds[ds.target_genes.index(gid)] for gid in gene_ids]
    regs = []
    keep = ds._load
    try:
        for gid in gene_ids:
            chrom, tss, _ = ds.genes[gid]["tss"]
            slots = {(chrom, tss - 20000, tss + 20000): 0}
            slots.update({tuple(p): 1 + s for s, p in enumerate(ds.genes[gid]["pcres"])})

            def load(chrom, start, end, slots=slots):
                name = "%s:%d-%d.npy" % (chrom, start, end)
                a = np.load("%s/%s" % (ds.npy_dir, name)).astype(np.float64)
                d = np.load("%s/%s" % (donor_dir, name)).astype(np.float64) if donor_dir is not None else None
                rho = slots[chrom, start, end]
                col0 = 20000 - ds.w_prom // 2 if rho == 0 else 0
                ncols = ds.w_prom if rho == 0 else a.shape[1]
                if rho <= S:
                    for g in range(W):
                        lo, hi = col0 + g * bc, col0 + min((g + 1) * bc, ncols)
                        if table[rho][g] and lo < hi:
                            ms = sorted(table[rho][g])
                            if d is None:
                                a[ms, lo:hi] *= scale
                            else:
                                a[ms, lo:hi] = d[ms, lo:hi]
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
