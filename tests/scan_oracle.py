"""Oracles of the in-silico perturbation scan (cf_perturbation_scan, model.perturbation_scan), on the CPU in any dtype.

  * scan_rows / oracle_scan: the rule of include/chromoformer_hip.h evaluated with torch on a batch dict.  Per region and resolution
    the centre pad-mask row gives the first real row q and the count n (holes inside count); genomic bin j is row q + j, mirrored
    q + n - 1 - j; window g of width w covers the coarse genomic bins [g, min(g + w, n_c)) and R_r times those at resolution r, clipped
    to n_r; covered features of the set's marks become log1p(s * expm1(u)).  Logits by orc.forward on the perturbed rows.
  * batch_from_scaled_raw: the definition itself.  The dataset's _load is patched so that the window's samples of the set's marks are
    multiplied by s in the RAW region, which is then binned by the dataset's own code (as tests/raw_ig_oracle.batch_from_raw does).  It
    never forms a bin mean: the identity between the two is what the tests check."""
import numpy as np
import torch

from oracle import chromoformer_oracle as orc

KEYS = ("promoter_feats", "promoter_pad_masks", "pcre_feats", "pcre_pad_masks", "interaction_masks", "interaction_freq")


def default_mark_sets(n_feats=7):
    return [(f,) for f in range(n_feats)] + [tuple(range(n_feats))]


def centre_row(mask, lead, L):
    """The centre query row [lead, L] (bool) of a pad mask: the reference's [.., 1, L, L] tensor or a compact [.., L] row array."""
    m = torch.as_tensor(mask).bool()
    if m.numel() == lead * L * L:
        return m.reshape(lead, L, L)[:, L // 2]
    return m.reshape(lead, L)


def extent(row):
    """-> (first unmasked row, count up to the last unmasked row) of a bool mask row; (0, 0) if every row is masked."""
    real = torch.nonzero(~row).flatten()
    if not real.numel():
        return 0, 0
    return int(real[0]), int(real[-1] - real[0] + 1)


def covered_rows(q, n, n_c, R, g, width, flip):
    """Rows of a region at a resolution with R bins per coarse bin that window g covers -> (first, one past the last)."""
    if g >= n_c:
        return 0, 0
    j0, j1 = g * R, min(min(g + width, n_c) * R, n)
    if j0 >= j1:
        return 0, 0
    return (q + n - j1, q + n - j0) if flip else (q + j0, q + j1)


def rule(u, scale):
    """log1p(s expm1(u)) in the dtype of u, each operation rounded."""
    return torch.log1p(scale * torch.expm1(u))


def scan_rows(batch, region=0, scale=0.0, width=1, mark_sets=None, flip=None, dtype=torch.float32, variants=None):
    """-> (feats {binsize: [B, nv, L, F]}, rows): the scanned region's features per (gene, variant) and the batch dict of the B * nv
    rows, gene-major.  variants: the v to evaluate (default: all V = 1 + n_sets * W)."""
    bins = list(batch["promoter_feats"])
    n_bins = {b: batch["promoter_feats"][b].shape[-2] for b in bins}
    F = batch["promoter_feats"][bins[0]].shape[-1]
    B = batch["interaction_freq"].shape[0]
    S = batch["pcre_feats"][bins[0]].shape[1]
    bc = min(bins, key=lambda b: n_bins[b])
    W = n_bins[bc]
    mark_sets = default_mark_sets(F) if mark_sets is None else [tuple(ms) for ms in mark_sets]
    variants = list(range(1 + len(mark_sets) * W)) if variants is None else list(variants)
    flip = [False] * B if flip is None else [bool(f) for f in flip]
    nv = len(variants)

    def rows_of(b):
        L = n_bins[b]
        if region == 0:
            return centre_row(batch["promoter_pad_masks"][b], B, L)
        return centre_row(batch["pcre_pad_masks"][b], B * S, L).reshape(B, S, L)[:, region - 1]

    feats = {}
    for b in bins:
        L = n_bins[b]
        src = (batch["promoter_feats"][b].reshape(B, L, F) if region == 0 else batch["pcre_feats"][b].reshape(B, S, L, F)[:, region - 1]).to(dtype)
        out = src[:, None].repeat(1, nv, 1, 1)
        mr, mc = rows_of(b), rows_of(bc)
        for i in range(B):
            q, n = extent(mr[i])
            _, n_c = extent(mc[i])
            for k, v in enumerate(variants):
                if v == 0:
                    continue
                ms, g = mark_sets[(v - 1) // W], (v - 1) % W
                lo, hi = covered_rows(q, n, n_c, L // W, g, width, flip[i])
                for f in set(ms):
                    out[i, k, lo:hi, f] = rule(src[i, lo:hi, f], scale)
        feats[b] = out

    def rep(t):
        t = t.to(dtype) if t.is_floating_point() else t
        return t[:, None].expand(B, nv, *t.shape[1:]).reshape(B * nv, *t.shape[1:]).clone()

    rows = {k: ({b: rep(t) for b, t in v.items()} if isinstance(v, dict) else rep(v)) for k, v in batch.items() if k in KEYS}
    for b in bins:
        L = n_bins[b]
        if region == 0:
            rows["promoter_feats"][b] = feats[b].reshape(B * nv, 1, L, F).clone()
        else:
            rows["pcre_feats"][b].reshape(B * nv, S, L, F)[:, region - 1] = feats[b].reshape(B * nv, L, F)
    return feats, rows


def oracle_scan(P, batch, cfg=None, dtype=torch.float32, **kw):
    """-> (logits [B, nv, n_out], feats) of scan_rows(batch, **kw) by orc.forward in `dtype`."""
    feats, rows = scan_rows(batch, dtype=dtype, **kw)
    Pd = {k: v.detach().to(dtype) for k, v in P.items()}
    B = batch["interaction_freq"].shape[0]
    with torch.no_grad():
        lg = orc.forward(Pd, rows, cfg)
    return lg.reshape(B, -1, lg.shape[-1]), feats


def batch_from_scaled_raw(ds, gene_ids, region, g, width, marks, scale, dtype=torch.float32):
    """The model's inputs of `gene_ids` binned by the dataset's own code from raw regions in which window g (of `width` coarsest bins)
    of `region` (0 the promoter, 1 + j pCRE slot j) has the samples of `marks` multiplied by `scale` -> batch dict.  A gene without
    that region is left as it is."""
    F, S = ds.n_feats, ds.i_max
    bc = max(int(b) for b in ds.binsizes)
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
                if slots[chrom, start, end] == region:
                    col0 = 20000 - ds.w_prom // 2 if region == 0 else 0
                    ncols = ds.w_prom if region == 0 else a.shape[1]
                    lo, hi = col0 + g * bc, col0 + min((g + width) * bc, ncols)
                    if lo < hi:
                        a[list(marks), lo:hi] *= scale
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


def dataset_batch(ds, gene_ids, dtype=torch.float32):
    """The unperturbed inputs of `gene_ids` (batch_from_scaled_raw with nothing scaled)."""
    return batch_from_scaled_raw(ds, gene_ids, -1, 0, 1, (), 1.0, dtype)


def scan_dataset(out_dir, w_prom=39000):
    """A 20-gene synthetic dataset (tests.synth_data, seed 11: both strands, pCRE lengths that are multiples of neither 2,000 nor 500,
    genes without partners) read with the promoter narrowed to `w_prom` -> ChromoformerDataset."""
    import pandas as pd

    from chromoformer_amd.data import ChromoformerDataset
    from tests.synth_data import make_dataset
    meta = make_dataset(out_dir, n_genes=20, seed=11)
    table = pd.read_csv(meta)
    return ChromoformerDataset(meta, out_dir, table.gene_id.tolist(), w_prom=w_prom)
