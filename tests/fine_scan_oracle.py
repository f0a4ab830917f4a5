"""Oracles of the fine-resolution perturbation scan (cf_perturbation_scan_fine, model.perturbation_scan_fine), on the CPU.

  * fine_rows / oracle_fine: the rule of include/chromoformer_hip.h evaluated with torch on a batch dict, on scan_oracle's extent and
    rule.  f = the resolution with the smallest bin size; bin j of resolution r has the finest children K_j = [j R, min((j + 1) R, n_f)),
    R = n_bins[f] / n_bins[r], and cnt_j = sum of cnt_k (b_f each, the last real finest bin len - (n_f - 1) b_f with `lengths`).  For a
    window [lo, hi) of finest genomic bins and C = K_j n [lo, hi): C empty keeps the bits; C = K_j is the scan's log1p(s expm1(u));
    otherwise S = sum_{k in C} cnt_k expm1(u_k) in fp64, ascending k, m' = (dtype)(expm1(u_j) + (s - 1) S / cnt_j), u' = log1p(m').
  * region_from_scaled_raw: the definition itself.  The samples of the window are multiplied by s in the RAW region, which is then
    binned by oracle/dataset_oracle.region.  It never reads a stored feature: the identity between the two is what the tests check."""
import numpy as np
import torch

from oracle import chromoformer_oracle as orc
from oracle import dataset_oracle as dso
from tests import scan_oracle as so

NONE, WHOLE, PART = 0, 1, 2      # how a window covers a bin


def fine_windows(start, width, stride, n_windows, Lf):
    """-> [(lo, hi)] of one gene: window g covers [start + g stride, start + g stride + width), clipped to the Lf finest bins."""
    return [(min(start + g * stride, Lf), min(start + g * stride + width, Lf)) for g in range(n_windows)]


def fine_region(src, masks, binsizes, lo, hi, marks, scale, flip=False, length=None, dtype=torch.float32):
    """The rule on ONE region: src {binsize: [L, F]}, masks {binsize: [L] bool centre pad-mask row}, the window [lo, hi) in finest
    genomic bins -> (feats {binsize: [L, F]} in `dtype`, kinds {binsize: [L] of NONE / WHOLE / PART})."""
    bf = min(binsizes)
    qf, nf = so.extent(masks[bf])
    Lf = src[bf].shape[0]
    lo, hi = min(lo, nf), min(hi, nf)
    cnt = torch.full((max(nf, 1),), float(bf), dtype=torch.float64)
    if length is not None and nf:
        cnt[nf - 1] = length - (nf - 1) * bf
        assert 1 <= cnt[nf - 1] <= bf, (length, nf, bf)
    uf = src[bf].to(dtype)
    frow = (lambda k: qf + nf - 1 - k) if flip else (lambda k: qf + k)
    feats, kinds = {}, {}
    for b in binsizes:
        u = src[b].to(dtype)
        L = u.shape[0]
        out, kind = u.clone(), torch.zeros(L, dtype=torch.int8)
        q, n = so.extent(masks[b])
        R = Lf // L
        for j in range(lo // R, min(-(-hi // R), n)) if lo < hi else ():
            K0, K1 = j * R, min((j + 1) * R, nf)
            k0, k1 = max(lo, K0), min(hi, K1)
            row = q + n - 1 - j if flip else q + j
            if (k0, k1) == (K0, K1):
                kind[row] = WHOLE
                for f in set(marks):
                    out[row, f] = so.rule(u[row, f], scale)
                continue
            kind[row] = PART
            for f in set(marks):
                S = torch.zeros((), dtype=torch.float64)
                for k in range(k0, k1):                                      # ascending genomic k, each product and sum rounded in fp64
                    S = S + cnt[k] * torch.expm1(uf[frow(k), f]).double()
                m = (torch.expm1(u[row, f]).double() + (float(np.float32(scale)) - 1.0) * S / cnt[K0:K1].sum()).to(dtype)
                out[row, f] = torch.log1p(m)
        feats[b], kinds[b] = out, kind
    return feats, kinds


def fine_rows(batch, region=0, scale=0.0, width=1, stride=None, start=0, n_windows=None, mark_sets=None, lengths=None, flip=None,
              dtype=torch.float32, variants=None):
    """-> (feats {binsize: [B, nv, L, F]}, rows, kinds {binsize: [B, nv, L]}): the scanned region's features per (gene, variant), the
    batch dict of the B * nv rows (gene-major), and how each row is covered.  variants: the v to evaluate (default: all V = 1 +
    n_sets * n_windows)."""
    bins = list(batch["promoter_feats"])
    n_bins = {b: batch["promoter_feats"][b].shape[-2] for b in bins}
    F = batch["promoter_feats"][bins[0]].shape[-1]
    B = batch["interaction_freq"].shape[0]
    S = batch["pcre_feats"][bins[0]].shape[1]
    Lf = n_bins[min(bins)]
    stride = width if stride is None else stride
    start = [int(start)] * B if np.ndim(start) == 0 else [int(x) for x in start]
    n_windows = max(-(-(Lf - min(start)) // stride), 1) if n_windows is None else n_windows
    mark_sets = so.default_mark_sets(F) if mark_sets is None else [tuple(ms) for ms in mark_sets]
    variants = list(range(1 + len(mark_sets) * n_windows)) if variants is None else list(variants)
    flip = [False] * B if flip is None else [bool(f) for f in flip]
    nv = len(variants)
    feats = {b: torch.empty(B, nv, n_bins[b], F, dtype=dtype) for b in bins}
    kinds = {b: torch.zeros(B, nv, n_bins[b], dtype=torch.int8) for b in bins}
    for i in range(B):
        src, masks = {}, {}
        for b in bins:
            L = n_bins[b]
            if region == 0:
                src[b], masks[b] = batch["promoter_feats"][b].reshape(B, L, F)[i], so.centre_row(batch["promoter_pad_masks"][b], B, L)[i]
            else:
                src[b] = batch["pcre_feats"][b].reshape(B, S, L, F)[i, region - 1]
                masks[b] = so.centre_row(batch["pcre_pad_masks"][b], B * S, L).reshape(B, S, L)[i, region - 1]
        wins = fine_windows(start[i], width, stride, n_windows, Lf)
        for k, v in enumerate(variants):
            ms, (lo, hi) = ((), (0, 0)) if v == 0 else (mark_sets[(v - 1) // n_windows], wins[(v - 1) % n_windows])
            f, kd = fine_region(src, masks, bins, lo, hi, ms, scale, flip[i], None if lengths is None else int(lengths[i]), dtype)
            for b in bins:
                feats[b][i, k], kinds[b][i, k] = f[b], kd[b]

    def rep(t):
        t = t.to(dtype) if t.is_floating_point() else t
        return t[:, None].expand(B, nv, *t.shape[1:]).reshape(B * nv, *t.shape[1:]).clone()

    rows = {k: ({b: rep(t) for b, t in v.items()} if isinstance(v, dict) else rep(v)) for k, v in batch.items() if k in so.KEYS}
    for b in bins:
        L = n_bins[b]
        if region == 0:
            rows["promoter_feats"][b] = feats[b].reshape(B * nv, 1, L, F).clone()
        else:
            rows["pcre_feats"][b].reshape(B * nv, S, L, F)[:, region - 1] = feats[b].reshape(B * nv, L, F)
    return feats, rows, kinds


def oracle_fine(P, batch, cfg=None, dtype=torch.float32, **kw):
    """-> (logits [B, nv, n_out], feats, kinds) of fine_rows(batch, **kw) by orc.forward in `dtype`."""
    feats, rows, kinds = fine_rows(batch, dtype=dtype, **kw)
    Pd = {k: v.detach().to(dtype) for k, v in P.items()}
    B = batch["interaction_freq"].shape[0]
    with torch.no_grad():
        lg = orc.forward(Pd, rows, cfg)
    return lg.reshape(B, -1, lg.shape[-1]), feats, kinds


def region_from_scaled_raw(raw, binsizes, n_bins, lo, hi, marks, scale, strand="+", window=None):
    """The definition: the raw samples of the finest genomic bins [lo, hi) of `marks` multiplied by `scale` (fp32), then
    oracle/dataset_oracle.region -> {binsize: [L, F]}.  window: the promoter's width (its samples are the centre `window` of the file)."""
    bf = min(binsizes)
    col0, ncols = (0, raw.shape[1]) if window is None else (20000 - window // 2, window)
    x = np.asarray(raw).astype(np.float32)
    a, b = col0 + min(lo * bf, ncols), col0 + min(hi * bf, ncols)
    if a < b and len(marks):
        x[sorted(set(marks)), a:b] *= np.float32(scale)
    return {bs: dso.region(x, bs, L, strand, window)[0].t() for bs, L in zip(binsizes, n_bins)}


def partial_bound_factor(src, feats, kinds):
    """(1 + m_j) / (1 + m') of every element -> tensor like feats (1 where the row is not partly covered): the factor of the bound
    c 2^-24 (1 + m_j) / (1 + m') on a partly covered element."""
    r = torch.exp(src.double() - feats.double())
    return torch.where((kinds == PART)[..., None].expand_as(r), r, torch.ones_like(r))
