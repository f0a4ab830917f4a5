"""Reference gradients of the binning map (ChromoformerDataset._bin_and_pad + strand flip, data.py:68-113) with respect to the RAW
signal, for the tests of cf_bin_regions_multi_backward / raw_signal_gradients: the closed form in numpy fp64 and the same thing by
autograd through chromoformer_amd.data.bin_log1p + centred in any dtype.

For the window [col0, col0 + ncols) of x [F, len], bin sizes b_r with L_r output bins and dfeat_r [L_r, F] (gradient with respect
to the binned, centred, optionally mirrored features), n_r = min(ceil(ncols / b_r), L_r) real bins:
    draw[f, s] = sum_r dfeat_r[p_r(s), f] / (cnt (1 + mean))    over the bin of s at each resolution; bins past L_r contribute nothing."""
import numpy as np
import torch

from chromoformer_amd.data import bin_log1p, centred


def closed_form(x, col0, ncols, flip, binsizes, n_bins, dfeat, times_input=False):
    """-> float64 [F, ncols]."""
    xw = np.asarray(x, dtype=np.float64)[:, col0:col0 + ncols]
    out = np.zeros_like(xw)
    for b, L, d in zip(binsizes, n_bins, dfeat):
        d = np.asarray(d, dtype=np.float64)
        n = min(-(-ncols // b), L)
        left = -(-(L - n) // 2)
        for g in range(n):
            lo, hi = g * b, min((g + 1) * b, ncols)
            cnt = hi - lo
            m = xw[:, lo:hi].sum(axis=1) / cnt
            p = left + g
            if flip:
                p = L - 1 - p
            out[:, lo:hi] += (d[p] / (cnt * (1.0 + m)))[:, None]
    return out * xw if times_input else out


def autograd_form(x, col0, ncols, flip, binsizes, n_bins, dfeat, dtype=torch.float32, times_input=False):
    """The same by autograd through bin_log1p + centred, computed in `dtype` -> tensor [F, ncols] of that dtype."""
    xw = torch.as_tensor(np.ascontiguousarray(np.asarray(x)[:, col0:col0 + ncols]).astype(np.float64)).to(dtype)
    leaf = xw.clone().requires_grad_(True)
    if ncols == 0:
        return torch.zeros_like(xw)
    loss = 0
    for b, L, d in zip(binsizes, n_bins, dfeat):
        binned = bin_log1p(leaf, b)[:, :L]                      # bins past L are dropped, as the kernels drop them
        feats, _, _ = centred(binned, L, flip=bool(flip))       # [F, L]
        loss = loss + (feats * torch.as_tensor(np.asarray(d)).to(dtype).t()).sum()
    loss.backward()
    g = leaf.grad
    return g * xw if times_input else g


def make_small_dataset(out_dir):
    """tests.synth_data.make_dataset(n_genes=6, seed=5) -- both strands, partial last bins -- with the partners of gene 2 removed from
    the metadata (that draw has no gene without partners of its own) -> (metadata path, id of the gene without partners)."""
    import pandas as pd
    from tests.synth_data import make_dataset
    meta = make_dataset(out_dir, n_genes=6, seed=5)
    table = pd.read_csv(meta)
    table.loc[2, "neighbors"] = np.nan
    table.loc[2, "scores"] = np.nan
    table.to_csv(meta, index=False)
    return meta, table.gene_id[2]
