"""The oracle of the pCRE coalition forwards (ChromoformerBase.pcre_coalitions / pcre_shapley / pcre_epistasis): the contract's
edited interaction masks with one orc.forward per coalition word, exact Shapley values by the subset formula in float64, and the
pair-deletion epistasis in the fp32 operation order of the device.  A coalition is a word m: bit j set keeps pCRE slot j, a clear
bit sets row and column j + 1 of the interaction mask at every resolution.  Used by the coalition tests and by
tests/golden/make_pcre_coalition_goldens.py."""
from math import factorial

import numpy as np
import torch

from oracle import chromoformer_oracle as orc


def coalition_masks(batch, m, S):
    """The batch with every gene's interaction masks edited for coalition word m (row and column j + 1 set for every clear bit j < S)."""
    m = int(m)
    if m < 0 or m >> S:
        raise ValueError("coalition word 0x%x has a bit >= S = %d" % (m, S))
    out = {k: ({b: t.clone() for b, t in v.items()} if isinstance(v, dict) else v.clone()) for k, v in batch.items()}
    gone = [j + 1 for j in range(S) if not m >> j & 1]
    for im in out["interaction_masks"].values():
        im[:, 0, gone, :] = True
        im[:, 0, :, gone] = True
    return out


def oracle_coalitions(P, batch, keep, cfg=None):
    """-> logits [B, n_coal, n_out]: orc.forward on the contract's edited masks, one pass per word of `keep`."""
    S = orc._cfg(cfg)["i_max"]
    with torch.no_grad():
        return torch.stack([orc.forward(P, coalition_masks(batch, m, S), cfg) for m in keep], 1)


def shapley_weights(S):
    """w(k) = k! (S - k - 1)! / S!, k = 0..S-1, float64."""
    return np.array([factorial(k) * factorial(S - k - 1) / factorial(S) for k in range(S)], dtype=np.float64)


def shapley_fp64(v):
    """v [B, 2^S, n_out] indexed by coalition word -> (phi [B, S, n_out], bound [B, S, n_out]) in float64 by the subset formula:
    phi[b, j] = sum over m with bit j clear of w(|m|) (v[b, m | 1 << j] - v[b, m]);  bound = sum of w |difference| (the scale of
    the rounding-error bound of any fp32 evaluation)."""
    v = np.asarray(v, dtype=np.float64)
    n = v.shape[1]
    S = n.bit_length() - 1
    assert n == 1 << S
    words = np.arange(n)
    w = shapley_weights(S)[np.minimum([bin(m).count("1") for m in range(n)], S - 1)]      # (the full word is never a minuend's m)
    phi = np.zeros((v.shape[0], S, v.shape[2]))
    bound = np.zeros_like(phi)
    for j in range(S):
        m = words[(words >> j & 1) == 0]
        d = (v[:, m | 1 << j] - v[:, m]) * w[m][None, :, None]
        phi[:, j] = d.sum(1)
        bound[:, j] = np.abs(d).sum(1)
    return phi, bound


def pair_words(S):
    """The pair-deletion words: N = 2^S - 1, N without i (i ascending), N without i and j (i < j, lexicographic)."""
    N = (1 << S) - 1
    return [N] + [N & ~(1 << i) for i in range(S)] + [N & ~(1 << i) & ~(1 << j) for i in range(S) for j in range(i + 1, S)]


def epistasis_fp32(v):
    """v [B, 1 + S + S (S - 1) / 2, n_out] in the order of pair_words -> eps [B, S, S, n_out] float32:
    eps[i, j] = ((v_N - v_{N\\i}) - v_{N\\j}) + v_{N\\ij} for i < j, every operation rounded to fp32, mirrored below the diagonal;
    eps[i, i] = v_N - v_{N\\i}."""
    v = np.asarray(v, dtype=np.float32)
    R = v.shape[1]
    S = next(s for s in range(33) if 1 + s + s * (s - 1) // 2 == R)
    eps = np.zeros((v.shape[0], S, S, v.shape[2]), dtype=np.float32)
    p = 1 + S
    for i in range(S):
        eps[:, i, i] = v[:, 0] - v[:, 1 + i]
        for j in range(i + 1, S):
            e = ((v[:, 0] - v[:, 1 + i]).astype(np.float32) - v[:, 1 + j]).astype(np.float32) + v[:, p]
            eps[:, i, j] = eps[:, j, i] = e.astype(np.float32)
            p += 1
    return eps
