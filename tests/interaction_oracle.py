"""Oracles of the pairwise Shapley interaction indices (cf_shapley_interactions_from_rows, the *_shapley_interactions entry points and
the ChromoformerBase methods of the same names) on a coalition table v [B, 2^P, n_out], word m at column m.  For players i != j and S
over the 2^(P - 2) coalitions that hold neither:

    delta_ij(S) = (v(S + i + j) - v(S + j)) - (v(S + i) - v(S)),      I_ij = sum_S w(|S|) delta_ij(S)

with the weight table of the index (attribution.interaction_weights): "sii" s! (P - s - 2)! / (P - 1)!, the Shapley values on the
diagonal; "sti" (2 / P) / C(P - 1, s), v({i}) - v(nobody) on the diagonal.  pair_index_fp64 is the definition in float64 with the scale
of any fp32 evaluation's rounding error; pair_index_fp32 restates k_shapley_pairs operation by operation, summation order included."""
import numpy as np

from chromoformer_amd.attribution import interaction_weights
from tests.coalition_oracle import shapley_fp64, shapley_weights

THREADS = 256      # kShapThreads


def _players(v):
    n = v.shape[1]
    P = n.bit_length() - 1
    assert n == 1 << P and P >= 2, v.shape
    return P


def open_bits(q, i, j):
    """The words of rank q among those with bits i < j clear: a zero opened at bit i, then at bit j."""
    lowi, lowj = (1 << i) - 1, (1 << j) - 1
    m1 = (q & ~lowi) << 1 | (q & lowi)
    return (m1 & ~lowj) << 1 | (m1 & lowj)


def _popcount(m):
    m = np.asarray(m, dtype=np.int64)
    return sum(m >> k & 1 for k in range(32))


def pair_index_fp64(v, index):
    """-> (I, scale), float64 [B, P, P, n_out] each.  Off the diagonal I is the definition above and scale[i, j] =
    sum_S w (|a| + |b| + |c| + |d|) over the four table entries of delta; the diagonal is shapley_fp64's (phi, bound) for "sii" and
    (v({i}) - v(0), |v({i})| + |v(0)|) for "sti"."""
    v = np.asarray(v, dtype=np.float64)
    P = _players(v)
    w = interaction_weights(P, index)
    I = np.zeros((v.shape[0], P, P, v.shape[2]))
    scale = np.zeros_like(I)
    if index == "sii":
        phi, bound = shapley_fp64(v)
    q = np.arange(1 << (P - 2))
    for i in range(P):
        if index == "sii":
            I[:, i, i], scale[:, i, i] = phi[:, i], bound[:, i]
        else:
            I[:, i, i], scale[:, i, i] = v[:, 1 << i] - v[:, 0], np.abs(v[:, 1 << i]) + np.abs(v[:, 0])
        for j in range(i + 1, P):
            m = open_bits(q, i, j)
            ws = w[_popcount(m)][None, :, None]
            a, b, c, d = v[:, m | 1 << i | 1 << j], v[:, m | 1 << j], v[:, m | 1 << i], v[:, m]
            I[:, i, j] = I[:, j, i] = (ws * ((a - b) - (c - d))).sum(1)
            scale[:, i, j] = scale[:, j, i] = (ws * (np.abs(a) + np.abs(b) + np.abs(c) + np.abs(d))).sum(1)
    return I, scale


def _block_sum_fp32(terms):
    """terms float32 [B, n, n_out], in rank order -> float32 [B, n_out]: thread t adds the terms of rank t, t + 256, ... in ascending
    order to 0, then the tree red[t] += red[t + s], s = 128, 64, ..., 1."""
    B, n, n_out = terms.shape
    pad = -n % THREADS
    t = np.concatenate([terms, np.zeros((B, pad, n_out), np.float32)], 1).reshape(B, -1, THREADS, n_out)
    live = np.concatenate([np.ones(n, bool), np.zeros(pad, bool)]).reshape(-1, THREADS)
    red = np.zeros((B, THREADS, n_out), np.float32)
    for k in range(t.shape[1]):      # (a thread past the last rank adds nothing: its sum keeps its bits, -0 included)
        red = np.where(live[k][None, :, None], (red + t[:, k]).astype(np.float32), red)
    s = THREADS // 2
    while s:
        red[:, :s] = (red[:, :s] + red[:, s:2 * s]).astype(np.float32)
        s //= 2
    return red[:, 0]


def pair_index_fp32(v, index):
    """-> I float32 [B, P, P, n_out] in the operations and the order of k_shapley_pairs: the weights rounded to fp32, delta in the
    grouping above with every subtraction rounded, acc = acc + w delta per thread (product and sum rounded separately), the tree: off
    the diagonal the kernel's bits.  The "sti" diagonal is one subtraction (its bits too); the "sii" diagonal follows k_shapley's
    order with a separately rounded product -- the device's k_shapley fuses the product into the accumulate, so there the comparison
    is within rounding (the tests pin that diagonal to k_shapley's own phi instead)."""
    v = np.asarray(v, dtype=np.float32)
    P = _players(v)
    w2 = interaction_weights(P, index).astype(np.float32)
    w1 = shapley_weights(P).astype(np.float32)
    I = np.zeros((v.shape[0], P, P, v.shape[2]), dtype=np.float32)
    q = np.arange(1 << (P - 2))
    h = np.arange(1 << (P - 1))
    for i in range(P):
        if index == "sii":
            low = (1 << i) - 1
            m = (h & ~low) << 1 | (h & low)
            d = (v[:, m | 1 << i] - v[:, m]).astype(np.float32)
            I[:, i, i] = _block_sum_fp32((w1[_popcount(m)][None, :, None] * d).astype(np.float32))
        else:
            I[:, i, i] = (v[:, 1 << i] - v[:, 0]).astype(np.float32)
        for j in range(i + 1, P):
            m = open_bits(q, i, j)
            with_j = (v[:, m | 1 << i | 1 << j] - v[:, m | 1 << j]).astype(np.float32)
            without_j = (v[:, m | 1 << i] - v[:, m]).astype(np.float32)
            delta = (with_j - without_j).astype(np.float32)
            I[:, i, j] = I[:, j, i] = _block_sum_fp32((w2[_popcount(m)][None, :, None] * delta).astype(np.float32))
    return I


def epistasis_grouping_fp32(a, b, c, d):
    """k_epistasis's grouping of the same four values, a = v(S + i + j), b = v(S + j), c = v(S + i), d = v(S): ((a - b) - c) + d, every
    operation rounded to fp32.  Exactly 0 when the lower-indexed player i is null (a == b, c == d: (0 - c) + c); when the
    higher-indexed player j is null (a == c, b == d) it is ((a - b) - a) + b, which carries the rounding of a - b."""
    a, b, c, d = (np.float32(x) for x in (a, b, c, d))
    return np.float32(np.float32(np.float32(a - b) - c) + d)
