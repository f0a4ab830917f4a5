"""The permutation estimator of cf_mark_shapley_sampled (model.mark_shapley_sampled) restated in numpy, row layout included.

Per gene the rows are: column 0 nobody present, column 1 everybody, column 2 + q (P - 1) + (k - 1) the first k players of permutation q
(k = 1 .. P - 1).  With r the position of player p in permutation q:
    d_q   = v[col(q, r + 1)] - v[col(q, r)]
    phi   = mean_q d_q
    se    = sqrt(sum_q (d_q - phi)^2 / (n_perm (n_perm - 1)))      0 for n_perm = 1
prefix_words builds the rows' coalitions (Python ints, bit p set: player p present), marginals the d_q in a chosen dtype (float32: the
device's one rounded subtraction), estimate_fp64 the mean and standard error of given d_q in float64."""
import numpy as np


def n_rows(P, n_perm):
    return 2 + int(n_perm) * (int(P) - 1)


def col(q, k, P):
    """The column of the first k players of permutation q."""
    return 0 if k == 0 else 1 if k == P else 2 + q * (P - 1) + (k - 1)


def prefix_words(perms):
    """perms [n_perm, P] -> the R coalitions as Python ints, in row order."""
    perms = np.asarray(perms)
    n_perm, P = perms.shape
    words = [0, (1 << P) - 1]
    for q in range(n_perm):
        m = 0
        for k in range(1, P):
            m |= 1 << int(perms[q, k - 1])
            words.append(m)
    assert len(words) == n_rows(P, n_perm)
    return words


def rows_of_game(value, perms):
    """value(m) -> [n_out] for a coalition word m (a Python int) -> the row table [1, R, n_out] float64 of one gene."""
    return np.array([np.atleast_1d(np.asarray(value(m), dtype=np.float64)) for m in prefix_words(perms)])[None]


def marginals(v, perms, dtype=np.float32):
    """v [B, R, n_out], perms [n_perm, P] -> d [B, n_perm, P, n_out]: d[b, q, p] = v[col(q, r + 1)] - v[col(q, r)], r = rank_q[p],
    one subtraction in `dtype`."""
    perms = np.asarray(perms)
    n_perm, P = perms.shape
    v = np.asarray(v, dtype=dtype)
    assert v.shape[1] == n_rows(P, n_perm), (v.shape, P, n_perm)
    d = np.empty((v.shape[0], n_perm, P, v.shape[2]), dtype=dtype)
    for q in range(n_perm):
        assert sorted(int(x) for x in perms[q]) == list(range(P)), q
        for r in range(P):
            d[:, q, int(perms[q, r])] = v[:, col(q, r + 1, P)] - v[:, col(q, r, P)]
    return d


def estimate_fp64(d):
    """d [B, n_perm, P, n_out] -> (phi, se) [B, P, n_out] in float64."""
    d = np.asarray(d, dtype=np.float64)
    n = d.shape[1]
    phi = d.sum(1) / n
    se = np.sqrt(((d - phi[:, None]) ** 2).sum(1) / (n * (n - 1))) if n > 1 else np.zeros_like(phi)
    return phi, se


def sampled_shapley_fp64(v, perms):
    """The estimator on a row table, everything in float64 -> (phi, se)."""
    return estimate_fp64(marginals(v, perms, np.float64))
