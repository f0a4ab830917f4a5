"""The focal-player estimator of the sampled interaction indices (cf_mark_*_shapley_interactions_sampled, cf_perm_interactions_from_rows,
model.mark_shapley_interactions_sampled) restated in plain Python / numpy, row layout included.

Focal player i, an order pi of all P players, o = pi with i removed, T_k = the first k players of o, r the position of i in pi.  For
j = o[a]:
    d(j) = (v(T_{a+1} + i) - v(T_{a+1})) - (v(T_a + i) - v(T_a))
    s(j) = d(j) for "sii", w_a d(j) with w_a = 2 (P - 1 - a) / P for "sti"
    inter[i, j] = mean_q s_q(j),   se = sqrt(sum_q (s_q - mean)^2 / (n_perm (n_perm - 1)))      0 for n_perm = 1
The diagonal j = i: "sii" the sample is i's marginal at its own position, v(T_r + i) - v(T_r) (the Shapley sample); "sti" it is
v({i}) - v(nobody) in every order (se 0).

Rows per gene: perm_oracle.prefix_words (nobody, everybody, the prefixes of every order), then per focal player {i} alone, everybody but
i, and per order the rows T_k + i for k = 1 .. r - 1, then the rows T_k for k = r + 1 .. P - 2: the other T_k, T_k + i are prefixes of pi.
focal_words builds the words and col[f, q, k, {without, with}] from the sets themselves; focal_samples the samples in a chosen dtype
(float32: the device's rounded operations, in its grouping); focal_estimate_fp64 mean and standard error of given samples in float64;
focal_pairs_fp32 the kernel's operations in the kernel's order (interaction_oracle._block_sum_fp32: thread t sums q = t, t + 256, ...,
then the tree)."""
import numpy as np

from tests.interaction_oracle import _block_sum_fp32
from tests.perm_oracle import prefix_words


def _word(players):
    return sum(1 << int(p) for p in players)


def n_rows(perms, focal):
    """The row-count formula: R = 2 + n_perm (P - 1) + sum_f (2 + sum_q extra), extra = P - 2 where i is first or last, else P - 3."""
    perms = np.asarray(perms)
    n_perm, P = perms.shape
    R = 2 + n_perm * (P - 1)
    for i in focal:
        R += 2
        for q in range(n_perm):
            r = [int(x) for x in perms[q]].index(int(i))
            R += P - 2 if r in (0, P - 1) else P - 3
    return R


def focal_words(perms, focal, want_words=True):
    """-> (words, col): the R coalitions as Python ints in row order, and int64 [n_focal, n_perm, P, 2] with col[f, q, k, 0] the row of
    T_k and col[f, q, k, 1] the row of T_k + i.  want_words=False: the rows behind the leading block are counted, their words not built
    (None stands for each)."""
    perms = np.asarray(perms)
    n_perm, P = perms.shape
    words = list(prefix_words(perms))
    lead = len(words)
    col = np.full((len(focal), n_perm, P, 2), -1, dtype=np.int64)
    for f, i in enumerate(int(x) for x in focal):
        alone, without = len(words), len(words) + 1
        words += [1 << i, (1 << P) - 1 - (1 << i)]
        for q in range(n_perm):
            pi = [int(x) for x in perms[q]]
            r = pi.index(i)
            o = pi[:r] + pi[r + 1:]
            base = 2 + q * (P - 1) - 1      # the first k players of pi sit at row base + k, 1 <= k <= P - 1
            col[f, q, 0] = (0, alone if r else base + 1)      # (a prefix of pi wherever there is one: pi starts / ends with i)
            col[f, q, P - 1] = (without if r < P - 1 else base + P - 1, 1)
            for k in range(1, r):                  # T_k + i is no prefix of pi while i comes later
                col[f, q, k, 1] = len(words)
                words.append(_word(o[:k]) | 1 << i if want_words else None)
            for k in range(max(r, 1), P - 1):      # ... and is pi[:k + 1] from i's position on
                col[f, q, k, 1] = base + k + 1
            for k in range(1, min(r, P - 2) + 1):  # T_k is pi[:k] up to i's position
                col[f, q, k, 0] = base + k
            for k in range(r + 1, P - 1):          # ... and no prefix behind it
                col[f, q, k, 0] = len(words)
                words.append(_word(o[:k]) if want_words else None)
    assert (col >= 0).all() and len(words) == n_rows(perms, focal) and lead == 2 + n_perm * (P - 1)
    return words, col


def sti_weights(P):
    """w_a = 2 (P - 1 - a) / P, a = 0 .. P - 2, float64."""
    return np.array([2.0 * (P - 1 - a) / P for a in range(P - 1)], dtype=np.float64)


def focal_samples(v, perms, focal, index, dtype=np.float32, col=None):
    """v [B, R, n_out] in focal_words' layout -> s [B, n_perm, n_focal, P, n_out]: the samples, every operation in `dtype` (the weight
    rounded to it first), in the grouping above."""
    assert index in ("sii", "sti"), index
    perms = np.asarray(perms)
    n_perm, P = perms.shape
    if col is None:
        col = focal_words(perms, focal, want_words=False)[1]
    v = np.asarray(v, dtype=dtype)
    assert v.shape[1] == n_rows(perms, focal), (v.shape, n_rows(perms, focal))
    w = sti_weights(P).astype(dtype)
    s = np.zeros((v.shape[0], n_perm, len(focal), P, v.shape[2]), dtype=dtype)
    for f, i in enumerate(int(x) for x in focal):
        for q in range(n_perm):
            pi = [int(x) for x in perms[q]]
            r = pi.index(i)
            o = np.array(pi[:r] + pi[r + 1:])
            c = col[f, q]
            m = (v[:, c[:, 1]] - v[:, c[:, 0]]).astype(dtype)      # [B, P, n_out]: i's marginal on top of T_k
            d = (m[:, 1:] - m[:, :-1]).astype(dtype)               # [B, P - 1, n_out]: at a = 0 .. P - 2
            if index == "sti":
                d = (w[None, :, None] * d).astype(dtype)
            s[:, q, f, o] = d
            if q == 0:
                alone = m[:, 0]      # v({i}) - v(nobody) through the rows order 0 names (the same words in every order)
            s[:, q, f, i] = m[:, r] if index == "sii" else alone
    return s


def focal_estimate_fp64(s):
    """s [B, n_perm, n_focal, P, n_out] -> (mean, se) [B, n_focal, P, n_out] in float64."""
    s = np.asarray(s, dtype=np.float64)
    n = s.shape[1]
    mean = s.sum(1) / n
    se = np.sqrt(((s - mean[:, None]) ** 2).sum(1) / (n * (n - 1))) if n > 1 else np.zeros_like(mean)
    return mean, se


def focal_pairs_fp32(v, perms, focal, index, col=None):
    """-> (inter, se) float32 [B, n_focal, P, n_out] in the operations and the order of k_perm_pairs: the fp32 samples, per thread
    acc = acc + s_q over q = t, t + 256, ..., the tree, one division by float32(n_perm); then e = s_q - mean, acc = acc + e e (product
    and sum rounded separately), the tree, the division by float32(n_perm (n_perm - 1)) and the square root.  The "sti" diagonal is the
    one subtraction, se 0.  The "sii" diagonal's se returned here is NOT the kernel's: there the kernel runs k_perm_shapley's own
    function (the square fused into the sum, an approximate root), which numpy does not restate; the GPU tests pin that entry to
    k_perm_shapley's stderr bit for bit instead and leave it out of the comparison with this function.  Its inter is the kernel's."""
    s = focal_samples(v, perms, focal, index, np.float32, col)
    B, n, F, P, n_out = s.shape
    flat = s.reshape(B, n, F * P * n_out)
    mean = (_block_sum_fp32(flat) / np.float32(n)).astype(np.float32)
    if n > 1:
        e = (flat - mean[:, None]).astype(np.float32)
        sq = _block_sum_fp32((e * e).astype(np.float32))
        se = np.sqrt((sq / np.float32(float(n) * (n - 1))).astype(np.float32)).astype(np.float32)
    else:
        se = np.zeros_like(mean)
    inter, se = mean.reshape(B, F, P, n_out), se.reshape(B, F, P, n_out)
    if index == "sti":
        for f, i in enumerate(int(x) for x in focal):
            inter[:, f, i] = s[:, 0, f, i]
            se[:, f, i] = 0
    return inter, se
