"""The focal-player estimator of the sampled Shapley interaction indices on the host: the definition (tests/focal_oracle.py) against the
exact indices, its identities, its exact zeros, and the row layout that attribution.focal_words hands the library."""
import itertools

import numpy as np
import pytest

from chromoformer_amd.attribution import focal_players, focal_row_count, focal_words, shapley_permutations
from tests import focal_oracle as fo
from tests import perm_oracle as po
from tests.interaction_oracle import pair_index_fp64


def _game(P, seed, n_out=2):
    """A random game -> v float64 [1, 2^P, n_out], word m at column m."""
    return np.random.default_rng(seed).standard_normal((1, 1 << P, n_out))


def _table(v, words):
    return v[:, [int(m) for m in words]]


def _all_orders(P):
    return np.array(list(itertools.permutations(range(P))), dtype=np.uint8)


@pytest.mark.parametrize("P", [2, 3, 4, 5])
@pytest.mark.parametrize("index", ["sii", "sti"])
def test_all_orders_give_the_exact_index(P, index):
    v = _game(P, 100 + P)
    perms, focal = _all_orders(P), list(range(P))
    words, col = fo.focal_words(perms, focal)
    s = fo.focal_samples(_table(v, words), perms, focal, index, np.float64, col)
    est, _ = fo.focal_estimate_fp64(s)
    ref, scale = pair_index_fp64(v, index)
    assert est.shape == ref.shape == (1, P, P, 2)
    assert (np.abs(est - ref) <= 1e-12 * np.maximum(scale, 1e-300)).all(), np.abs(est - ref).max()
    if P > 2:
        assert np.abs(ref[0][~np.eye(P, dtype=bool)]).min() > 0      # (nothing is compared to zero by accident)


@pytest.mark.parametrize("P", [2, 3, 7])
def test_sii_telescopes_in_every_order(P):
    v = _game(P, 7)
    perms = shapley_permutations(P, 5, 3)
    focal = list(range(P))
    words, col = fo.focal_words(perms, focal)
    s = fo.focal_samples(_table(v, words), perms, focal, "sii", np.float64, col)
    N = (1 << P) - 1
    for i in range(P):
        off = [j for j in range(P) if j != i]
        want = (v[:, N] - v[:, N & ~(1 << i)]) - (v[:, 1 << i] - v[:, 0])
        for q in range(len(perms)):
            assert np.abs(s[:, q, i, off].sum(1) - want).max() <= 1e-12 * np.abs(v).max() * P, (i, q)


def test_the_sii_diagonal_is_the_shapley_sample():
    P = 6
    v = _game(P, 11)
    perms = shapley_permutations(P, 9, 1)
    focal = [4, 0, 5]
    words, col = fo.focal_words(perms, focal)
    table = _table(v, words)
    mean, se = fo.focal_estimate_fp64(fo.focal_samples(table, perms, focal, "sii", np.float64, col))
    phi, phi_se = po.sampled_shapley_fp64(table[:, :po.n_rows(P, 9)], perms)
    for f, i in enumerate(focal):
        assert np.array_equal(mean[:, f, i], phi[:, i]) and np.array_equal(se[:, f, i], phi_se[:, i])
    sti, sti_se = fo.focal_estimate_fp64(fo.focal_samples(table, perms, focal, "sti", np.float64, col))
    for f, i in enumerate(focal):
        assert np.abs(sti[:, f, i] - (v[:, 1 << i] - v[:, 0])).max() <= 1e-15 * 9 and np.abs(sti_se[:, f, i]).max() <= 1e-15


@pytest.mark.parametrize("index", ["sii", "sti"])
def test_null_players_are_exact_zeros_in_fp32(index):
    """Player 2 is null: v(S + 2) = v(S) bit for bit.  As the focal player both marginals are 0; as the partner j the two marginals
    are the same float: d = 0, so inter and se are exactly 0 in the kernel's arithmetic."""
    P, null = 5, 2
    g = _game(P, 23).astype(np.float32)
    v = g[:, [m & ~(1 << null) for m in range(1 << P)]]
    perms = shapley_permutations(P, 300, 2)      # more orders than threads: the strided sums and the tree
    focal = [null, 0, 4]
    words, col = fo.focal_words(perms, focal)
    inter, se = fo.focal_pairs_fp32(_table(v, words), perms, focal, index, col)
    assert inter.dtype == np.float32 and (inter[:, 0] == 0).all() and (se[:, 0] == 0).all()      # a null focal player: its whole row
    assert (inter[:, 1:, null] == 0).all() and (se[:, 1:, null] == 0).all()                       # a null partner: its column
    live = [j for j in range(P) if j != null]
    assert (inter[:, 1][:, live] != 0).all() and (se[:, 1][:, [1, 3, 4]] > 0).all()


@pytest.mark.parametrize("P,n_perm,focal", [(2, 3, [1, 0]), (3, 4, [0, 2]), (4, 24, [0, 1, 2, 3]), (63, 2, [31, 60]), (63, 16, [0, 5, 31, 62]),
                                            (128, 1, [127])])
def test_layout(P, n_perm, focal):
    perms = _all_orders(P) if (P, n_perm) == (4, 24) else shapley_permutations(P, n_perm, 5)
    words, col = focal_words(perms, focal)
    ref_words, ref_col = fo.focal_words(perms, focal)
    assert words == ref_words and col.dtype == np.uint32 and col.shape == (len(focal), n_perm, P, 2) and np.array_equal(col, ref_col)
    lead = po.prefix_words(perms)
    assert words[:len(lead)] == lead      # mark_shapley_sampled's table, unchanged
    R = fo.n_rows(perms, focal)
    assert len(words) == R
    if (P, n_perm) == (63, 2):
        assert R == 370
    if (P, n_perm) == (4, 24):
        assert R == 226
    if (P, n_perm) == (63, 16):      # the unshared layout: 2 + n_focal n_perm (2 (P - 1) - 2) + 2 n_focal rows
        assert R < 5000 < 2 + 4 * 16 * 2 * 61 + 8 == 7818
    used = np.zeros(R, dtype=bool)
    used[:2] = True
    for f, i in enumerate(focal):
        at = focal_row_count(perms, focal[:f])      # the focal player's own rows start with {i} alone and everybody but i
        assert words[at] == 1 << i and words[at + 1] == (1 << P) - 1 - (1 << i)
        used[at:at + 2] = True      # (read by the reducer unless an order starts / ends with i: then the prefix row is)
        for q in range(n_perm):
            o = [int(x) for x in perms[q] if int(x) != i]
            for k in range(P):      # every col entry names the right word
                T = sum(1 << p for p in o[:k])
                assert words[col[f, q, k, 0]] == T and words[col[f, q, k, 1]] == T | 1 << i, (f, q, k)
            used[col[f, q].reshape(-1)] = True
    assert used[len(lead):].all()      # no row behind the leading block goes unread


def test_the_documented_row_count():
    """README / DESIGN.md: P = 63, shapley_permutations(63, 16, 0), focal players 0, 10, 31, 62 (tools/mark_pairs_sampled_bench.py's
    shape): four (focal, order) pairs have the focal player first or last, 4 * 16 * 60 + 4 more rows than 2 + 16 * 62 + 8."""
    perms = shapley_permutations(63, 16, 0)
    assert focal_row_count(perms, [0, 10, 31, 62]) == fo.n_rows(perms, [0, 10, 31, 62]) == 4846 == 2 + 16 * 62 + 8 + 64 * 60 + 4


def test_row_count_formula_by_position():
    for P in (2, 3, 63):
        for r in range(P):
            pi = [p for p in range(1, P)]
            pi.insert(r, 0)
            perms = np.array([pi], dtype=np.uint8)
            words, _ = focal_words(perms, [0])
            extra = P - 2 if r in (0, P - 1) else P - 3
            assert len(words) == 2 + (P - 1) + 2 + extra == fo.n_rows(perms, [0]), (P, r)


def test_python_helpers_refuse_by_name():
    names = ["a", "b", "c"]
    assert focal_players(["c", 0], names, 3).tolist() == [2, 0] and focal_players(1, names, 3).dtype == np.int32
    assert focal_players("b", names, 3).tolist() == [1] and focal_players(np.array([2, 1]), None, 3).tolist() == [2, 1]
    for bad, msg in (([], "at least one"), ([0, 0], "repeats"), (["a", 0], "repeats"), ([3], "outside 0..2"), ([-1], "outside"), (["d"], "not a player name"),
                     ([0.5], "neither"), ([True], "neither"), (None, "at least one")):
        with pytest.raises(ValueError, match="focal_players.*" + msg):
            focal_players(bad, names, 3)
    with pytest.raises(ValueError, match="focal_words: perms"):
        focal_words(np.zeros((1, 1), dtype=np.uint8), [0])
    with pytest.raises(ValueError, match="focal_words: perms\\[1\\]"):
        focal_words(np.array([[0, 1, 2], [0, 0, 2]]), [0])
    with pytest.raises(ValueError, match="focal_players"):
        focal_words(np.array([[0, 1, 2]]), [3])
