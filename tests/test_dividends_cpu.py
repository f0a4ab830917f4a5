"""Harsanyi dividends and interaction indices of any order without a GPU: the oracles of tests/dividend_oracle.py against each other, against
games whose dividends are known in closed form and against the existing Shapley and pair oracles; the bit identities and the
null-player zeros of the fp32 recurrence; the helpers of chromoformer_amd.attribution, their refusals and the exports."""
import os
from math import comb

import numpy as np
import pytest

from chromoformer_amd import _lib
from chromoformer_amd.attribution import (INTERACTION_INDICES, dividend_bound, interaction_sets, set_interaction_weights, set_names,
                                          top_dividends)
from tests import dividend_oracle as dv
from tests.coalition_oracle import shapley_fp64
from tests.interaction_oracle import pair_index_fp32, pair_index_fp64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


def _bits(P):
    """bool [2^P, P]: player p is in coalition m."""
    return (np.arange(1 << P)[:, None] >> np.arange(P)[None, :] & 1).astype(bool)


def _moebius_by_enumeration(v):
    """The definition, subset by subset (float64)."""
    P = dv.players(v)
    out = np.zeros(v.shape)
    for S in range(1 << P):
        T = S
        while True:      # every subset T of S
            out[:, S] += (-1.0) ** (bin(S).count("1") - bin(T).count("1")) * v[:, T]
            if T == 0:
                break
            T = (T - 1) & S
    return out


def _from_dividends(m, sets, index, order):
    """index(S) = sum over U >= S of w[|S|, |U|] m(U) in float64, with the table of set_interaction_weights."""
    P = dv.players(m)
    w = set_interaction_weights(P, index, order)
    words = np.arange(1 << P)
    size = dv.popcount(words)
    out = np.zeros((m.shape[0], len(sets), m.shape[2]))
    for k, S in enumerate(int(x) for x in sets):
        sup = words[(words & S) == S]
        out[:, k] = np.einsum("u,buo->bo", w[bin(S).count("1")][size[sup]], m[:, sup])
    return out


@pytest.mark.parametrize("P", range(1, 9))
def test_the_butterfly_equals_the_definition(P):
    rng = np.random.RandomState(P)
    v = rng.randn(2, 1 << P, 2)
    m = dv.moebius_fp64(v)
    if P <= 6:
        assert np.abs(m - _moebius_by_enumeration(v)).max() < 1e-12
    a = v.copy()      # the recurrence in float64
    for k in range(P):
        x = a.reshape(2, (1 << P) >> (k + 1), 2, 1 << k, 2)
        x[:, :, 1] -= x[:, :, 0]
    assert np.abs(a - m).max() < 1e-12
    # the dividends add back up to every coalition, and the mass is the same sum of magnitudes
    words = np.arange(1 << P)
    for S in (0, 1, (1 << P) - 1, (1 << P) // 3):
        sub = words[(words & ~S) == 0]
        assert np.abs(m[:, sub].sum(1) - v[:, S]).max() < 1e-12
        assert np.abs(dv.mass_fp64(v)[:, S] - np.abs(v[:, sub]).sum(1)).max() < 1e-12
    # the fp32 restatement within the bound of the recurrence, and its mass within rounding of the exact one
    v32 = v.astype(np.float32)
    err = np.abs(dv.moebius_fp32(v32).astype(np.float64) - dv.moebius_fp64(v32))
    assert (err <= dv.dividend_bound(v32)).all()
    assert np.allclose(dv.mass_fp32(v32), dv.mass_fp64(v32), rtol=P * U, atol=0)
    assert (dividend_bound(dv.mass_fp32(v32), P) >= dv.dividend_bound(v32)).all()      # the public bound covers the rounding of mass


def test_closed_form_games():
    P = 6
    x = _bits(P).astype(np.float64)
    rng = np.random.RandomState(3)
    # additive: v(S) = c0 + sum of a_i -- nothing above order 1
    c0, a = rng.randn(), rng.randn(P)
    m = dv.moebius_fp64((c0 + x @ a)[None, :, None])[0, :, 0]
    size = dv.popcount(np.arange(1 << P))
    assert abs(m[0] - c0) < 1e-13 and np.abs(m[1 << np.arange(P)] - a).max() < 1e-13 and np.abs(m[size > 1]).max() < 1e-12
    # unanimity on R = {1, 3, 4}: one dividend
    R = 0b011010
    u = ((np.arange(1 << P) & R) == R).astype(np.float64)
    m = dv.moebius_fp64(u[None, :, None])[0, :, 0]
    assert m[R] == 1.0 and np.abs(np.delete(m, R)).max() < 1e-13
    # three marks of seven that carry the prediction only together: 1/2 on each pair, 1/3 per player, one dividend of 1
    P = 7
    v = ((np.arange(1 << P) & 0b1001001) == 0b1001001).astype(np.float64)[None, :, None]
    sii = pair_index_fp64(v, "sii")[0][0, :, :, 0]
    for i, j in ((0, 3), (0, 6), (3, 6)):
        assert abs(sii[i, j] - 0.5) < 1e-14
    assert np.abs(np.diag(sii)[[0, 3, 6]] - 1 / 3).max() < 1e-14
    m = dv.moebius_fp32(v)[0, :, 0]
    assert m[0b1001001] == 1.0 and np.count_nonzero(m) == 1
    sets = interaction_sets(P, 3)
    I3 = dv.set_index_fp64(v, sets, "sii", 3)[0, :, 0]
    assert abs(I3[list(sets).index(0b1001001)] - 1.0) < 1e-14 and abs(I3[list(sets).index(0b0001001)] - 0.5) < 1e-14
    assert set_names([0b1001001], ["mark%d" % k for k in range(7)]) == ["mark0*mark3*mark6"]


@pytest.mark.parametrize("P", [1, 2, 3, 5, 6])
def test_the_weights_agree_with_the_discrete_derivative_definition(P):
    rng = np.random.RandomState(20 + P)
    v = rng.randn(2, 1 << P, 2)
    m = dv.moebius_fp64(v)
    for index, order in (("sii", 1), ("sii", 2), ("sii", 3), ("sii", 4), ("sti", 1), ("sti", 2), ("sti", 3)):
        if order > P:
            continue
        sets = interaction_sets(P, order)
        ref = dv.set_index_fp64(v, sets, index, order)
        assert np.abs(_from_dividends(m, sets, index, order) - ref).max() < 1e-12, (index, order)
        if index == "sti":      # efficiency: every set of size 1..order together
            assert np.abs(ref.sum(1) - (v[:, -1] - v[:, 0])).max() < 1e-12, order
        # the restatement of the kernel on the fp32 dividends within its derived bound
        v32 = v.astype(np.float32)
        got = dv.set_index_fp32(dv.moebius_fp32(v32), sets, index, order).astype(np.float64)
        assert (np.abs(got - dv.set_index_fp64(v32, sets, index, order)) <= dv.set_index_bound(v32, sets, index, order)).all(), (index, order)


@pytest.mark.parametrize("P", [2, 4, 6])
def test_orders_one_and_two_are_the_existing_indices(P):
    rng = np.random.RandomState(40 + P)
    v = rng.randn(2, 1 << P, 2)
    sets = interaction_sets(P, 2)
    phi = shapley_fp64(v)[0]
    for index in INTERACTION_INDICES:
        got = dv.set_index_fp64(v, sets, index, 2)
        pair = pair_index_fp64(v, index)[0]
        for k, S in enumerate(int(s) for s in sets):
            p = [b for b in range(P) if S >> b & 1]
            want = pair[:, p[0], p[-1]]
            assert np.abs(got[:, k] - want).max() < 1e-12, (index, S)
    one = dv.set_index_fp64(v, interaction_sets(P, 1), "sii", 1)
    assert np.abs(one - phi).max() < 1e-12
    assert np.abs(_from_dividends(dv.moebius_fp64(v), interaction_sets(P, 1), "sii", 1) - phi).max() < 1e-12


def test_bit_identities_and_null_players_in_fp32():
    rng = np.random.RandomState(6)
    P = 6
    v = (rng.randn(2, 1 << P, 2) * 3).astype(np.float32)
    m = dv.moebius_fp32(v)
    assert m.dtype == np.float32 and np.array_equal(m[:, 0], v[:, 0])
    sti = pair_index_fp32(v, "sti")
    for i in range(P):
        assert np.array_equal(m[:, 1 << i], v[:, 1 << i] - v[:, 0]) and np.array_equal(m[:, 1 << i], sti[:, i, i])
        for j in range(i + 1, P):
            want = ((v[:, 1 << i | 1 << j] - v[:, 1 << j]).astype(np.float32) - (v[:, 1 << i] - v[:, 0]).astype(np.float32)).astype(np.float32)
            assert np.array_equal(m[:, 1 << i | 1 << j], want), (i, j)
    words = np.arange(1 << P)
    for null in (0, 2, 5):
        vn = v[:, words & ~(1 << null)]      # the player's rows bit-equal present and absent
        mn = dv.moebius_fp32(vn)
        holds = (words >> null & 1) == 1
        assert (mn[:, holds] == 0).all() and not np.signbit(mn[:, holds]).any()
        assert (mn[:, ~holds] != 0).all()
        for index, order in (("sii", 3), ("sti", 3), ("sii", 1)):
            sets = interaction_sets(P, order)
            I = dv.set_index_fp32(mn, sets, index, order)
            with_null = (sets >> np.uint32(null) & np.uint32(1)) == 1
            assert (I[:, with_null] == 0).all() and (I[:, ~with_null] != 0).all(), (null, index)
    # sti below the top order: the dividends' bits
    sets = interaction_sets(P, 3)
    I = dv.set_index_fp32(m, sets, "sti", 3)
    low = dv.popcount(sets) < 3
    assert np.array_equal(I[:, low], m[:, sets[low]])


def test_interaction_sets_and_the_other_helpers():
    assert interaction_sets(3, 3).tolist() == [1, 2, 4, 3, 5, 6, 7] and interaction_sets(3, 1).tolist() == [1, 2, 4]
    s = interaction_sets(16, 3)
    assert s.dtype == np.uint32 and len(s) == 696 == 16 + comb(16, 2) + comb(16, 3)
    size = dv.popcount(s)
    assert (np.diff(size) >= 0).all() and all((np.diff(s[size == k].astype(np.int64)) > 0).all() for k in (1, 2, 3))
    assert len(interaction_sets(7, 7)) == 127 and len(interaction_sets(1, 1)) == 1
    for P, order in ((16, 16), (5, 2)):
        for index in INTERACTION_INDICES:
            w = set_interaction_weights(P, index, order)
            assert w.shape == (order + 1, P + 1) and w.dtype == np.float64 and (w[0] == 0).all()
    assert np.array_equal(set_interaction_weights(3, "sii", 2), [[0, 0, 0, 0], [0, 1, 1 / 2, 1 / 3], [0, 0, 1, 1 / 2]])
    assert np.array_equal(set_interaction_weights(3, "sti", 2), [[0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 1 / 3]])
    names = ["a", "b", "c"]
    assert set_names(np.arange(8), names) == ["", "a", "b", "a*b", "c", "a*c", "b*c", "a*b*c"]
    mass = np.ones((2, 8, 1), dtype=np.float32)
    b = dividend_bound(mass, 3)
    assert b.shape == mass.shape and b.dtype == np.float64 and (b[:, 0] == 0).all() and np.allclose(b[:, 7], 3 * U, rtol=1e-6)
    div = np.zeros((8, 2), dtype=np.float32)
    div[5], div[2], div[7] = (1, -4), (3, 0), (0.5, 0.5)
    top = top_dividends(div, names, k=2)
    assert [(n, w) for n, w, _ in top] == [("a*c", 5), ("b", 2)] and np.array_equal(top[0][2], [1, -4])
    assert [n for n, _, _ in top_dividends(div, names, k=5, min_order=2)][:2] == ["a*c", "a*b*c"]


def test_the_python_refusals():
    for P, order in ((0, 1), (17, 1), (4, 0), (4, 5)):
        with pytest.raises(ValueError, match="interaction_sets"):
            interaction_sets(P, order)
        with pytest.raises(ValueError, match="set_interaction_weights"):
            set_interaction_weights(P, "sii", order)
    for bad in ("shap", None, 0):
        with pytest.raises(ValueError, match=r"\['sii', 'sti'\]"):
            set_interaction_weights(4, bad, 2)
    with pytest.raises(ValueError, match=r"set_names: words\[1\]"):
        set_names([1, 8], ["a", "b", "c"])
    with pytest.raises(ValueError, match="dividend_bound"):
        dividend_bound(np.ones((2, 8, 1)), 4)
    with pytest.raises(ValueError, match="top_dividends"):
        top_dividends(np.ones((8, 1)), ["a", "b"])
    with pytest.raises(ValueError, match="top_dividends"):
        top_dividends(np.ones((4, 1)), ["a", "b"], k=0)
    # the model's shape checks come before the device is asked for
    import torch
    from chromoformer_amd import ChromoformerClassifier
    model = ChromoformerClassifier(seed=1, max_batch=2)
    for bad in (torch.zeros(3, 100, 2), torch.zeros(3, 1, 2), torch.zeros(3, 256, 1), torch.zeros(256, 2), torch.zeros(3, 256, 2, dtype=torch.float64),
                np.zeros((3, 4, 2), np.float32)):
        with pytest.raises(ValueError, match="shapley_dividends"):
            model.shapley_dividends(bad)
        with pytest.raises(ValueError, match="set_interactions"):
            model.set_interactions(bad)
    with pytest.raises(ValueError, match="sii"):
        model.set_interactions(torch.zeros(1, 4, 2), index="shap")
    with pytest.raises(RuntimeError, match="not on a GPU"):
        model.shapley_dividends(torch.zeros(1, 4, 2))


def test_exports():
    hdr = " ".join(open(os.path.join(ROOT, "include", "chromoformer_hip.h")).read().split())
    assert "#define CF_ABI_VERSION 1" in hdr
    assert "int cf_dividends_from_rows(cf_handle* h, const float* rows, int B, int P, float* div, float* mass /* or NULL */, void* stream);" in hdr
    assert ("int cf_set_interactions_from_dividends(cf_handle* h, const float* div, int B, int P, const uint32_t* sets /* host */, int n_sets, "
            "int index, int order, float* out /* [B, n_sets, n_out] */, void* stream);") in hdr
    assert [len(_lib.SYMBOLS[n][1]) for n in ("cf_dividends_from_rows", "cf_set_interactions_from_dividends")] == [7, 10]
    L = _lib.lib()
    assert L.cf_dividends_from_rows(None, None, 1, 2, None, None, None) != 0
    assert L.cf_last_error() == b"cf_dividends_from_rows: null handle"
    assert L.cf_set_interactions_from_dividends(None, None, 1, 2, None, 1, 0, 1, None, None) != 0
    assert L.cf_last_error() == b"cf_set_interactions_from_dividends: null handle"
    from chromoformer_amd.net import ChromoformerBase
    for name in ("shapley_dividends", "set_interactions", "pcre_dividends", "mark_dividends", "mark_donor_dividends", "mark_window_dividends",
                 "mark_fine_window_dividends"):
        assert getattr(ChromoformerBase, name).__doc__, name
