"""The pairwise Shapley interaction indices without a GPU: the two weight tables and the oracles of tests/interaction_oracle.py against
games whose indices are known in closed form, Shapley-Taylor efficiency, the Shapley values on the sii diagonal, exact zeros for a
null player in the kernel's grouping (and not in k_epistasis's), the refusals of interaction_weights and the exports."""
import os
import re
from math import comb

import numpy as np
import pytest

from chromoformer_amd import _lib
from chromoformer_amd.attribution import INTERACTION_INDICES, interaction_index, interaction_weights
from tests.coalition_oracle import shapley_fp64
from tests.interaction_oracle import epistasis_grouping_fp32, pair_index_fp32, pair_index_fp64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cf_shapley_interactions_from_rows", "cf_pcre_shapley_interactions", "cf_mark_shapley_interactions", "cf_mark_donor_shapley_interactions",
         "cf_mark_window_shapley_interactions", "cf_mark_fine_shapley_interactions")


def _bits(P):
    """bool [2^P, P]: player p is in coalition m."""
    return (np.arange(1 << P)[:, None] >> np.arange(P)[None, :] & 1).astype(bool)


def _pair_game(P, rng):
    """v(S) = c0 + sum_{i in S} a_i + sum_{i < j in S} b_ij -> (v [1, 2^P, 1], b [P, P] symmetric, zero diagonal)."""
    c0, a = rng.randn(), rng.randn(P)
    b = np.triu(rng.randn(P, P), 1)
    b = b + b.T
    x = _bits(P).astype(np.float64)
    v = c0 + x @ a + 0.5 * np.einsum("mi,ij,mj->m", x, b, x)
    return v[None, :, None], b


@pytest.mark.parametrize("index", INTERACTION_INDICES)
def test_a_game_of_pair_terms_returns_them(index):
    rng = np.random.RandomState(0)
    for P in (2, 3, 5, 7):
        v, b = _pair_game(P, rng)
        I, scale = pair_index_fp64(v, index)
        off = ~np.eye(P, dtype=bool)
        assert np.abs(I[0, :, :, 0] - b)[off].max() < 1e-12, P
        assert (scale[0, :, :, 0][off] > 0).all()
        assert np.array_equal(I, I.transpose(0, 2, 1, 3))


def test_a_triple_term_is_shared_by_its_three_pairs():
    """c [{0, 1, 2} in S] adds c / 2 to each of its pairs under sii and c / 3 under sti, and nothing to any other pair (P = 5)."""
    rng = np.random.RandomState(1)
    P, c = 5, 1.75
    v, b = _pair_game(P, rng)
    v = v + c * _bits(P)[:, :3].all(1)[None, :, None]
    for index, share in (("sii", c / 2), ("sti", c / 3)):
        I = pair_index_fp64(v, index)[0][0, :, :, 0]
        for i in range(P):
            for j in range(P):
                if i != j:
                    want = b[i, j] + (share if i < 3 and j < 3 else 0.0)
                    assert abs(I[i, j] - want) < 1e-12, (index, i, j)


def test_the_weight_tables():
    for P in range(2, 17):
        sii, sti = interaction_weights(P, "sii"), interaction_weights(P, "sti")
        assert sii.dtype == sti.dtype == np.float64 and sii.shape == sti.shape == (P - 1,)
        counts = np.array([comb(P - 2, s) for s in range(P - 1)], dtype=np.float64)
        assert abs((counts * sii).sum() - 1.0) < 1e-14, P
        assert np.allclose(sti, [(2.0 / P) / comb(P - 1, s) for s in range(P - 1)], rtol=1e-15, atol=0)
    assert np.array_equal(interaction_weights(2, "sii"), [1.0]) and np.array_equal(interaction_weights(2, "sti"), [1.0])
    assert np.allclose(interaction_weights(5), [0.25, 1 / 12, 1 / 12, 0.25])


@pytest.mark.parametrize("P", [2, 3, 5, 7])
def test_shapley_taylor_efficiency_and_the_sii_diagonal(P):
    rng = np.random.RandomState(10 + P)
    v = rng.randn(3, 1 << P, 2)
    I, _ = pair_index_fp64(v, "sti")
    upper = np.triu(np.ones((P, P), dtype=bool))
    gap = I[:, upper].sum(1) - (v[:, -1] - v[:, 0])
    assert np.abs(gap).max() < 1e-12
    for i in range(P):
        assert np.array_equal(I[:, i, i], v[:, 1 << i] - v[:, 0])
    S, scale = pair_index_fp64(v, "sii")
    phi, bound = shapley_fp64(v)
    for i in range(P):
        assert np.array_equal(S[:, i, i], phi[:, i]) and np.array_equal(scale[:, i, i], bound[:, i])
    # the fp32 restatement of the kernel stays within the rounding bound of the definition
    for index, ref in (("sii", S), ("sti", I)):
        n = 2 ** (P - 2) + 5
        err = np.abs(pair_index_fp32(v.astype(np.float32), index).astype(np.float64) - pair_index_fp64(v.astype(np.float32), index)[0])
        assert (err <= n * 2.0 ** -24 / (1 - n * 2.0 ** -24) * pair_index_fp64(v.astype(np.float32), index)[1] + 1e-300).all(), index


@pytest.mark.parametrize("null", [1, 4], ids=["lower_index", "higher_index"])
def test_a_null_player_gives_exact_zeros_in_the_kernels_grouping(null):
    """Player `null` of 6: its rows bit-equal present and absent.  Its row and column of pair_index_fp32 are exact zeros under both
    indices, whether it is the lower- or the higher-indexed player of a pair; the pairs of the other players are not."""
    rng = np.random.RandomState(5)
    P = 6
    v = (rng.randn(2, 1 << P, 2) * 3).astype(np.float32)
    m = np.arange(1 << P)
    v = v[:, m & ~(1 << null)]
    for index in INTERACTION_INDICES:
        I = pair_index_fp32(v, index)
        off = [p for p in range(P) if p != null]
        assert (I[:, null, off] == 0).all() and (I[:, off, null] == 0).all(), index
        assert (I[:, off][:, :, off] != 0).all(), index
        assert np.array_equal(I, I.transpose(0, 2, 1, 3))
        if index == "sii":
            assert (I[:, null, null] == 0).all()


def test_the_epistasis_grouping_is_not_exact_for_a_null_higher_player():
    """a = v(S + i + j), b = v(S + j), c = v(S + i), d = v(S).  j null: a == c and b == d.  The kernel's (a - b) - (c - d) is x - x = 0;
    k_epistasis's ((a - b) - c) + d rounds a - b first: with a = 1 and b = 2^-25 it is ((1 - 2^-25 -> 1) - 1) + 2^-25 = 2^-25."""
    a = c = np.float32(1.0)
    b = d = np.float32(2.0 ** -25)
    assert np.float32(np.float32(a - b) - np.float32(c - d)) == 0
    assert epistasis_grouping_fp32(a, b, c, d) == np.float32(2.0 ** -25)
    # the lower-indexed player null (a == b, c == d): both groupings give an exact zero
    a = b = np.float32(1.0)
    c = d = np.float32(2.0 ** -25)
    assert epistasis_grouping_fp32(a, b, c, d) == 0 and np.float32(np.float32(a - b) - np.float32(c - d)) == 0


def test_interaction_weights_and_index_reject_bad_names():
    for bad in ("shap", "SII", "", None, 0):
        with pytest.raises(ValueError, match=r"\['sii', 'sti'\]"):
            interaction_weights(4, bad)
        with pytest.raises(ValueError, match=r"\['sii', 'sti'\]"):
            interaction_index(bad)
    with pytest.raises(ValueError, match="at least 2"):
        interaction_weights(1, "sii")
    assert interaction_index("sii") == 0 and interaction_index("sti") == 1


def test_exports():
    hdr = open(os.path.join(ROOT, "include", "chromoformer_hip.h")).read()
    flat = " ".join(hdr.split())
    assert "#define CF_ABI_VERSION 1" in hdr and "#define CF_INTERACTION_SII 0" in hdr and "#define CF_INTERACTION_STI 1" in hdr
    assert "int cf_shapley_interactions_from_rows(cf_handle* h, const float* rows, int B, int P, int index, float* inter, void* stream);" in flat
    assert ("int cf_pcre_shapley_interactions(cf_handle* h, const cf_batch* batch, int index, float* inter, float* phi, float* logits_all, "
            "void* stream);") in flat
    for name, opts in zip(NAMES[2:], ("cf_mark_opts", "cf_mark_donor_opts", "cf_mark_window_opts", "cf_mark_fine_opts")):
        assert re.search(r"int %s\(cf_handle\* h, const cf_batch\* batch, const %s\* opts, int index, float\* inter, float\* phi, "
                         r"float\* logits_all, void\* stream\);" % (name, opts), flat), name
    assert set(NAMES) <= set(_lib.SYMBOLS)
    assert [len(_lib.SYMBOLS[n][1]) for n in NAMES] == [7, 7, 8, 8, 8, 8]
    L = _lib.lib()
    for name in NAMES:
        assert hasattr(L, name), name
    # refusals that need no device: by name
    assert L.cf_shapley_interactions_from_rows(None, None, 1, 2, 0, None, None) != 0
    assert L.cf_last_error() == b"cf_shapley_interactions_from_rows: null handle"
    assert L.cf_pcre_shapley_interactions(None, None, 0, None, None, None, None) != 0
    assert L.cf_last_error() == b"cf_pcre_shapley_interactions: null handle"
    for name in NAMES[2:]:
        assert getattr(L, name)(None, None, None, 0, None, None, None, None) != 0
        assert L.cf_last_error() == name.encode() + b": null handle"
    from chromoformer_amd.net import ChromoformerBase
    for name in ("pcre_shapley_interactions", "mark_shapley_interactions", "mark_donor_shapley_interactions", "mark_window_shapley_interactions",
                 "mark_fine_window_shapley_interactions", "shapley_interactions"):
        doc = getattr(ChromoformerBase, name).__doc__
        assert "Phi_ij = I_ij / 2" in doc and "Phi_ii = phi_i - sum_{j != i} I_ij / 2" in doc, name
