"""pCRE coalitions without a GPU: the oracle of tests/coalition_oracle.py reproduces the reference's logits of all 256 coalitions of
the demo batch (tests/golden/pcre_coalitions.npz); shapley_fp64 is the Shapley value (permutation definition, efficiency, null
players exactly 0); coalition words that differ only in dummy bits give equal rows; the coalition rows are those of the ablation
oracle; attribution.coalition_table's orders and the host-side normalisation and refusals of `keep`; the entry points are declared,
bound and offered."""
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import chromoformer_oracle as orc
from tests.ablation_oracle import oracle_ablation
from tests.coalition_oracle import coalition_masks, epistasis_fp32, oracle_coalitions, pair_words, shapley_fp64, shapley_weights
from tests.helpers import GOLDEN, load_npz_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S3 = dict(i_max=3)


@pytest.fixture(scope="module")
def small():
    """i_max = 3, 5 genes with [0, 0, 0, 2, 3] dummy slots: all 8 coalition rows by the oracle, computed once (40 gene-forwards)."""
    cfg = orc._cfg(S3)
    batch = orc.synthetic_batch(5, cfg=cfg, seed=13, regime="realistic")
    P = orc.init_params(cfg, 3, False)
    v = oracle_coalitions(P, batch, range(8), cfg)
    dummy = torch.stack([m[:, 0, 0, 1:] for m in batch["interaction_masks"].values()]).all(0).numpy()
    return cfg, batch, P, v, dummy


@pytest.mark.parametrize("head", ["clf", "reg"])
def test_the_oracle_reproduces_the_reference_on_sampled_coalitions(head):
    """32 of the 256 words (the corners, single deletions and a seeded sample): 192 oracle gene-forwards per head."""
    z = np.load(os.path.join(GOLDEN, "pcre_coalitions.npz"))
    ref = z["demo.%s" % head]
    assert ref.shape == (6, 256, 1 if head == "reg" else 2) and ref.dtype == np.float32
    batch = load_npz_batch("demo_subset.npz")[0]
    rng = np.random.RandomState(5)
    words = sorted({255, 0} | {255 & ~(1 << j) for j in range(8)} | set(rng.choice(256, 22, replace=False).tolist()))
    assert len(words) <= 32 and {0, 255} <= set(words)
    got = oracle_coalitions(orc.init_params(None, 42, head == "reg"), batch, words).numpy()
    assert np.abs(got - ref[:, words]).max() <= 1e-5


def test_the_golden_has_the_structure_of_the_demo_batch():
    """6 genes with 0, 1, 5, 8, 8 and 3 pCREs: a bit of a dummy slot changes nothing, a bit of a live slot does."""
    z = np.load(os.path.join(GOLDEN, "pcre_coalitions.npz"))
    m = np.arange(256)
    for head in ("clf", "reg"):
        v = z["demo.%s" % head]
        for b, n in enumerate((0, 1, 5, 8, 8, 3)):
            live = (1 << n) - 1
            assert np.array_equal(v[b], v[b][m & live]), (head, b)
            for j in range(n):
                assert (v[b][m | 1 << j] != v[b][m & ~(1 << j)]).any(), (head, b, j)
        phi, _ = shapley_fp64(v)
        assert np.abs(phi.sum(1) - (v[:, 255].astype(np.float64) - v[:, 0])).max() < 1e-12
        for b, n in enumerate((0, 1, 5, 8, 8, 3)):
            assert (phi[b, n:] == 0).all() and (phi[b, :n] != 0).all()


def test_shapley_fp64_is_the_permutation_definition():
    rng = np.random.RandomState(0)
    v = rng.randn(4, 8, 2)
    phi, bound = shapley_fp64(v)
    ref = np.zeros_like(phi)
    perms = list(itertools.permutations(range(3)))
    for perm in perms:
        m = 0
        for j in perm:
            ref[:, j] += (v[:, m | 1 << j] - v[:, m]) / len(perms)
            m |= 1 << j
    assert np.abs(phi - ref).max() < 1e-14
    assert (bound >= np.abs(phi) - 1e-15).all()
    for S in (1, 2, 3, 8, 16):      # a slot's weights sum to 1: C(S - 1, k) subsets of size k
        w = shapley_weights(S)
        from math import comb
        assert abs(sum(comb(S - 1, k) * w[k] for k in range(S)) - 1.0) < 1e-13


def test_small_config_efficiency_null_players_and_dummy_twins(small):
    cfg, batch, P, v, dummy = small
    assert dummy.sum(1).tolist() == [0, 0, 0, 2, 3]
    phi, _ = shapley_fp64(v.numpy())
    gap = np.abs(phi.sum(1) - (v[:, 7].double() - v[:, 0].double()).numpy()).max()
    assert gap < 1e-14, gap      # (fp64 rounding of 2^S terms of magnitude ~1)
    assert (phi[dummy] == 0).all()
    assert (phi[~dummy] != 0).all()
    for b in range(5):      # words differing only in dummy bits give equal rows
        drop = sum(1 << j for j in range(3) if dummy[b, j])
        for m in range(8):
            assert torch.equal(v[b, m], v[b, m & ~drop]), (b, m)
    assert all(torch.equal(v[4, m], v[4, 0]) for m in range(8))      # the gene with no pCRE


def test_coalition_rows_are_the_ablation_rows(small):
    cfg, batch, P, v, dummy = small
    abl = oracle_ablation(P, batch, cfg)
    assert torch.equal(v[:, [7, 6, 5, 3, 0]], abl)
    # and the masks are the ablation's
    from tests.ablation_oracle import variant_masks
    for m, var in ((7, 0), (6, 1), (5, 2), (3, 3), (0, 4)):
        a, b = coalition_masks(batch, m, 3), variant_masks(batch, var, 3)
        assert all(torch.equal(a["interaction_masks"][r], b["interaction_masks"][r]) for r in a["interaction_masks"])
    with pytest.raises(ValueError):
        coalition_masks(batch, 8, 3)


def test_epistasis_fp32_on_an_additive_and_a_redundant_game():
    S = 3
    words = pair_words(S)
    add = np.array([[[sum((j + 1.0) for j in range(S) if m >> j & 1)] for m in words]], dtype=np.float32)      # additive: no interaction
    e = epistasis_fp32(add)
    assert e.shape == (1, 3, 3, 1) and np.array_equal(e[0, :, :, 0], np.diag([1.0, 2.0, 3.0]).astype(np.float32))
    red = np.array([[[float(bool(m & 3))] for m in words]], dtype=np.float32)      # slots 0 and 1 redundant: either one suffices
    e = epistasis_fp32(red)[0, :, :, 0]
    assert np.array_equal(e, e.T) and e[0, 1] == -1.0 and e[0, 0] == 0.0 and e[1, 1] == 0.0 and e[0, 2] == 0.0


def test_coalition_table_orders():
    from chromoformer_amd.attribution import coalition_table
    assert coalition_table("all", 3).tolist() == list(range(8)) and coalition_table("all", 3).dtype == np.uint32
    assert coalition_table("pairs", 3).tolist() == [7, 6, 5, 3, 4, 2, 1]
    p = coalition_table("pairs", 8)
    assert len(p) == 1 + 8 + 28 and p.tolist() == pair_words(8) and p[9] == 255 - 3 and p[-1] == 63
    assert len(coalition_table("all", 16)) == 65536
    for bad in (("some", 3), ("all", 0), ("pairs", 2.5)):
        with pytest.raises(ValueError, match="coalition_table"):
            coalition_table(*bad)


def test_keep_normalisation_and_refusals_on_the_host():
    from chromoformer_amd.attribution import coalition_words
    assert coalition_words([7, 0, 5], 3).tolist() == [7, 0, 5] and coalition_words([7], 3).dtype == np.uint32
    assert coalition_words(np.array([1, 2], dtype=np.int16), 3).tolist() == [1, 2]
    assert coalition_words(torch.tensor([3, 4]), 3).tolist() == [3, 4]
    assert coalition_words(np.array([[True, False, True], [False, False, False]]), 3).tolist() == [5, 0]
    assert coalition_words(torch.tensor([[False, True, True]]), 3).tolist() == [6]
    assert coalition_words([65535], 16).tolist() == [65535]
    for bad in ([8], [-1], [1, 256], np.array([[True, False]]), [], [1.5], np.zeros((2, 2), dtype=np.int64)):
        with pytest.raises(ValueError, match="pcre_coalitions"):
            coalition_words(bad, 3)
    with pytest.raises(ValueError, match="i_max = 3"):
        coalition_words([8], 3)


def test_the_entry_points_are_declared_bound_and_offered():
    hdr = open(os.path.join(ROOT, "include", "chromoformer_hip.h")).read()
    for name in ("cf_pcre_coalitions", "cf_pcre_shapley", "cf_pcre_epistasis"):
        assert re.search(r"int\s+%s\s*\(\s*cf_handle\s*\*" % name, hdr), name
    assert re.search(r"cf_pcre_coalitions\([^)]*const\s+uint32_t\s*\*\s*keep\s*,\s*int\s+n_coal\s*,\s*float\s*\*\s*logits\s*,\s*void\s*\*\s*stream\s*\)", hdr)
    from chromoformer_amd import _lib
    assert {"cf_pcre_coalitions", "cf_pcre_shapley", "cf_pcre_epistasis"} <= set(_lib.SYMBOLS)
    from chromoformer_amd import ChromoformerRegressor
    from chromoformer_amd.net import Chromoformer
    for name in ("pcre_coalitions", "pcre_shapley", "pcre_epistasis"):
        assert getattr(Chromoformer, name) is getattr(ChromoformerRegressor, name)
    out = subprocess.run([sys.executable, "-m", "chromoformer_amd.predict", "--help"], cwd=ROOT, capture_output=True, text=True,
                         check=True).stdout
    assert "--pcre-shapley-out" in out and "--pcre-epistasis-out" in out
