"""Histone-mark coalitions, host side (no GPU): attribution.mark_players and its refusals; the rule log1p(s expm1(u)) on every element
of an absent player equals binning the raw signal scaled over the whole region; the oracle reproduces the reference's logits on
scaled raw files (golden); Shapley values and epistasis of hand-made games with seven players; the C ABI declares, exports and
mirrors the three entry points; the methods and the CLI options are offered."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from chromoformer_amd import _lib
from chromoformer_amd.attribution import coalition_table, mark_coalition_words, mark_players
from oracle import chromoformer_oracle as orc
from tests import mark_oracle as mo
from tests import scan_oracle as so
from tests.coalition_oracle import epistasis_fp32, pair_words, shapley_fp64
from tests.helpers import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINS = (2000, 500, 100)
GENES = ["ENSGSYN00001", "ENSGSYN00000", "ENSGSYN00002"]


def test_mark_players_named_specs():
    marks, regions, names = mark_players("marks", 7, 8)
    assert marks.dtype == regions.dtype == np.uint32
    assert marks.tolist() == [1 << f for f in range(7)] and regions.tolist() == [0x1FF] * 7 and names[3] == "mark3" and len(names) == 7
    marks, regions, names = mark_players("compartments", 7, 8)
    assert marks.tolist() == [1 << f for f in range(7)] * 2 and regions.tolist() == [1] * 7 + [0x1FE] * 7
    assert names[0] == "mark0@promoter" and names[13] == "mark6@pcres"
    marks, regions, names = mark_players("regions", 7, 8)
    assert marks.tolist() == [0x7F] * 9 and regions.tolist() == [1 << r for r in range(9)] and names[:2] == ["promoter", "pcre0"]
    marks, regions, names = mark_players("regions", 7, 15)
    assert len(marks) == 16 and regions[-1] == 1 << 15
    marks, regions, names = mark_players("marks", 3, 2)
    assert marks.tolist() == [1, 2, 4] and regions.tolist() == [7, 7, 7]


def test_mark_players_explicit_lists_and_refusals():
    marks, regions, names = mark_players([((0, 1), (0,)), ([1, 2, 2], range(0, 9, 2)), (iter([6]), [8])], 7, 8)
    assert marks.tolist() == [3, 6, 64] and regions.tolist() == [1, 0b101010101, 256] and len(names) == 3 and len(set(names)) == 3
    bad = ["genes", [], [((0,), (0,))] * 17, [((), (0,))], [((0,), ())], [((7,), (0,))], [((-1,), (0,))], [((0,), (9,))], [((0,), (-1,))],
           [(0, 1)], [((0,), (0,), (0,))], 5]
    for spec in bad:
        with pytest.raises(ValueError, match="mark_players"):
            mark_players(spec, 7, 8)
    with pytest.raises(ValueError, match="mark_players"):
        mark_players("marks", 17, 8)                  # 17 players
    with pytest.raises(ValueError, match="mark_players"):
        mark_players("regions", 7, 16)                # 17 players
    with pytest.raises(ValueError, match="mark_players"):
        mark_players("compartments", 9, 8)            # 18 players
    assert mark_coalition_words([127, 0, 5], 7).tolist() == [127, 0, 5]
    assert mark_coalition_words(np.array([[True, False, True]]), 3).tolist() == [5]
    for keep in ([128], [-1], [], [1.5], np.array([[True, False]])):
        with pytest.raises(ValueError, match="mark_coalitions"):
            mark_coalition_words(keep, 7)


def test_gone_words_of_overlapping_players():
    marks, regions, _ = mark_players([((0, 1), (0, 1)), ((1, 2), (0, 2))], 7, 8)
    assert mo.gone_words(marks, regions, 0b11, 9) == [0] * 9
    assert mo.gone_words(marks, regions, 0b10, 9) == [3, 3] + [0] * 7
    assert mo.gone_words(marks, regions, 0b01, 9) == [6, 0, 6] + [0] * 6
    assert mo.gone_words(marks, regions, 0b00, 9) == [7, 3, 6] + [0] * 6      # the union: mark 1 of the promoter is scaled once


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    ds = so.scan_dataset(str(tmp_path_factory.mktemp("marks")), w_prom=39000)
    return ds, so.dataset_batch(ds, GENES)


HOST32 = 2.384185791015625e-07


def test_rule_equals_binning_the_signal_scaled_over_whole_regions(data):
    """The torch fp32 evaluation of the rule (mark_oracle.mark_rows) against the from-raw oracle (the raw samples of the absent
    players' marks scaled over the whole region, binned by the dataset's own code in fp32), every resolution, s = 2.5 and s = 0, on
    a '-' strand promoter narrowed to 39000 and a 1,800-sample pCRE.  Bound: 4 x what that evaluation reaches on these inputs.  It
    reaches 2.384e-07 (one ulp of a feature in [2, 4); measured on the CPU over the three coalitions below), so the bound is
    9.537e-07.  s = 0 gives exact zeros."""
    ds, batch = data
    assert ds.w_prom == 39000 and ds.genes[GENES[0]]["tss"][2] == "-"
    c, s, e = ds.genes[GENES[1]]["pcres"][0]
    assert e - s == 1800 and not ds.genes[GENES[2]]["pcres"]
    cases = [("marks", 0x7F & ~0x12), ("compartments", 0x3FFF & ~(1 << 1) & ~(1 << 11)), ("regions", 0x1FF & ~0b11)]
    worst = 0.0
    for scale in (2.5, 0.0):
        for spec, word in cases:
            marks, regions, _ = mark_players(spec, 7, 8)
            gone = mo.gone_words(marks, regions, word, 9)
            assert any(gone)
            ref = mo.batch_from_scaled_regions(ds, GENES, gone, scale)
            got = mo.mark_rows(batch, (marks, regions), [word], scale)
            for b in BINS:
                for key in ("promoter_feats", "pcre_feats"):
                    d = (got[key][b] - ref[key][b]).abs().max().item()
                    worst = max(worst, d)
                    if scale == 0.0:
                        assert d == 0.0, (spec, b, key, d)
                for f in range(7):      # s = 0: the absent marks are exact zeros, the others the gene's own bits
                    if scale == 0.0 and gone[0] >> f & 1:
                        assert bool((got["promoter_feats"][b][..., f] == 0).all())
                    if not gone[0] >> f & 1:
                        assert torch.equal(got["promoter_feats"][b][..., f], batch["promoter_feats"][b][..., f])
                    for j in range(8):
                        if scale == 0.0 and gone[1 + j] >> f & 1:
                            assert bool((got["pcre_feats"][b][:, j, :, f] == 0).all())
                        if not gone[1 + j] >> f & 1:
                            assert torch.equal(got["pcre_feats"][b][:, j, :, f], batch["pcre_feats"][b][:, j, :, f])
                for key in ("promoter_pad_masks", "pcre_pad_masks", "interaction_masks"):
                    assert torch.equal(got[key][b], ref[key][b])
            assert torch.equal(got["interaction_freq"], ref["interaction_freq"])
    print("torch fp32 rule vs from raw: %.3e (recorded %.3e), bound %.3e" % (worst, HOST32, 4 * HOST32))
    assert worst <= 4 * HOST32


def test_oracle_logits_equal_the_golden(data):
    """The reference's own dataset and model on scaled raw files (tests/golden/make_mark_coalition_goldens.py) against the rule +
    orc.forward on the unscaled dataset."""
    ds, batch = data
    g = np.load(os.path.join(GOLDEN, "mark_coalitions.npz"))
    assert [str(x) for x in g["genes"]] == GENES and int(g["w_prom"]) == 39000 and len(g["words"]) == 6
    for head, regression in (("clf", False), ("reg", True)):
        P = orc.init_params(None, 42, regression)
        assert g[head].shape == (6, 3, 1 if regression else 2) and g[head].dtype == np.float32
        for k in range(len(g["words"])):
            n = int(g["n_players"][k])
            players = (g["player_marks"][k][:n], g["player_regions"][k][:n])
            lg = mo.oracle_mark_coalitions(P, batch, players, [int(g["words"][k]), (1 << n) - 1], float(g["scales"][k]))
            d = (lg[:, 0] - torch.from_numpy(g[head][k])).abs().max().item()
            d0 = (lg[:, 1] - torch.from_numpy(g["base." + head])).abs().max().item()
            print(head, "case", k, "oracle vs reference %.2e, unperturbed %.2e" % (d, d0))
            assert d < 1e-5 and d0 < 1e-5, (head, k, d, d0)
            assert (g[head][k] != g["base." + head]).any()


def _table(fn, P=7):
    return np.array([[[fn(m)] for m in range(1 << P)]], dtype=np.float64)


def test_shapley_of_hand_made_games_with_seven_players():
    P = 7
    a = np.array([0.5, -1.25, 2.0, 0.0, 3.5, -0.75, 1.0])      # player 3: a dummy
    add = _table(lambda m: 10.0 + sum(a[p] for p in range(P) if m >> p & 1))
    phi, bound = shapley_fp64(add)
    assert phi.shape == (1, P, 1) and np.abs(phi[0, :, 0] - a).max() < 1e-14 and phi[0, 3, 0] == 0.0
    # players 0 and 1 redundant (either one gives 4), player 2 adds 1, player 6 only counts together with player 2, the rest are dummies
    red = _table(lambda m: 4.0 * bool(m & 3) + 1.0 * (m >> 2 & 1) + 6.0 * ((m >> 2 & 1) and (m >> 6 & 1)))
    phi, _ = shapley_fp64(red)
    assert np.abs(phi[0, :, 0] - np.array([2.0, 2.0, 4.0, 0.0, 0.0, 0.0, 3.0])).max() < 1e-14
    assert (phi[0, 3:6, 0] == 0.0).all()
    assert abs(phi.sum() - (red[0, 127, 0] - red[0, 0, 0])) < 1e-14                                    # efficiency
    words = coalition_table("pairs", P)
    assert words.tolist() == pair_words(P) and len(words) == 1 + 7 + 21
    e = epistasis_fp32(add[:, words])[0, :, :, 0]
    assert np.array_equal(e, np.diag(a).astype(np.float32))                                            # additive: no interaction
    e = epistasis_fp32(red[:, words])[0, :, :, 0]
    assert np.array_equal(e, e.T)
    assert e[0, 1] == -4.0 and e[0, 0] == 0.0 and e[1, 1] == 0.0           # redundant: each deletion alone changes nothing, both lose 4
    assert e[2, 6] == 6.0 and e[2, 2] == 7.0 and e[6, 6] == 6.0            # cooperation
    assert (e[3] == 0).all() and (e[:, 3] == 0).all() and e[0, 2] == 0.0    # the dummy; independent players


def test_the_entry_points_are_declared_bound_and_offered():
    hdr = open(os.path.join(ROOT, "include", "chromoformer_hip.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert "int cf_mark_coalitions(cf_handle* h, const cf_batch* batch, const cf_mark_opts* opts, const uint32_t* keep, int n_coal, float* logits, void* stream);" in flat
    assert "int cf_mark_shapley(cf_handle* h, const cf_batch* batch, const cf_mark_opts* opts, float* phi, float* logits_all, void* stream);" in flat
    assert "int cf_mark_epistasis(cf_handle* h, const cf_batch* batch, const cf_mark_opts* opts, float* eps, float* logits_pairs, void* stream);" in flat
    assert {"cf_mark_coalitions", "cf_mark_shapley", "cf_mark_epistasis"} <= set(_lib.SYMBOLS)
    assert "#define CF_ABI_VERSION 1" in hdr
    # int n_players; (pad) const unsigned*; const unsigned*; float scale; (pad)
    assert C.sizeof(_lib.cf_mark_opts) == 32
    assert [_lib.cf_mark_opts.n_players.offset, _lib.cf_mark_opts.player_marks.offset, _lib.cf_mark_opts.player_regions.offset,
            _lib.cf_mark_opts.scale.offset] == [0, 8, 16, 24]
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct cf_mark_opts \{(.*?)\} cf_mark_opts;", hdr, re.S).group(1), flags=re.S)
    assert re.findall(r"(\w+);", body) == [n for n, _ in _lib.cf_mark_opts._fields_]
    L = _lib.lib()
    for name in ("cf_mark_coalitions", "cf_mark_shapley", "cf_mark_epistasis"):
        assert hasattr(L, name), name
    assert L.cf_mark_coalitions(None, None, None, None, 0, None, None) != 0
    assert L.cf_last_error() == b"cf_mark_coalitions: null handle"
    assert L.cf_mark_shapley(None, None, None, None, None, None) != 0 and L.cf_last_error() == b"cf_mark_shapley: null handle"
    assert L.cf_mark_epistasis(None, None, None, None, None, None) != 0 and L.cf_last_error() == b"cf_mark_epistasis: null handle"
    from chromoformer_amd import ChromoformerRegressor
    from chromoformer_amd.net import Chromoformer
    for name in ("mark_coalitions", "mark_shapley", "mark_epistasis", "mark_shapley_dataset"):
        assert getattr(Chromoformer, name) is getattr(ChromoformerRegressor, name)
    out = subprocess.run([sys.executable, "-m", "chromoformer_amd.predict", "--help"], cwd=ROOT, capture_output=True, text=True,
                         check=True).stdout
    for opt in ("--mark-shapley-out", "--mark-epistasis-out", "--mark-players", "--mark-scale"):
        assert opt in out, opt
