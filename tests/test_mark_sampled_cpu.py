"""Wide histone-mark coalitions and permutation-sampled Shapley values, host side (no GPU): the C ABI declares, exports and mirrors the
two entry points and their options struct; the methods and the CLI options are offered and the parser errors hold;
attribution.mark_players_wide, mark_wide_words and shapley_permutations; the estimator restated in float64 (tests/perm_oracle.py) on
hand-made games."""
import ctypes as C
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from chromoformer_amd import _lib
from chromoformer_amd.attribution import mark_players, mark_players_wide, mark_wide_words, shapley_permutations
from tests import perm_oracle as po
from tests.coalition_oracle import shapley_fp64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cf_mark_coalitions_wide", "cf_mark_shapley_sampled")


def test_the_entry_points_are_declared_bound_and_offered():
    hdr = open(os.path.join(ROOT, "include", "chromoformer_hip.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert ("int cf_mark_coalitions_wide(cf_handle* h, const cf_batch* batch, const cf_mark_wide_opts* opts, const uint32_t* keep, int n_coal, "
            "float* logits, void* stream);") in flat
    assert ("int cf_mark_shapley_sampled(cf_handle* h, const cf_batch* batch, const cf_mark_wide_opts* opts, const uint8_t* perms, int n_perm, "
            "float* phi, float* se, float* logits_rows, void* stream);") in flat
    assert set(NAMES) <= set(_lib.SYMBOLS)
    assert "#define CF_ABI_VERSION 1" in hdr
    # int n_players; (pad) const unsigned*; const unsigned*; float scale; (pad) const float* [3]; const float* [3]
    o = _lib.cf_mark_wide_opts
    assert C.sizeof(o) == 80
    assert [getattr(o, n).offset for n, _ in o._fields_] == [0, 8, 16, 24, 32, 56]
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct cf_mark_wide_opts \{(.*?)\} cf_mark_wide_opts;", hdr, re.S).group(1), flags=re.S)
    assert re.findall(r"(\w+)(?:\[CF_MAX_RES\])?;", body) == [n for n, _ in o._fields_] == [
        "n_players", "player_marks", "player_regions", "scale", "donor_promoter_feats", "donor_pcre_feats"]
    assert C.sizeof(_lib.cf_mark_opts) == 32 and C.sizeof(_lib.cf_mark_donor_opts) == 72      # the exact game's structs are left as they are
    for name in NAMES:
        res, args = _lib.SYMBOLS[name]
        assert res is C.c_int and args[1] == C.POINTER(_lib.cf_batch) and args[2] == C.POINTER(o), name
    assert len(_lib.SYMBOLS["cf_mark_coalitions_wide"][1]) == 7 and len(_lib.SYMBOLS["cf_mark_shapley_sampled"][1]) == 9
    L = _lib.lib()
    for name in NAMES:
        assert hasattr(L, name), name
    assert L.cf_abi_version() == 1
    assert L.cf_mark_coalitions_wide(None, None, None, None, 0, None, None) != 0
    assert L.cf_last_error() == b"cf_mark_coalitions_wide: null handle"
    assert L.cf_mark_shapley_sampled(None, None, None, None, 0, None, None, None, None) != 0
    assert L.cf_last_error() == b"cf_mark_shapley_sampled: null handle"
    from chromoformer_amd import ChromoformerRegressor
    from chromoformer_amd.net import Chromoformer
    for name in ("mark_coalitions_wide", "mark_shapley_sampled", "mark_shapley_sampled_dataset"):
        assert getattr(Chromoformer, name) is getattr(ChromoformerRegressor, name)
    out = subprocess.run([sys.executable, "-m", "chromoformer_amd.predict", "--help"], cwd=ROOT, capture_output=True, text=True,
                         check=True).stdout
    for opt in ("--mark-sampled-shapley-out", "--mark-donor-sampled-shapley-out", "--mark-sampled-players", "--mark-perms", "--mark-seed"):
        assert opt in out, opt
    assert "{marks,compartments,regions,cells}" in out


def test_parser_errors(tmp_path):
    from chromoformer_amd import predict
    base = ["-m", str(tmp_path / "meta.csv"), "-d", str(tmp_path), "-o", str(tmp_path / "p.csv")]
    out = str(tmp_path / "out.npz")
    bad = [["--mark-donor-sampled-shapley-out", out],                                 # needs --donor-npy-dir
           ["--donor-npy-dir", str(tmp_path)],                                         # donor signals nobody reads: still an error
           ["--mark-perms", "8"], ["--mark-seed", "1"], ["--mark-sampled-players", "cells"],      # options without their output
           ["--mark-sampled-shapley-out", out, "--mark-perms", "0"],
           ["--mark-sampled-shapley-out", out, "--mark-sampled-players", "genes"],
           ["--mark-sampled-shapley-out", out, "--mark-scale", "-1"],
           ["--mark-sampled-shapley-out", out, "--mark-players", "marks"],             # the exact game's players do not apply
           ["--mark-scale", "0.5"],                                                    # still needs an output it applies to
           ["--mark-donor-sampled-shapley-out", out, "--donor-npy-dir", str(tmp_path), "--mark-scale", "0.5"]]      # the donor rule has no scale
    for extra in bad:
        with pytest.raises(SystemExit) as e:
            predict.main(base + extra)
        assert e.value.code == 2, extra
    # accepted by the parser: the run then fails on the missing metadata file, not in the parser
    for extra in (["--mark-sampled-shapley-out", out, "--mark-scale", "0.5", "--mark-perms", "2", "--mark-seed", "3", "--mark-sampled-players", "regions"],
                  ["--mark-donor-sampled-shapley-out", out, "--donor-npy-dir", str(tmp_path)]):
        with pytest.raises(FileNotFoundError):
            predict.main(base + extra)


def test_mark_players_wide():
    marks, regions, names = mark_players_wide("cells", 7, 8)
    assert marks.dtype == regions.dtype == np.uint32 and len(marks) == len(names) == 63
    for rho in range(9):
        for f in range(7):
            p = rho * 7 + f
            assert marks[p] == 1 << f and regions[p] == 1 << rho
            assert names[p] == ("mark%d@promoter" % f if rho == 0 else "mark%d@pcre%d" % (f, rho - 1))
    marks, regions, names = mark_players_wide("cells", 7, 16)
    assert len(marks) == 119 and names[118] == "mark6@pcre15" and regions[118] == 1 << 16
    with pytest.raises(ValueError, match=r"mark_players_wide: 136 players"):
        mark_players_wide("cells", 8, 16)
    with pytest.raises(ValueError, match="mark_players_wide: 129 players"):
        mark_players_wide([((0,), (0,))] * 129, 7, 8)
    assert len(mark_players_wide([((0,), (0,))] * 128, 7, 8)[0]) == 128
    with pytest.raises(ValueError, match="mark_players"):
        mark_players("cells", 7, 8)                                   # the exact game's function is as it was
    for spec in ("marks", "compartments", "regions", [((0, 1), (0, 1)), ((1, 2), (0, 2))]):
        a, b = mark_players(spec, 7, 8), mark_players_wide(spec, 7, 8)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    for spec in ("genes", [], [((), (0,))], [((7,), (0,))], [((0,), (9,))], 5):
        with pytest.raises(ValueError, match="mark_players_wide"):
            mark_players_wide(spec, 7, 8)


def test_mark_wide_words():
    bits = (0, 31, 32, 63, 64, 118)
    m = sum(1 << p for p in bits)
    w = mark_wide_words([m, 0, (1 << 119) - 1], 119)
    assert w.dtype == np.uint32 and w.shape == (3, 4) and w.flags["C_CONTIGUOUS"]
    assert w[0].tolist() == [0x80000001, 0x80000001, 0x00000001, 1 << (118 - 96)] and w[1].tolist() == [0] * 4
    assert w[2].tolist() == [0xFFFFFFFF] * 3 + [(1 << 23) - 1]
    for row, word in zip(w, (m, 0, (1 << 119) - 1)):      # round trip
        assert sum(int(x) << (32 * k) for k, x in enumerate(row)) == word
        assert [p for p in range(119) if row[p // 32] >> (p % 32) & 1] == [p for p in range(119) if word >> p & 1]
    keep = np.zeros((2, 119), dtype=bool)
    keep[0, list(bits)] = True
    assert np.array_equal(mark_wide_words(keep, 119), w[:2])
    assert mark_wide_words([5, 127], 7).tolist() == [[5], [127]] and mark_wide_words([1 << 32], 33).tolist() == [[0, 1]]
    for bad in ([1 << 119], [-1], [], [1.5], np.zeros((2, 118), dtype=bool), "ab"):
        with pytest.raises(ValueError, match="mark_coalitions_wide"):
            mark_wide_words(bad, 119)


def test_shapley_permutations():
    a = shapley_permutations(63, 16, 0)
    assert a.dtype == np.uint8 and a.shape == (16, 63) and (np.sort(a, 1) == np.arange(63)).all()
    assert np.array_equal(a, shapley_permutations(63, 16, 0)) and not np.array_equal(a, shapley_permutations(63, 16, 1))
    assert len({tuple(r) for r in a}) == 16
    assert np.array_equal(shapley_permutations(63, 4, 0), a[:4])      # a prefix of the same stream
    assert shapley_permutations(1, 3, 7).tolist() == [[0]] * 3 and shapley_permutations(128, 1, 0).max() == 127
    for P, n in ((0, 1), (129, 1), (5, 0)):
        with pytest.raises(ValueError, match="shapley_permutations"):
            shapley_permutations(P, n)


def test_the_row_layout():
    perms = np.array([[2, 0, 1], [1, 2, 0]])
    assert po.n_rows(3, 2) == 6
    assert po.prefix_words(perms) == [0b000, 0b111, 0b100, 0b101, 0b010, 0b110]
    assert [po.col(1, k, 3) for k in range(4)] == [0, 4, 5, 1]
    assert po.prefix_words(np.array([[0]])) == [0, 1]


def test_the_estimator_on_hand_made_games():
    rng = np.random.default_rng(3)
    # an additive game: every order gives the weights exactly, so the standard error is 0
    P = 7
    a = np.array([3.0, -1.5, 0.25, 0.0, 2.0, -4.0, 0.5])
    perms = shapley_permutations(P, 5, 11)
    v = po.rows_of_game(lambda m: 10.0 + sum(a[p] for p in range(P) if m >> p & 1), perms)
    assert v.shape == (1, 2 + 5 * 6, 1)
    d = po.marginals(v, perms, np.float64)
    assert np.array_equal(d, np.broadcast_to(a[None, None, :, None], d.shape))
    phi, se = po.estimate_fp64(d)
    assert np.array_equal(phi[0, :, 0], a) and (se == 0).all() and phi[0, 3, 0] == 0.0
    # four players, all 24 orders: the exact Shapley values; efficiency
    table = rng.normal(size=(1, 16, 2))
    every = np.array(list(itertools.permutations(range(4))), dtype=np.uint8)
    v = po.rows_of_game(lambda m: table[0, m], every)
    phi, se = po.sampled_shapley_fp64(v, every)
    exact, _ = shapley_fp64(table)
    assert np.abs(phi - exact).max() < 1e-14 and (se > 0).all()
    assert np.abs(phi.sum(1) - (table[:, 15] - table[:, 0])).max() < 1e-14
    # efficiency holds for any sample of orders (it telescopes in each), also for one order, whose standard error is 0
    for n in (1, 3):
        some = every[rng.choice(24, n, replace=False)]
        v = po.rows_of_game(lambda m: table[0, m], some)
        phi, se = po.sampled_shapley_fp64(v, some)
        assert np.abs(phi.sum(1) - (table[:, 15] - table[:, 0])).max() < 1e-14
        assert (se == 0).all() if n == 1 else (se > 0).any()
    # a null player (its bit never changes the value) gets exactly 0 in float32 marginals as well
    v = po.rows_of_game(lambda m: table[0, m & ~0b0100], every).astype(np.float32)
    d = po.marginals(v, every, np.float32)
    assert d.dtype == np.float32 and (d[:, :, 2] == 0).all() and (d[:, :, 0] != 0).any()
