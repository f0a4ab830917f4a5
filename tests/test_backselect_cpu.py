"""Greedy player selection, host side (no GPU): the selection rule restated in numpy (tests/backselect_oracle.py) on hand-made games;
attribution.backselect_row_count, backselect_words and subset_names; the C ABI declares, exports and mirrors the four entry points and
their two structs; the functions of chromoformer_amd.backselect and the CLI options are offered; what is refused without a device."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from chromoformer_amd import _lib
from chromoformer_amd import backselect as bs
from chromoformer_amd.attribution import backselect_row_count, backselect_words, subset_bools, subset_names
from tests import backselect_oracle as bo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cf_mark_backselect", "cf_mark_window_backselect", "cf_mark_fine_backselect", "cf_backselect_from_rows")


def game(f):
    return lambda m: np.array([f(m)], dtype=np.float32)


def has(m, *players):
    return all(m >> p & 1 for p in players)


def test_three_marks_together():
    """The README's example: three marks that only count together, a weak fourth and a null fifth.  Every mark alone scores zero;
    the back-selection drops the null and the weak player first and keeps exactly the three."""
    v = game(lambda m: 2.0 * has(m, 0, 1, 2) + 0.1 * has(m, 3))
    assert all(v(1 << p)[0] - v(0)[0] == 0 for p in (0, 1, 2, 4))      # alone, none of them moves the prediction
    order, values, s, rows = bo.greedy(v, 5)
    assert s == 1 and order.tolist() == [4, 3, 0, 1, 2]
    assert values[:, 0].tolist() == [np.float32(2.1), np.float32(2.1), 2.0, 0.0, 0.0, 0.0]
    assert [len(r) for r in rows] == [2, 5, 4, 3, 2] and sum(len(r) for r in rows) == backselect_row_count(5)
    thr, size, subset = bo.finish(values, order, s, frac=0.9)
    assert thr == np.float32(np.float32(0.9) * np.float32(2.1)) and size == 3 and subset.tolist() == [True, True, True, False, False]
    # a stricter threshold needs the weak player as well; a threshold nobody misses needs no player at all
    assert bo.finish(values, order, s, frac=1.0)[1:][0] == 4 and bo.finish(values, order, s, frac=0.0)[1] == 0
    assert bo.finish(values, order, s, threshold=5.0)[1] == 5      # never reached below everybody: everybody, by definition
    o2, v2, s2 = bo.replay(rows, 5)
    assert np.array_equal(o2, order) and np.array_equal(v2, values) and s2 == s


def test_two_redundant_players_keep_exactly_one():
    v = game(lambda m: 1.0 if m & 0b011 else 0.0)      # player 2 is null
    full = 0b111
    assert v(full)[0] - v(full & ~1)[0] == 0 and v(full)[0] - v(full & ~2)[0] == 0      # leave-one-out scores both zero
    order, values, s, _ = bo.greedy(v, 3)
    assert order.tolist() == [0, 2, 1] and values[:, 0].tolist() == [1.0, 1.0, 1.0, 0.0]      # (the three-way tie goes to player 0)
    thr, size, subset = bo.finish(values, order, s)
    assert size == 1 and subset.tolist() == [False, True, False]


def test_ties_nulls_and_nan():
    assert bo.pick([1.0, 3.0, 3.0, 2.0], 1) == 1 and bo.pick([1.0, 3.0, 3.0, 2.0], -1) == 0
    assert bo.pick([np.nan, -np.inf, np.nan], 1) == 0 and bo.pick([np.nan, -5.0, np.nan], 1) == 1 and bo.pick([np.nan, -5.0], -1) == 1
    assert bo.pick([np.inf, np.nan], -1) == 0      # both keys are -inf: the lowest index
    v = game(lambda m: 0.0)      # all null: every round is a tie, the players leave in index order
    order, values, s, _ = bo.greedy(v, 4)
    assert s == 1 and order.tolist() == [0, 1, 2, 3] and bo.finish(values, order, s)[1] == 0
    a = np.array([1.0, 2.0, 4.0, 8.0])
    nan_at = 0b1011      # everybody less player 2: never chosen while any other candidate is a number
    v = game(lambda m: np.nan if m == nan_at else sum(a[p] for p in range(4) if m >> p & 1))
    order, values, s, rows = bo.greedy(v, 4)
    assert order.tolist() == [0, 1, 2, 3] and not np.isnan(values).any() and np.isnan(rows[1][2, 0])
    thr, size, subset = bo.finish(np.where(np.arange(5)[:, None] == 2, np.nan, values), order, s, frac=0.5)
    assert size == 1      # the NaN set of two players is not sufficient, the single player 3 (8 >= 7.5) is


def test_direction_and_modes():
    a = np.array([3.0, -1.0, 0.5, 2.0])
    v = game(lambda m: 1.0 + sum(a[p] for p in range(4) if m >> p & 1))
    back, vb, s, _ = bo.greedy(v, 4)
    assert s == 1 and back.tolist() == [1, 2, 3, 0]      # the removal that leaves the most first: the negative player, then ascending weight
    fwd, vf, sf, _ = bo.greedy(v, 4, mode="forward")
    assert fwd.tolist() == [0, 3, 2, 1] == back[::-1].tolist() and vf[0, 0] == 1.0 and vf[4, 0] == vb[0, 0] == 5.5
    neg, vn, sn, _ = bo.greedy(v, 4, direction=-1)
    assert sn == -1 and neg.tolist() == [0, 3, 2, 1]      # keyed on -v: the removal that lowers the value most
    w = game(lambda m: -v(m)[0])
    auto, _, sa, _ = bo.greedy(w, 4)
    assert sa == -1 and auto.tolist() == back.tolist()      # a prediction below the absent row: the sign flips by itself
    # forward mode: the sufficient set is the first `size` additions
    thr, size, subset = bo.finish(vf, fwd, sf, mode="forward", frac=0.9)
    assert thr == np.float32(np.float32(1.0) + np.float32(np.float32(0.9) * np.float32(4.5))) and size == 2 and subset.tolist() == [True, False, False, True]
    # the path is not monotone: the count runs from the small end
    vals = np.array([[4.0], [1.0], [5.0], [0.5], [0.0]], dtype=np.float32)      # after 0 .. 4 removals
    assert bo.finish(vals, np.arange(4), 1, frac=0.9)[1] == 2      # the 2-player set reaches 5 >= 3.6 although the 3-player set does not


def test_greedy_agrees_with_replay_and_visited_on_random_tables():
    rng = np.random.default_rng(5)
    for P, mode, direction in ((1, "backward", 0), (2, "forward", 0), (6, "backward", 0), (6, "forward", -1), (9, "backward", 1)):
        table = rng.normal(size=(1 << P, 2)).astype(np.float32)
        table[rng.integers(0, 1 << P, 3)] = table[0]      # some ties
        order, values, s, rows = bo.greedy(lambda m: table[m], P, mode, direction, target=1)
        o2, v2, s2 = bo.replay(rows, P, mode, direction, target=1)
        assert np.array_equal(order, o2) and np.array_equal(values, v2) and s == s2 and sorted(order.tolist()) == list(range(P))
        words = bo.visited(order, P, mode)
        assert [len(w) for w in words] == [P - t for t in range(P - 1)]
        for t, ws in enumerate(words):
            assert np.array_equal(np.stack([table[w] for w in ws]), rows[1 + t])
        path = backselect_words(order, mode)
        assert np.array_equal(np.stack([table[int(w[0])] for w in path]), values)


def test_host_helpers():
    assert [backselect_row_count(P) for P in (1, 2, 63, 128)] == [2, 4, 2017, 8257]
    with pytest.raises(ValueError, match="backselect_row_count"):
        backselect_row_count(0)
    for P in (5, 40, 119):      # kw = 1, 2, 4
        order = np.random.default_rng(P).permutation(P)
        for mode in ("backward", "forward"):
            w = backselect_words(order, mode)
            assert w.dtype == np.uint32 and w.shape == (P + 1, (P + 31) // 32)
            sets = [sum(int(x) << (32 * k) for k, x in enumerate(row)) for row in w]
            assert sets[0] == (0 if mode == "forward" else (1 << P) - 1) and sets[P] == ((1 << P) - 1 if mode == "forward" else 0)
            for t in range(P):
                assert sets[t] ^ sets[t + 1] == 1 << int(order[t])
    for bad in ([0, 0, 1], [], [[0, 1]], [1, 2]):
        with pytest.raises(ValueError, match="backselect_words"):
            backselect_words(bad)
    with pytest.raises(ValueError, match="backselect_words"):
        backselect_words([0, 1], "sideways")
    names = ["a", "b", "c", "d"]
    assert subset_names(np.array([True, False, False, True]), names) == ["a", "d"] == subset_names(0b1001, names)
    assert subset_names(np.array([0b0110], dtype=np.uint32), names) == ["b", "c"]
    with pytest.raises(ValueError, match="subset_names"):
        subset_names(np.array([True, False]), names)
    words = torch.tensor([[-1, 1], [0, 0]], dtype=torch.int32)      # (the library's words arrive as int32: bit 31 is the sign)
    b = subset_bools(words, 35)
    assert b.shape == (2, 35) and b[0].tolist() == [True] * 33 + [False] * 2 and not b[1].any()


def test_the_entry_points_are_declared_bound_and_offered():
    hdr = open(os.path.join(ROOT, "include", "chromoformer_hip.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    for stem, opts in (("cf_mark_backselect", "cf_mark_wide_opts"), ("cf_mark_window_backselect", "cf_mark_window_opts"),
                       ("cf_mark_fine_backselect", "cf_mark_fine_opts")):
        assert ("int %s(cf_handle* h, const cf_batch* batch, const %s* opts, const cf_backselect_opts* bopts, const cf_backselect_out* out, "
                "void* stream);" % (stem, opts)) in flat
    assert ("int cf_backselect_from_rows(cf_handle* h, const float* rows, int B, int P, int n_out, const cf_backselect_opts* bopts, "
            "const cf_backselect_out* out, void* stream);") in flat
    assert "#define CF_ABI_VERSION 1" in hdr and "#define CF_BACKSELECT_BACKWARD 0" in hdr and "#define CF_BACKSELECT_FORWARD 1" in hdr
    assert _lib.BACKSELECT_MODE == {"backward": 0, "forward": 1}
    for struct, size, fields in ((_lib.cf_backselect_opts, 24, ["mode", "target", "direction", "frac", "threshold"]),
                                 (_lib.cf_backselect_out, 56, ["order", "values", "size", "subset", "rows", "threshold", "direction"])):
        name = struct.__name__
        assert C.sizeof(struct) == size and [n for n, _ in struct._fields_] == fields
        body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1), flags=re.S)
        assert re.findall(r"(\w+);", body) == fields
    # the siblings' structs keep their sizes
    assert [C.sizeof(s) for s in (_lib.cf_mark_opts, _lib.cf_mark_donor_opts, _lib.cf_mark_wide_opts, _lib.cf_mark_window_opts)] == [32, 72, 80, 104]
    assert set(NAMES) <= set(_lib.SYMBOLS)
    L = _lib.lib()
    assert L.cf_abi_version() == 1
    for name in NAMES:
        assert hasattr(L, name), name
        n = len(_lib.SYMBOLS[name][1])
        assert getattr(L, name)(*([None] * 2 + [0, 0, 0] + [None] * 3 if n == 8 else [None] * n)) != 0
        assert L.cf_last_error() == b"%s: null handle" % name.encode()
    import inspect
    from chromoformer_amd.net import Chromoformer
    for name in ("mark_backselect", "mark_window_backselect", "mark_fine_window_backselect", "backselect", "mark_backselect_dataset"):
        f = getattr(bs, name)      # functions on a model: the model classes' public names are a kept surface
        assert callable(f) and inspect.getdoc(f) and list(inspect.signature(f).parameters)[0] == "model" and not hasattr(Chromoformer, name), name
    out = subprocess.run([sys.executable, "-m", "chromoformer_amd.predict", "--help"], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    for opt in ("--mark-backselect-out", "--mark-donor-backselect-out", "--mark-backselect-players", "--backselect-mode", "--backselect-frac"):
        assert opt in out, opt


def test_refusals_without_a_device(tmp_path):
    from chromoformer_amd import net, predict
    model = net.ChromoformerClassifier(seed=1, max_batch=2)      # (never .cuda())
    b = _lib.cf_batch()
    table = torch.zeros(1, 8, 2)
    for kw, text in ((dict(mode="sideways"), "mode = 'sideways'"), (dict(direction=2), "direction = 2"), (dict(direction=0), "direction = 0"),
                     (dict(frac=float("nan")), "frac = nan"), (dict(frac=float("inf")), "frac = inf"), (dict(target=2), "target = 2 outside"),
                     (dict(target=-1), "target = -1 outside")):
        for who, call in (("mark_backselect", lambda **k: bs.mark_backselect(model, b, **k)),
                          ("mark_window_backselect", lambda **k: bs.mark_window_backselect(model, b, **k)),
                          ("mark_fine_window_backselect", lambda **k: bs.mark_fine_window_backselect(model, b, **k)),
                          ("backselect", lambda **k: bs.backselect(model, table, **k))):
            with pytest.raises(ValueError, match=re.escape("%s: %s" % (who, text))):
                call(**kw)
    with pytest.raises(ValueError, match="mark_players_wide"):
        bs.mark_backselect(model, b, players="nucleosomes")
    with pytest.raises(ValueError, match=r"backselect: coalitions has shape \(1, 6, 2\)"):
        bs.backselect(model, torch.zeros(1, 6, 2))
    with pytest.raises(ValueError, match="backselect: coalitions has shape"):
        bs.backselect(model, torch.zeros(1, 1 << 17, 2))      # P > 16
    with pytest.raises(RuntimeError, match="backselect: the model is not on a GPU"):
        bs.backselect(model, table)
    with pytest.raises(RuntimeError, match="call .cuda"):
        bs.mark_backselect(model, b)
    # the command line: options without their output, a bad value, the donor output without the donor's signals
    base = ["-m", str(tmp_path / "meta.csv"), "-d", str(tmp_path), "-o", str(tmp_path / "p.csv")]
    out = str(tmp_path / "out.npz")
    for extra in (["--backselect-mode", "forward"], ["--backselect-frac", "0.5"], ["--mark-backselect-players", "cells"],
                  ["--mark-donor-backselect-out", out], ["--mark-backselect-out", out, "--backselect-frac", "nan"],
                  ["--mark-backselect-out", out, "--backselect-mode", "sideways"], ["--mark-backselect-out", out, "--mark-backselect-players", "genes"],
                  ["--mark-donor-backselect-out", out, "--donor-npy-dir", str(tmp_path), "--mark-scale", "0.5"]):
        with pytest.raises(SystemExit) as e:
            predict.main(base + extra)
        assert e.value.code == 2, extra
    for extra in (["--mark-backselect-out", out, "--backselect-mode", "forward", "--backselect-frac", "0.5", "--mark-scale", "0.5"],
                  ["--mark-donor-backselect-out", out, "--donor-npy-dir", str(tmp_path)]):
        with pytest.raises(FileNotFoundError):      # accepted by the parser: the run fails on the missing metadata file
            predict.main(base + extra)
