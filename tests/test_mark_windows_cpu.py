"""The window game, host side (no GPU): the edited features of a coalition equal binning the raw signal edited inside the windows of
the absent players (scale rule: within the scan's tolerance; donor rule: bit for bit); the oracle reproduces the reference's logits on
such edited raw files (golden); attribution.window_players; the C ABI declares, exports and mirrors the three entry points and
cf_mark_window_opts; the predict parser; the walker's genomic coordinates for both strands."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from chromoformer_amd import _lib
from chromoformer_amd.attribution import window_player_coordinates, window_players
from oracle import chromoformer_oracle as orc
from oracle import dataset_oracle as dso
from tests import scan_oracle as so
from tests import window_oracle as wo
from tests.helpers import GOLDEN
from tests.test_perturbation_scan_cpu import BINS, NB, F, _binned, _raw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cf_mark_window_coalitions", "cf_mark_window_shapley", "cf_mark_window_shapley_sampled")
TOL = 3e-7      # the scan CPU test's measured error of the rule against binning (tests/test_perturbation_scan_cpu.py)


def _two_absent(g):
    """Three players on the promoter, the first two ABSENT and overlapping in coarse bin g + 2 and in mark 4; the third present."""
    players = [((1, 4), (0,), (g, min(g + 3, 20))), ((4, 6), (0,), (min(g + 2, 19), min(g + 4, 20))), (tuple(range(F)), (0,), (0, 20))]
    return players, 0b100


def _edited_raw(raw, players, word, col0, ncols, scale=None, donor=None):
    """The raw region with, per coarse bin, the samples of the marks gone there scaled ONCE (or replaced by the donor's) -> float32."""
    x = raw.astype(np.float32)
    table = wo.gone_table(players, word, 1, 20)
    for g in range(20):
        lo, hi = col0 + g * BINS[0], col0 + min((g + 1) * BINS[0], ncols)
        if table[0][g] and lo < hi:
            ms = sorted(table[0][g])
            if donor is None:
                x[ms, lo:hi] *= np.float32(scale)
            else:
                x[ms, lo:hi] = donor.astype(np.float32)[ms, lo:hi]
    return x


def _worst(raw, strand, window, donor_raw=None):
    """max |edited features - binning of the edited signal| over window placements, scales and resolutions of one promoter (scale rule,
    evaluated in fp64 on the fp32 features as the scan's test does); under the donor rule the fp32 features must be bit-equal."""
    col0, ncols = (0, raw.shape[1]) if window is None else (20000 - window // 2, window)
    base = _binned(raw, strand, window)
    n_c = -(-ncols // BINS[0])
    flip = [strand != "+"]
    worst = 0.0
    for g in sorted({0, max(n_c - 3, 0), max(n_c - 1, 0), 16}):
        players, word = _two_absent(g)
        if donor_raw is None:
            for s in (0.0, 2.5):
                got = wo.edited_batch(base, players, word, s, flip=flip, dtype=torch.float64)
                x = _edited_raw(raw, players, word, col0, ncols, scale=s)
                for bs, L in zip(BINS, NB):
                    ref = dso.region(x, bs, L, strand, window)[0].t().double()
                    worst = max(worst, (got["promoter_feats"][bs][0, 0] - ref).abs().max().item())
        else:
            donor = _binned(donor_raw, strand, window)
            got = wo.edited_batch(base, players, word, donor=donor, flip=flip)
            x = _edited_raw(raw, players, word, col0, ncols, donor=donor_raw)
            for bs, L in zip(BINS, NB):
                ref = dso.region(x, bs, L, strand, window)[0].t()
                assert torch.equal(got["promoter_feats"][bs][0, 0], ref), (g, bs)
                if g < n_c:
                    assert not torch.equal(ref, base["promoter_feats"][bs][0, 0])
    return worst


@pytest.mark.parametrize("length", [100, 1999, 2000, 2001, 7300, 12345, 39901, 40000])
@pytest.mark.parametrize("strand", ["+", "-"])
def test_edited_features_equal_binning_the_edited_signal(length, strand):
    worst = _worst(_raw(length, length), strand, None)
    print("length %d strand %s: worst %.2e (tolerance %.1e)" % (length, strand, worst, TOL))
    assert worst <= TOL
    _worst(_raw(length, length), strand, None, donor_raw=_raw(length, length + 1))


def test_a_narrowed_mirrored_promoter():
    raw = _raw(40000, 7)
    worst = _worst(raw, "-", 39000)
    print("narrowed '-' promoter: worst %.2e (tolerance %.1e)" % (worst, TOL))
    assert worst <= TOL
    _worst(raw, "-", 39000, donor_raw=_raw(40000, 8))
    # the last genomic window (half a coarse bin) sits in the FIRST stored rows; the unmirrored mapping edits other rows
    base = _binned(raw, "-", 39000)
    players = [((1, 4), (0,), (19, 20))]
    got = wo.edited_batch(base, players, 0, 0.0, flip=[True])
    ch = (got["promoter_feats"][500][0, 0] != base["promoter_feats"][500][0, 0]).any(-1).nonzero().flatten().tolist()
    assert ch and set(ch) <= {1, 2}, ch
    wrong = wo.edited_batch(base, players, 0, 0.0, flip=[False])
    assert not torch.equal(wrong["promoter_feats"][500], got["promoter_feats"][500])


def test_gone_table_and_the_identities_of_the_definition():
    players = [((0, 1), (0, 1), (2, 7)), ((1, 2), (0,), (5, 12)), ((3,), (2,), (0, 20))]
    t = wo.gone_table(players, 0b100, 3, 20)
    assert t[0][1] == set() and t[0][2] == {0, 1} and t[0][5] == {0, 1, 2} and t[0][7] == {1, 2} and t[0][12] == set()
    assert t[1][4] == {0, 1} and t[1][8] == set() and not any(t[2])
    assert not any(any(row) for row in wo.gone_table(players, 0b111, 3, 20))
    # (a) one absent single-region player = the scan's window; (b) windows [0, W) = the whole-region game (padded rows hold zeros)
    batch = orc.synthetic_batch(2, seed=3, regime="realistic")
    one = [((1, 4), (2,), (3, 6)), ((0,), (0,), (0, 20))]
    got = wo.edited_batch(batch, one, 0b10, 2.5)
    _, rows = so.scan_rows(batch, region=2, scale=2.5, width=3, mark_sets=[(1, 4)], variants=[1 + 3])
    for b in BINS:
        assert torch.equal(got["pcre_feats"][b], rows["pcre_feats"][b]) and torch.equal(got["promoter_feats"][b], batch["promoter_feats"][b])
    from tests import mark_oracle as mo
    whole = [((0, 5), (0, 3), (0, 20)), ((5, 6), (3, 8), (0, 20))]
    marks = np.array([0b100001, 0b1100000], dtype=np.uint32)
    regions = np.array([0b1001, 0b100001000], dtype=np.uint32)
    P = orc.init_params(None, 42, False)
    with torch.no_grad():
        ref = mo.oracle_mark_coalitions(P, batch, (marks, regions), [0b01], 0.0)[:, 0]
        mine = orc.forward(P, wo.edited_batch(batch, whole, 0b01, 0.0))
    assert torch.equal(mine, ref)


def test_oracle_logits_equal_the_golden():
    """The reference's own dataset and models on raw files edited inside the windows (tests/golden/make_mark_window_goldens.py)
    against the window oracle + orc.forward on the unedited dataset, at the project's logit bound."""
    import tempfile
    g = np.load(os.path.join(GOLDEN, "mark_windows.npz"))
    assert os.path.getsize(os.path.join(GOLDEN, "mark_windows.npz")) <= os.path.getsize(os.path.join(GOLDEN, "mark_coalitions.npz"))
    table = g["players"].astype(np.int64)
    with tempfile.TemporaryDirectory() as tmp:
        ds = so.scan_dataset(tmp, w_prom=int(g["w_prom"]))
        genes = [str(x) for x in g["genes"]]
        base = so.dataset_batch(ds, genes)
        flips = [ds.genes[x]["tss"][2] != "+" for x in genes]
        assert any(flips) and not all(flips)
        for head, regression in (("clf", False), ("reg", True)):
            P = orc.init_params(None, 42, regression)
            with torch.no_grad():
                assert (orc.forward(P, base) - torch.from_numpy(g["base." + head])).abs().max().item() <= 1e-4
            for k, scale in enumerate(g["scales"].tolist()):
                rows = table[table[:, 0] == k]
                players = [(tuple(f for f in range(7) if m >> f & 1), tuple(r for r in range(9) if rs >> r & 1), (int(lo), int(hi)))
                           for _, m, rs, lo, hi, _ in rows]
                word = sum(int(p) << i for i, p in enumerate(rows[:, 5]))
                with torch.no_grad():
                    lg = orc.forward(P, wo.edited_batch(base, players, word, float(scale), flip=flips))
                d = (lg - torch.from_numpy(g[head][k])).abs().max().item()
                print(head, "case", k, "P", len(players), "oracle vs reference %.2e" % d)
                assert d <= 1e-4, (head, k, d)
                assert not np.array_equal(g[head][k], g["base." + head])      # the edit moves the prediction


def test_window_players():
    m, r, lo, hi, names = window_players("promoter", 7, 8, 20)
    ref = wo.players_promoter(7, 20)
    assert len(m) == 20 and m.dtype == r.dtype == np.uint32 and lo.dtype == hi.dtype == np.int32
    assert m.tolist() == [0x7F] * 20 and r.tolist() == [1] * 20 and list(zip(lo.tolist(), hi.tolist())) == [w for _, _, w in ref]
    assert names[4] == "promoter[4:5]" and window_players("promoter", 7, 8, 20, 2)[4][2] == "promoter[4:6]"
    m, r, lo, hi, names = window_players("promoter", 7, 8, 20, 3)      # 7 windows, the last one narrower
    assert len(m) == 7 and (lo[-1], hi[-1]) == (18, 20) and names[-1] == "promoter[18:20]"
    m, r, lo, hi, names = window_players("promoter_cells", 7, 8, 20, 2)
    ref = wo.players_promoter_cells(7, 20, 2)
    assert len(m) == 70 and m.tolist() == [1 << ms[0] for ms, _, _ in ref] and set(r.tolist()) == {1}
    assert list(zip(lo.tolist(), hi.tolist())) == [w for _, _, w in ref] and names[2 * 7 + 3] == "mark3@promoter[4:6]"
    m, r, lo, hi, names = window_players("regions", 7, 8, 20, 2)
    ref = wo.players_regions(7, 8, 20, 2)
    assert len(m) == 90 and r.tolist() == [1 << rs[0] for _, rs, _ in ref] and list(zip(lo.tolist(), hi.tolist())) == [w for _, _, w in ref]
    assert names[0] == "promoter[0:2]" and names[2 * 10] == "pcre1[0:2]" and names[-1] == "pcre7[18:20]"
    assert len(window_players("regions", 7, 16, 20, 3)[0]) == 119
    m, r, lo, hi, names = window_players([((1, 4), (0, 2), (3, 6)), ([0], [8], [0, 20])], 7, 8, 20)
    assert m.tolist() == [0b10010, 1] and r.tolist() == [0b101, 1 << 8] and lo.tolist() == [3, 0] and hi.tolist() == [6, 20]
    assert names == ["marks(1,4)@regions(0,2)[3:6]", "marks(0)@regions(8)[0:20]"]
    for spec, kw, needle in (("promoter_cells", dict(width=1), "140 players.*larger width"), ("regions", dict(width=1), "180 players.*larger width"),
                             ("cells", {}, "choose from"), ("promoter", dict(width=0), "width = 0"), ([], {}, "0 players"),
                             ([((0,), (0,), (0, 1))] * 129, {}, "129 players"), ([((), (0,), (0, 1))], {}, "player 0 is empty"),
                             ([((0,), (), (0, 1))], {}, "player 0 is empty"), ([((7,), (0,), (0, 1))], {}, "n_feats"),
                             ([((0,), (9,), (0, 1))], {}, "i_max"), ([((0,), (0,), (-1, 1))], {}, r"window \[-1, 1\)"),
                             ([((0,), (0,), (0, 21))], {}, r"window \[0, 21\)"), ([((0,), (0,), (5, 5))], {}, r"player 0 has the window \[5, 5\)"),
                             ([((0,), (0,))], {}, "triples"), (7, {}, "triples")):
        with pytest.raises(ValueError, match="window_players: .*" + needle):
            window_players(spec, 7, 8, 20, **kw)
    with pytest.raises(ValueError, match="window_players: W = 0"):
        window_players("promoter", 7, 8, 0)


def test_abi_symbols_struct_and_null_handle():
    hdr = open(os.path.join(ROOT, "include", "chromoformer_hip.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert ("int cf_mark_window_coalitions(cf_handle* h, const cf_batch* batch, const cf_mark_window_opts* opts, const uint32_t* keep, int n_coal, "
            "float* logits, void* stream);") in flat
    assert "int cf_mark_window_shapley(cf_handle* h, const cf_batch* batch, const cf_mark_window_opts* opts, float* phi, float* logits_all, void* stream);" in flat
    assert ("int cf_mark_window_shapley_sampled(cf_handle* h, const cf_batch* batch, const cf_mark_window_opts* opts, const uint8_t* perms, int n_perm, "
            "float* phi, float* se, float* logits_rows, void* stream);") in flat
    assert set(NAMES) <= set(_lib.SYMBOLS)
    o = _lib.cf_mark_window_opts
    # int n_players (pad); five pointers; float scale (pad); two pointer arrays
    assert C.sizeof(o) == 8 + 5 * 8 + 8 + 2 * 8 * _lib.MAX_RES == 104 and "104 bytes" in hdr
    assert [getattr(o, n).offset for n, _ in o._fields_] == [0, 8, 16, 24, 32, 40, 48, 56, 80]
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct cf_mark_window_opts \{(.*?)\} cf_mark_window_opts;", hdr, re.S).group(1), flags=re.S)
    assert re.findall(r"(\w+)(?:\[CF_MAX_RES\])?;", body) == [n for n, _ in o._fields_]
    assert [C.sizeof(s) for s in (_lib.cf_mark_opts, _lib.cf_mark_donor_opts, _lib.cf_mark_wide_opts)] == [32, 72, 80]      # the siblings keep theirs
    for name in NAMES:
        res, args = _lib.SYMBOLS[name]
        assert res is C.c_int and args[2] == C.POINTER(o)
    assert [len(_lib.SYMBOLS[n][1]) for n in NAMES] == [7, 6, 9]
    L = _lib.lib()
    assert L.cf_abi_version() == 1
    assert L.cf_mark_window_coalitions(None, None, None, None, 0, None, None) != 0
    assert L.cf_last_error() == b"cf_mark_window_coalitions: null handle"
    assert L.cf_mark_window_shapley(None, None, None, None, None, None) != 0
    assert L.cf_last_error() == b"cf_mark_window_shapley: null handle"
    assert L.cf_mark_window_shapley_sampled(None, None, None, None, 0, None, None, None, None) != 0
    assert L.cf_last_error() == b"cf_mark_window_shapley_sampled: null handle"
    from chromoformer_amd.net import ChromoformerBase
    for name in ("mark_window_coalitions", "mark_window_shapley", "mark_window_shapley_sampled", "mark_window_shapley_dataset"):
        assert callable(getattr(ChromoformerBase, name))


def test_parser(tmp_path):
    from chromoformer_amd import predict
    base = ["-m", str(tmp_path / "meta.csv"), "-d", str(tmp_path), "-o", str(tmp_path / "p.csv")]
    out = str(tmp_path / "out.npz")
    a = predict.build_parser().parse_args(base + ["--window-shapley-out", out, "--window-players", "promoter_cells", "--window-width", "2",
                                                  "--window-perms", "8", "--window-seed", "3", "--window-scale", "0.5"])
    assert (a.window_shapley_out, a.window_players, a.window_width, a.window_perms, a.window_seed, a.window_scale) == (out, "promoter_cells", 2, 8, 3, 0.5)
    b = predict.build_parser().parse_args(base)
    assert b.window_shapley_out is None and b.window_donor_shapley_out is None and b.window_players is None and b.window_width is None
    bad = [["--window-donor-shapley-out", out],                                        # needs --donor-npy-dir
           ["--window-players", "promoter"], ["--window-width", "2"], ["--window-perms", "8"], ["--window-seed", "1"], ["--window-scale", "0.5"],
           ["--window-shapley-out", out, "--window-players", "cells"],
           ["--window-shapley-out", out, "--window-width", "0"],
           ["--window-shapley-out", out, "--window-perms", "0"],
           ["--window-shapley-out", out, "--window-scale", "-1"],
           ["--window-shapley-out", out, "--window-players", "promoter_cells"],      # 140 players at width 1
           ["--window-shapley-out", out, "--mark-scale", "0.5"],                       # the mark game's scale does not apply
           ["--window-donor-shapley-out", out, "--donor-npy-dir", str(tmp_path), "--window-scale", "0.5"]]      # the donor rule has no scale
    for extra in bad:
        with pytest.raises(SystemExit) as e:
            predict.main(base + extra)
        assert e.value.code == 2, extra
    for extra in (["--window-shapley-out", out, "--window-players", "regions", "--window-width", "2", "--window-scale", "2"],
                  ["--window-donor-shapley-out", out, "--donor-npy-dir", str(tmp_path)]):
        with pytest.raises(FileNotFoundError):
            predict.main(base + extra)


def test_walker_coordinates_for_both_strands(tmp_path):
    """window_player_coordinates against the definition: zero the raw samples of the player's genomic window [start, end) and bin; the
    rows that change are the rows the oracle edits with flip from the strand."""
    ds = so.scan_dataset(str(tmp_path), w_prom=39000)
    plus = [x for x in ds.target_genes if ds.genes[x]["tss"][2] == "+" and ds.genes[x]["pcres"]][0]
    minus = [x for x in ds.target_genes if ds.genes[x]["tss"][2] == "-" and ds.genes[x]["pcres"]][0]
    game = window_players([(range(7), (0,), (0, 2)), (range(7), (0,), (18, 20)), (range(7), (1,), (0, 1)), (range(7), (1,), (19, 20)),
                           (range(7), (0, 1), (1, 3)), (range(7), (8,), (0, 20))], 7, 8, 20)
    triples = [(tuple(range(7)), rs, w) for rs, w in (((0,), (0, 2)), ((0,), (18, 20)), ((1,), (0, 1)), ((1,), (19, 20)), ((0, 1), (1, 3)), ((8,), (0, 20)))]
    for gid in (plus, minus):
        chrom, tss, strand = ds.genes[gid]["tss"]
        start = tss - 20000 + 500
        c, s, e = ds.genes[gid]["pcres"][0]
        n_pc = -(-(e - s) // 2000)
        assert n_pc < 20
        regions = {0: (chrom, start, start + 39000), 1: (c, s, e)}      # (the gene's other pCREs left out: slot 7 reads as a dummy)
        windows, null = window_player_coordinates(game, regions, {0: 20, 1: n_pc}, 2000)
        assert windows[0] == [(0, chrom, start, start + 4000)] and windows[1] == [(0, chrom, start + 36000, start + 39000)]
        assert windows[2] == [(1, c, s, min(s + 2000, e))] and windows[3] == [] and windows[5] == []
        assert windows[4] == [(0, chrom, start + 2000, start + 6000)] + ([(1, c, s + 2000, min(s + 6000, e))] if n_pc > 1 else [])
        assert null.tolist() == [False, False, False, True, False, True]
        base = so.dataset_batch(ds, [gid], torch.float64)
        for p in (0, 1, 2):
            rho, _, w0, w1 = windows[p][0]
            r0 = regions[rho][1]
            assert (w0 - r0) % 2000 == 0
            pert = so.batch_from_scaled_raw(ds, [gid], rho, (w0 - r0) // 2000, -(-(w1 - w0) // 2000), range(7), 0.0, torch.float64)
            mine = wo.edited_batch(base, [triples[p]], 0, 0.0, flip=[strand == "-"], dtype=torch.float64)
            for b in BINS:
                for key in ("promoter_feats", "pcre_feats"):
                    assert (mine[key][b] - pert[key][b]).abs().max().item() <= TOL, (gid, p, b, key)
                    changed = (mine[key][b] != base[key][b]).any().item()
                    assert changed == (key == ("promoter_feats" if rho == 0 else "pcre_feats")), (gid, p, b, key)
