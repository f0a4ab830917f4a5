"""Pairwise Shapley interaction indices on the GPU (cf_shapley_interactions_from_rows, the five cf_*_shapley_interactions entry points,
the ChromoformerBase methods of the same names, the `interactions=` option of the dataset generators, predict --*-interactions-out):
a second reduction (k_shapley_pairs) of the [B, 2^P, n_out] table the exact Shapley calls reduce with k_shapley.

  * the operator on random tables at every subset count the kernel treats differently, against the float64 definition within the fp32
    rounding bound, against the fp32 restatement of the kernel bit for bit, symmetric, the diagonals, call after call;
  * each of the five games: the sibling's table and phi bit for bit, the operator on that table bit for bit, the Shapley-Taylor
    efficiency gap, whatever max_batch is;
  * null players (a dummy slot, a window past the real bins, a donor that agrees with the gene) exactly 0, the other pairs not;
  * P = 2 against mark_epistasis within rounding;
  * every refusal by name with nothing launched, the launch count, a pending backward, no side effects on training, the generators and
    the CLI.

The shapes are those of tests/test_mark_coalitions_gpu.py (the seed-42 classifier at max_batch = 4, the three scan genes) and the
i_max = 3 model of tests/test_pcre_coalitions_gpu.py."""
import ctypes as C
import types

import numpy as np
import pandas as pd
import pytest
import torch

from chromoformer_amd import _lib
from chromoformer_amd.attribution import fine_window_players, mark_players, window_players
from oracle import chromoformer_oracle as orc
from tests import donor_oracle as do
from tests import scan_oracle as so
from tests.coalition_oracle import shapley_fp64
from tests.interaction_oracle import pair_index_fp32, pair_index_fp64
from tests.test_input_grads_gpu import _model
from tests.test_mark_coalitions_gpu import GENES, OVERLAP
from tests.test_mark_donor_gpu import _dev, _feats
from tests.test_mark_fine_windows_cpu import PLAYERS
from tests.test_mark_fine_windows_gpu import ZOOMS
from tests.test_mark_fine_windows_gpu import _raw_opts as _fine_opts
from tests.test_mark_windows_gpu import THREE
from tests.test_mark_windows_gpu import _raw_opts as _window_opts
from tests.test_pcre_coalitions_gpu import U, _dummies, _gamma
from tests.test_pcre_coalitions_gpu import _model as _pcre_model

pytestmark = pytest.mark.gpu
ALL = tuple(range(7))
INDICES = ("sii", "sti")


def _args(batch):
    return tuple(batch[k] for k in so.KEYS)


def _gamma_pairs(P):
    """n u / (1 - n u), n = 2^(P - 2) + 5, times scale = sum_S w (|a| + |b| + |c| + |d|): every one of the four table entries of a
    delta passes through at most three rounded subtractions; the weight is rounded once; the product once; a pair's sum has 2^(P - 2)
    terms, so whatever the order at most 2^(P - 2) rounded additions lie on a term's way to the result.  3 + 1 + 1 + 2^(P - 2)
    factors (1 + e), |e| <= u, bound a term's relative error by gamma_n (Higham, Lemma 3.1), as _gamma does for k_shapley."""
    n = 2 ** (P - 2) + 5
    return n * U / (1 - n * U)


def _sti_gap_bound(v, P):
    """The bound of |info["delta"]| under sti from the call's own table v [B, 2^P, n_out] (float64): the exact sum of the diagonal and
    the upper triangle IS v(N) - v(0), so the gap is rounding alone -- each entry's own error (gamma_pairs scale off the diagonal, u
    (|v_i| + |v_0|) on it), the K = P (P + 1) / 2 terms' fp32 sum in any order (gamma_K sum |entry|), and the two roundings of
    logits - absent and of the final subtraction (4 u max |v| covers them)."""
    I, scale = pair_index_fp64(v, "sti")
    upper = np.triu(np.ones((P, P), dtype=bool))
    own = np.where(np.eye(P, dtype=bool)[None, :, :, None], U * scale, _gamma_pairs(P) * scale)[:, upper].sum(1)
    K = P * (P + 1) // 2
    return own + K * U / (1 - K * U) * (np.abs(I[:, upper]).sum(1) + own) + 4 * U * np.abs(v).max(1)


def _check_table(inter, rows, index, phi=None):
    """inter [B, P, P, n_out] of `rows` [B, 2^P, n_out] (host tensors): the float64 definition within the bound, off the diagonal the
    fp32 restatement bit for bit, exactly symmetric, the diagonal (phi bit for bit where the game's k_shapley result is given, else within k_shapley's
    bound; v({i}) - v(0) bit for bit under sti)."""
    v = rows.numpy()
    P = v.shape[1].bit_length() - 1
    got = inter.numpy()
    assert got.shape == (v.shape[0], P, P, v.shape[2]) and got.dtype == np.float32
    I64, scale = pair_index_fp64(v, index)
    off = ~np.eye(P, dtype=bool)
    err = np.abs(got.astype(np.float64) - I64)[:, off]
    bound = (_gamma_pairs(P) * scale)[:, off]
    print("P %d %s: max err %.3e, max bound %.3e, max err / bound %.3f" % (P, index, err.max(), bound.max(), (err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all(), (err.max(), bound.max())
    assert torch.equal(inter, inter.transpose(1, 2))
    assert np.array_equal(got[:, off], pair_index_fp32(v, index)[:, off])
    diag = got[:, np.arange(P), np.arange(P)]
    if index == "sti":
        assert np.array_equal(diag, v[:, 1 << np.arange(P)] - v[:, :1])
    elif phi is not None:
        assert np.array_equal(diag, phi.numpy())
    else:
        phi64, pscale = shapley_fp64(v)
        assert (np.abs(diag.astype(np.float64) - phi64) <= _gamma(P) * pscale).all()


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """The three scan genes and the donor cell type: host and device batches and the promoter flips, built once, never written."""
    ds = so.scan_dataset(str(tmp_path_factory.mktemp("interactions")), w_prom=39000)
    dn = do.donor_dataset(ds.npy_dir, str(tmp_path_factory.mktemp("donor")), do.DONOR_SEED, w_prom=39000)
    cpu, dcpu = so.dataset_batch(ds, GENES), so.dataset_batch(dn, GENES)
    flips = [ds.genes[g]["tss"][2] != "+" for g in GENES]
    return types.SimpleNamespace(cpu=cpu, dev=_dev(cpu), dcpu=dcpu, ddev=_dev(dcpu), flips=flips)


@pytest.fixture(scope="module")
def models():
    """The seed-42 classifier at max_batch = 4 and 7 and the seed-42 regressor at 4."""
    P = orc.init_params(None, 42, False)
    return types.SimpleNamespace(small=_model(None, False, P, 4), seven=_model(None, False, P, 7),
                                 reg=_model(None, True, orc.init_params(None, 42, True), 4))


@pytest.fixture(scope="module")
def pcre():
    """The i_max = 3 model of tests/test_pcre_coalitions_gpu.py at max_batch 5 and 7, 5 genes with [0, 0, 0, 2, 3] dummy slots."""
    cfg = orc._cfg(dict(i_max=3))
    batch = orc.synthetic_batch(5, cfg=cfg, seed=13, regime="realistic")
    P = orc.init_params(cfg, 3, False)
    ms = []
    for cap in (5, 7):
        m = _pcre_model(cfg, B=cap, seed=3)
        m.load_state_dict(P)
        ms.append(m)
    return types.SimpleNamespace(batch=batch, five=ms[0], seven=ms[1])


@pytest.mark.parametrize("n_out", [1, 2])
@pytest.mark.parametrize("P", [2, 3, 9, 10, 11, 16])
def test_operator_on_random_tables(models, P, n_out):
    """B = 2.  2^(P - 2) subsets per pair: one (P = 2); fewer than the 256 threads (3, 9); exactly 256 (10); two strides (11); 16,384 with
    bits 0 and 15 and adjacent bits among the pairs (16)."""
    model = models.small if n_out == 2 else models.reg
    g = torch.Generator().manual_seed(100 * P + n_out)
    rows = torch.randn(2, 1 << P, n_out, generator=g) * 3 + torch.randn(2, 1, n_out, generator=g)
    dev = rows.cuda()
    for index in INDICES:
        inter = model.shapley_interactions(dev, index=index)
        again = model.shapley_interactions(dev, index=index)
        torch.cuda.synchronize()
        assert not inter.requires_grad and torch.equal(inter, again)
        _check_table(inter.cpu(), rows, index)
    assert torch.equal(model.shapley_interactions(rows, index="sti").cpu(), inter.cpu())      # (a host table is moved)


def _game_checks(call, sibling, absent, P, models_pair, operator_model, players):
    """call(model, index, **kw) -> (inter, info) and sibling(model) -> (phi, info with the table) on two models that differ in max_batch."""
    first, second = models_pair
    phi, sinfo = sibling(first)
    table = sinfo["coalitions"].cpu()
    for index in INDICES:
        inter, info = call(first, index, return_coalitions=True)
        want = ["coalitions", absent, "index", "logits", "phi"] + (["players"] if players else []) + (["delta"] if index == "sti" else [])
        assert sorted(info) == sorted(want) and info["index"] == index and not inter.requires_grad
        assert torch.equal(info["coalitions"].cpu(), table)
        assert torch.equal(info["phi"].cpu(), phi.cpu())
        assert torch.equal(info["logits"].cpu(), table[:, -1]) and torch.equal(info[absent].cpu(), table[:, 0])
        if players:
            assert info["players"] == sinfo["players"]
        assert torch.equal(inter, operator_model.shapley_interactions(info["coalitions"], index=index))
        _check_table(inter.cpu(), table, index, phi=phi.cpu() if index == "sii" else None)
        if index == "sti":
            gap, bound = np.abs(info["delta"].cpu().numpy()), _sti_gap_bound(table.numpy().astype(np.float64), P)
            print("sti delta: max %.3e, max bound %.3e" % (gap.max(), bound.max()))
            assert gap.shape == bound.shape and (gap <= bound).all(), (gap.max(), bound.max())
        other, oinfo = call(second, index)
        assert "coalitions" not in oinfo and torch.equal(other.cpu(), inter.cpu()) and torch.equal(oinfo["phi"].cpu(), phi.cpu())
    return inter.cpu(), table


def test_pcre_game(pcre):
    a = _args(pcre.batch)
    inter, table = _game_checks(lambda m, index, **kw: m.pcre_shapley_interactions(*a, index=index, **kw),
                                lambda m: m.pcre_shapley(*a, return_coalitions=True), "promoter_only", 3, (pcre.five, pcre.seven), pcre.five, False)
    dummy = _dummies(pcre.batch)      # a dummy slot is a null player: its row and column are exact zeros, the live pairs are not
    assert dummy.sum(1).tolist() == [0, 0, 0, 2, 3]
    for index in INDICES:
        x = pcre.five.pcre_shapley_interactions(*a, index=index)[0].cpu()
        null = dummy[:, :, None] | dummy[:, None, :]
        assert bool((x[null] == 0).all()) and bool((x[~null] != 0).any(-1).all()), index


def test_mark_game(data, models):
    a = _args(data.dev)
    _game_checks(lambda m, index, **kw: m.mark_shapley_interactions(*a, index=index, **kw),
                 lambda m: m.mark_shapley(*a, return_coalitions=True), "erased", 7, (models.small, models.seven), models.small, True)
    inter = models.small.mark_shapley_interactions(*a, scale=0.5)[0].cpu()
    assert inter.shape == (3, 7, 7, 2) and bool((inter != 0).any(-1).all())
    for p in (models.small.pack_batch(data.dev),):      # the packed form
        assert torch.equal(models.small.mark_shapley_interactions(p, scale=0.5)[0].cpu(), inter)


def test_mark_donor_game(data, models):
    a, don = _args(data.dev), _feats(data.ddev)
    _game_checks(lambda m, index, **kw: m.mark_donor_shapley_interactions(*a, donor=don, index=index, **kw),
                 lambda m: m.mark_donor_shapley(*a, donor=don, return_coalitions=True), "donor", 7, (models.small, models.seven), models.small, True)


def test_mark_window_game(data, models):
    a = _args(data.dev)
    for rule, absent in ((dict(scale=2.5), "erased"), (dict(donor=_feats(data.ddev)), "donor")):
        kw0 = dict(players=THREE, flip=data.flips, **rule)
        inter, table = _game_checks(lambda m, index, **kw: m.mark_window_shapley_interactions(*a, index=index, **kw0, **kw),
                                    lambda m: m.mark_window_shapley(*a, return_coalitions=True, **kw0), absent, 3, (models.small, models.seven),
                                    models.small, True)
        # pCRE slot 7 is a dummy slot of gene 2: player 2 is null there; the two halves of the promoter are live in every gene
        assert bool((inter[2, 2] == 0).all()) and bool((inter[2, :, 2] == 0).all()) and bool((inter[:, :2, :2] != 0).any(-1).all())
    with pytest.raises(ValueError, match="17 players"):
        models.small.mark_window_shapley_interactions(*a, players=[(ALL, (0,), (g, g + 1)) for g in range(17)])


def test_mark_fine_game(data, models):
    a = _args(data.dev)
    for rule, absent in ((dict(scale=0.0), "erased"), (dict(donor=_feats(data.ddev)), "donor")):
        kw0 = dict(players=PLAYERS[:3], start=ZOOMS[0][0], lengths=ZOOMS[0][1], flip=data.flips, **rule)
        _game_checks(lambda m, index, **kw: m.mark_fine_window_shapley_interactions(*a, index=index, **kw0, **kw),
                     lambda m: m.mark_fine_window_shapley(*a, return_coalitions=True, **kw0), absent, 3, (models.small, models.seven),
                     models.small, True)
    inter, info = models.small.mark_fine_window_shapley_interactions(*a, return_feats=True, **kw0)
    assert sorted(info["feats"]) == [100, 500, 2000] and info["feats"][100].shape[:2] == (3, 8)


def test_null_players_of_the_fine_game_are_exact_zeros(data, models):
    a, small = _args(data.dev), models.small
    # windows past bin 390, beside a real one (start 350: [350, 355), [390, 397), [395, 410))
    players = [(ALL, (0, 5)), ((1, 4), (40, 47)), (ALL, (45, 60))]
    for index in INDICES:
        inter = small.mark_fine_window_shapley_interactions(*a, players=players, start=350, flip=data.flips, index=index)[0].cpu()
        off = ~torch.eye(3, dtype=torch.bool)
        assert bool((inter[:, off] == 0).all()) and bool((inter[:, 0, 0] != 0).all()), index
        assert bool((inter[:, 1, 1] == 0).all()) and bool((inter[:, 2, 2] == 0).all())
    # a donor equal to the gene inside a player: genomic finest bins [40, 60) of the '+' strand gene 1
    don = {b: t.clone() for b, t in data.ddev["promoter_feats"].items()}
    for b in (2000, 500, 100):
        R, q = b // 100, so.extent(so.centre_row(data.cpu["promoter_pad_masks"][b], 3, 40000 // b)[1])[0]
        don[b][1, 0, q + 40 // R:q - (-60 // R)] = data.dev["promoter_feats"][b][1, 0, q + 40 // R:q - (-60 // R)]
    players = [(ALL, (43, 57)), ((2,), (100, 110)), ((0, 3), (20, 30))]
    for index in INDICES:
        inter, info = small.mark_fine_window_shapley_interactions(*a, players=players, flip=data.flips, donor=(don, data.ddev["pcre_feats"]), index=index)
        inter = inter.cpu()
        assert bool((inter[1, 0, 1:] == 0).all()) and bool((inter[1, 1:, 0] == 0).all()), index      # the null player, lower index of its pairs
        assert bool((inter[1, 1, 2] != 0).any()) and bool((inter[0][off] != 0).any(-1).all()), index
        assert bool((info["phi"][1, 0] == 0).all())
    # ... and as the higher-indexed player of its pairs
    players = [((2,), (100, 110)), ((0, 3), (20, 30)), (ALL, (43, 57))]
    inter = small.mark_fine_window_shapley_interactions(*a, players=players, flip=data.flips, donor=(don, data.ddev["pcre_feats"]))[0].cpu()
    assert bool((inter[1, 2] == 0).all()) and bool((inter[1, :, 2] == 0).all()) and bool((inter[1, 0, 1] != 0).any())


def test_two_players_against_mark_epistasis(data, models):
    """P = 2: one subset, weight 1 under both indices; (a - b) - (c - d) against k_epistasis's ((a - b) - c) + d: three roundings each,
    each at most u times a partial result no larger than |a| + |b| + |c| + |d|: within 4 u of that sum (not bit for bit)."""
    a = _args(data.dev)
    eps = models.small.mark_epistasis(*a, players=OVERLAP)[0].cpu()
    for index in INDICES:
        inter, info = models.small.mark_shapley_interactions(*a, players=OVERLAP, index=index, return_coalitions=True)
        v = info["coalitions"].cpu().abs().sum(1)
        assert inter.shape == (3, 2, 2, 2) and bool(((inter.cpu()[:, 0, 1] - eps[:, 0, 1]).abs() <= 4 * U * v).all()), index
        assert bool((inter.cpu()[:, 0, 1] != 0).any(-1).all())


def test_launch_contract(data):
    """fwd = the sibling's rows (ceil(B 2^P / max_batch) (1 + n_fwd); the pCRE game: n_trunk + 1 + chunks (1 + n_reg_head)) plus one per
    reducer: k_shapley_pairs, and k_shapley for phi.  The operator alone: 1."""
    L = _lib.lib()
    model = _model(None, False, orc.init_params(None, 42, False), 7)
    a = _args(data.dev)
    with torch.no_grad():
        model(*a)
    n_fwd = model.launch_counts()[0]
    model.mark_shapley(*a)
    sib = model.launch_counts()[0]
    assert sib == -(-3 * 128 // 7) * (1 + n_fwd) + 1
    inter, info = model.mark_shapley_interactions(*a, return_coalitions=True)
    assert model.launch_counts()[0] == sib + 1      # the methods ask for phi: two reducers
    bs, keep_alive = model.pack_batch(data.dev)
    pm, pr, _ = mark_players("marks", 7, 8)
    o = _lib.cf_mark_opts()
    o.n_players, o.scale, o.player_marks, o.player_regions = 7, 0.0, pm.ctypes.data, pr.ctypes.data
    st = torch.cuda.current_stream().cuda_stream
    out = torch.empty(3, 7, 7, 2, device="cuda")
    assert L.cf_mark_shapley_interactions(model._handle, C.byref(bs), C.byref(o), 0, out.data_ptr(), None, None, st) == 0, L.cf_last_error()
    assert model.launch_counts()[0] == sib      # no phi: one reducer, the rows in the handle's own buffer
    assert torch.equal(out, inter)
    model.shapley_interactions(info["coalitions"])
    assert model.launch_counts()[0] == 1
    model.pcre_shapley(*a)
    sib = model.launch_counts()[0]
    model.pcre_shapley_interactions(*a, index="sti")
    assert model.launch_counts()[0] == sib + 1
    for method, kw in (("mark_window_shapley", dict(players=THREE)), ("mark_fine_window_shapley", dict(players=PLAYERS[:3], start=ZOOMS[0][0])),
                       ("mark_donor_shapley", dict(donor=_feats(data.ddev)))):
        getattr(model, method)(*a, **kw)
        sib = model.launch_counts()[0]
        getattr(model, method + "_interactions")(*a, **kw)
        assert model.launch_counts()[0] == sib + 1, method
    del keep_alive


def test_refusals_by_name_with_nothing_launched(data):
    L = _lib.lib()
    model = _model(None, False, orc.init_params(None, 42, False), 4)
    bs, keep_alive = model.pack_batch(data.dev)
    dbs, donor_alive = model.pack_batch(data.ddev)
    with torch.no_grad():
        model(*_args(data.dev))
    f0 = model.launch_counts()
    st = torch.cuda.current_stream().cuda_stream
    out = torch.full((3, 8, 8, 2), float("nan"), device="cuda")
    rows = torch.zeros(3, 256, 2, device="cuda")
    big = _lib.cf_batch.from_buffer_copy(bs)
    big.B = 5
    pm, pr, _ = mark_players("marks", 7, 8)
    dp, dc = [dbs.promoter_feats[r] for r in range(3)], [dbs.pcre_feats[r] for r in range(3)]

    def mark_opts(n_players=7, marks=pm, scale=0.0):
        o = _lib.cf_mark_opts()
        o.n_players, o.scale, o.player_marks, o.player_regions = n_players, scale, marks.ctypes.data if marks is not None else None, pr.ctypes.data
        return o, (marks,)

    def donor_opts(n_players=7, null_donor=False, **_):
        o = _lib.cf_mark_donor_opts()
        o.n_players, o.player_marks, o.player_regions = n_players, pm.ctypes.data, pr.ctypes.data
        for r in range(3):
            o.donor_promoter_feats[r], o.donor_pcre_feats[r] = dp[r], None if null_donor and r == 1 else dc[r]
        return o, ()

    wgame, fgame = window_players(THREE, 7, 8, 20), fine_window_players(PLAYERS[:3], 7, 1, 3)
    families = [(b"cf_mark_shapley_interactions", L.cf_mark_shapley_interactions, mark_opts, [(dict(n_players=0), b"n_players"), (dict(n_players=17), b"n_players"),
                                                                                         (dict(marks=None), b"null player_marks"), (dict(scale=-1.0), b"scale")]),
                (b"cf_mark_donor_shapley_interactions", L.cf_mark_donor_shapley_interactions, donor_opts, [(dict(n_players=17), b"n_players"),
                                                                                                     (dict(null_donor=True), b"null donor_promoter_feats / donor_pcre_feats[1]")]),
                (b"cf_mark_window_shapley_interactions", L.cf_mark_window_shapley_interactions, lambda **kw: _window_opts(wgame, **kw),
                 [(dict(n_players=0), b"n_players"), (dict(lo=None), b"null player_lo / player_hi"), (dict(scale=float("nan")), b"scale")]),
                (b"cf_mark_fine_shapley_interactions", L.cf_mark_fine_shapley_interactions, lambda **kw: _fine_opts(fgame, **kw),
                 [(dict(n_players=0), b"n_players"), (dict(region=9), b"region = 9 outside"), (dict(hi=None), b"null player_lo / player_hi")])]

    def refused(rc, *needles):
        err = L.cf_last_error()
        assert rc != 0 and all(n in err for n in needles), err

    for name, fn, make, bad in families:
        good, alive = make()
        refused(fn(None, C.byref(bs), C.byref(good), 0, out.data_ptr(), None, None, st), name, b"null handle")
        refused(fn(model._handle, None, C.byref(good), 0, out.data_ptr(), None, None, st), name, b"null batch")
        refused(fn(model._handle, C.byref(bs), None, 0, out.data_ptr(), None, None, st), name, b"null opts")
        refused(fn(model._handle, C.byref(big), C.byref(good), 0, out.data_ptr(), None, None, st), name, b"max_batch")
        refused(fn(model._handle, C.byref(bs), C.byref(good), 0, None, None, None, st), name, b"null inter")
        for index in (2, -1):
            refused(fn(model._handle, C.byref(bs), C.byref(good), index, out.data_ptr(), None, None, st), name, b"index = %d" % index)
        one, alive1 = make(n_players=1)
        refused(fn(model._handle, C.byref(bs), C.byref(one), 0, out.data_ptr(), None, None, st), name, b"1 player", b"at least 2")
        for kw, msg in bad:
            o, alive2 = make(**kw)
            refused(fn(model._handle, C.byref(bs), C.byref(o), 0, out.data_ptr(), None, None, st), name, msg)
    name, fn = b"cf_pcre_shapley_interactions", L.cf_pcre_shapley_interactions
    refused(fn(None, C.byref(bs), 0, out.data_ptr(), None, None, st), name, b"null handle")
    refused(fn(model._handle, None, 0, out.data_ptr(), None, None, st), name, b"null batch")
    refused(fn(model._handle, C.byref(big), 0, out.data_ptr(), None, None, st), name, b"max_batch")
    refused(fn(model._handle, C.byref(bs), 0, None, None, None, st), name, b"null inter")
    refused(fn(model._handle, C.byref(bs), 7, out.data_ptr(), None, None, st), name, b"index = 7")
    name, fn = b"cf_shapley_interactions_from_rows", L.cf_shapley_interactions_from_rows
    refused(fn(None, rows.data_ptr(), 3, 8, 0, out.data_ptr(), st), name, b"null handle")
    refused(fn(model._handle, None, 3, 8, 0, out.data_ptr(), st), name, b"null rows")
    refused(fn(model._handle, rows.data_ptr(), 3, 8, 0, None, st), name, b"null inter")
    refused(fn(model._handle, rows.data_ptr(), 0, 8, 0, out.data_ptr(), st), name, b"B = 0")
    for P in (1, 17, -3):
        refused(fn(model._handle, rows.data_ptr(), 3, P, 0, out.data_ptr(), st), name, b"P = %d outside 2..16" % P)
    refused(fn(model._handle, rows.data_ptr(), 3, 8, 3, out.data_ptr(), st), name, b"index = 3")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and model.launch_counts() == f0      # nothing was launched
    # a one-slot model has no pair
    cfg1 = orc._cfg(dict(i_max=1))
    m1 = _pcre_model(cfg1, B=4, seed=3)
    b1 = orc.synthetic_batch(2, cfg=cfg1, seed=13, regime="realistic")
    with pytest.raises(RuntimeError, match="cf_pcre_shapley_interactions: 1 player: a pair needs at least 2"):
        m1.pcre_shapley_interactions(*[b1[k] for k in so.KEYS])
    # the Python layer: raised before the library is called
    for kw in (dict(index="shap"), dict(index=0), dict(players="genes")):
        with pytest.raises(ValueError, match="sii|mark_players"):
            model.mark_shapley_interactions((bs, keep_alive), **kw)
    for bad in (torch.zeros(3, 100, 2), torch.zeros(3, 2, 2), torch.zeros(3, 256, 1), torch.zeros(256, 2), torch.zeros(3, 256, 2, dtype=torch.float64)):
        with pytest.raises(ValueError, match="shapley_interactions"):
            model.shapley_interactions(bad)
    # armed riders (a training step in flight): refused; the handle is not used again
    assert L.cf_rider_arm(model._handle, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, 0, 8) == 0, L.cf_last_error()
    for name, fn, make, bad in families:
        good, alive = make()
        refused(fn(model._handle, C.byref(bs), C.byref(good), 0, out.data_ptr(), None, None, st), name, b"riders")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    del keep_alive, donor_alive


def test_a_pending_backward_is_refused_and_training_is_left_alone():
    from chromoformer_amd.engine import Trainer
    batches = [orc.synthetic_batch(4, seed=41 + i, regime="realistic") for i in range(3)]
    P = orc.init_params(None, 42, False)
    model = _model(None, False, P, 8)
    b = batches[0]
    three = [((0, 1), (0,)), ((2, 3), (0, 1)), ((4, 5, 6), (0, 1, 2))]
    calls = (("pcre_shapley_interactions", {}), ("mark_shapley_interactions", dict(players=three)),
             ("mark_donor_shapley_interactions", dict(players=three, donor=_feats(_dev(batches[2])))),
             ("mark_window_shapley_interactions", dict(players=THREE)), ("mark_fine_window_shapley_interactions", dict(players=PLAYERS[:3])))
    with torch.enable_grad():
        for method, kw in calls:
            out = model(*_args(b))
            res = getattr(model, method)(*_args(_dev(batches[1])), **kw)
            assert not res[0].requires_grad
            with pytest.raises(RuntimeError, match=method):
                out[:, 1].sum().backward()
        out = model(*_args(b))
        table = res[1]["phi"].new_zeros(4, 8, 2).normal_()
        model.shapley_interactions(table)      # the operator runs no forward: the pending backward goes through
        out[:, 1].sum().backward()
    assert float(model._gflat.abs().sum()) > 0

    def run(interpose):
        m = _model(None, False, P, 8)
        tr = Trainer(m, lr=1e-3)
        slots = [tr.stage(x) for x in batches]
        tr.step(slots[0])
        torch.cuda.synchronize()
        snap = [t.clone() for t in (m._flat, m._gflat, m._mflat, m._vflat)]
        if interpose:
            for method, kw in calls:
                getattr(m, method)(*_args(_dev(batches[2])), index="sti", **kw)
            m.shapley_interactions(torch.randn(2, 16, 2))
            torch.cuda.synchronize()
            for x, y in zip(snap, (m._flat, m._gflat, m._mflat, m._vflat)):
                assert torch.equal(x, y)
        tr.step(slots[1])
        tr.step(slots[2])
        torch.cuda.synchronize()
        sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        sd["<exp_avg>"], sd["<exp_avg_sq>"] = m._mflat.cpu().clone(), m._vflat.cpu().clone()
        return sd

    ref, got = run(False), run(True)
    assert all(torch.equal(ref[k], got[k]) for k in ref)


def _subset(ds, genes):
    import copy
    sub = copy.copy(ds)
    sub.target_genes = list(genes)
    return sub


def test_dataset_generators_and_cli(tmp_path):
    from chromoformer_amd import ChromoformerClassifier, predict
    from chromoformer_amd.data import ChromoformerDataset, GeneStore
    from tests.synth_data import make_dataset
    npy, dnpy = str(tmp_path / "npy"), str(tmp_path / "donor")
    meta = make_dataset(npy, n_genes=20, seed=11)
    genes = pd.read_csv(meta).gene_id.tolist()
    ds = ChromoformerDataset(meta, npy, genes)
    dn = do.donor_dataset(npy, dnpy, do.DONOR_SEED, w_prom=40000)
    P = orc.init_params(seed=7)
    ck = str(tmp_path / "w.pt")
    torch.save({"net": P}, ck)
    outs = {k: str(tmp_path / (k + ".npy")) for k in ("pcre", "mark", "donor")}
    shap = str(tmp_path / "marks.npz")
    assert predict.main(["-m", meta, "-d", npy, "-w", ck, "-o", str(tmp_path / "p.csv"), "--pcre-interactions-out", outs["pcre"],
                         "--mark-interactions-out", outs["mark"], "--mark-donor-interactions-out", outs["donor"], "--donor-npy-dir", dnpy,
                         "--mark-players", "regions", "--mark-scale", "0.5", "--interaction-index", "sti", "--mark-shapley-out", shap]) == 0
    model = ChromoformerClassifier(seed=123, max_batch=32).cuda(0)
    model.load_state_dict(P)
    store, dstore = GeneStore(ds, device=model._device, resident=True), GeneStore(dn, device=model._device, resident=True)
    d, dd = store.batch(list(range(20))), dstore.batch(list(range(20)))
    a = _args(d)
    want = {"pcre": model.pcre_shapley_interactions(*a, index="sti"), "mark": model.mark_shapley_interactions(*a, players="regions", scale=0.5, index="sti"),
            "donor": model.mark_donor_shapley_interactions(*a, donor=_feats(dd), players="regions", index="sti")}
    for k, (inter, info) in want.items():
        z = np.load(outs[k])
        S = 8 if k == "pcre" else 9
        assert z.shape == (20, S, S) and z.dtype == np.float32 and np.array_equal(z, z.transpose(0, 2, 1)), k
        assert np.array_equal(z, inter.cpu()[..., 1].numpy()), k
    z = np.load(shap)      # one interactions call served both outputs: the Shapley file as --mark-shapley-out alone writes it
    phi, info = model.mark_shapley(*a, players="regions", scale=0.5)
    assert np.array_equal(z["phi"], phi.cpu()[..., 1].numpy()) and np.array_equal(z["erased"], info["erased"].cpu()[:, 1].numpy())
    for argv in (["--interaction-index", "sii"], ["--mark-donor-interactions-out", outs["donor"]], ["--pcre-interactions-out", outs["pcre"], "--interaction-index", "shap"]):
        with pytest.raises(SystemExit) as e:
            predict.main(["-m", meta, "-d", npy, "-w", ck, "-o", str(tmp_path / "q.csv")] + argv)
        assert e.value.code == 2, argv
    # the generators: interactions=None yields the sibling's dict key for key; an index adds `interactions` from one call per batch
    sub = genes[3:13]
    gs, gd = GeneStore(_subset(ds, sub), device=model._device, resident=True), GeneStore(_subset(dn, sub), device=model._device, resident=True)
    b, bd = gs.batch(list(range(7))), gd.batch(list(range(7)))
    flip = [ds.genes[g]["tss"][2] != "+" for g in sub[:7]]
    cases = [(lambda **kw: model.mark_shapley_dataset(ds, genes=sub, bsz=7, **kw),
              lambda: model.mark_shapley_interactions(*_args(b), index="sti")),
             (lambda **kw: model.mark_donor_shapley_dataset(ds, dn, genes=sub, bsz=7, **kw),
              lambda: model.mark_donor_shapley_interactions(*_args(b), donor=_feats(bd), index="sti")),
             (lambda **kw: model.mark_window_shapley_dataset(ds, genes=sub, width=4, bsz=7, **kw),
              lambda: model.mark_window_shapley_interactions(*_args(b), width=4, flip=flip, index="sti"))]
    for gen, call in cases:
        plain, default, res = list(gen()), list(gen(interactions=None)), list(gen(interactions="sti"))
        assert [r["gene_id"] for r in res] == sub
        inter, info = call()
        for i, (p, q, r) in enumerate(zip(plain, default, res)):
            assert sorted(p) == sorted(q) and sorted(r) == sorted(list(p) + ["interactions"])
            for k in p:
                same = np.array_equal(p[k], r[k]) if isinstance(p[k], np.ndarray) else p[k] == r[k]
                assert same and (np.array_equal(p[k], q[k]) if isinstance(p[k], np.ndarray) else p[k] == q[k]), k
            if i < 7:
                assert r["interactions"].dtype == np.float32 and np.array_equal(r["interactions"], inter[i].cpu().numpy())
    # the fine generator: per rank the index among the players with a real window
    kw = dict(genes=sub, region=1, zoom=1, coarse_width=5, width=25, scale=0.25, bsz=4)
    plain, res = list(model.mark_fine_window_shapley_dataset(ds, **kw)), list(model.mark_fine_window_shapley_dataset(ds, interactions="sii", **kw))
    assert any(len(r["interactions"]) for r in res)
    for p, r in zip(plain, res):
        assert sorted(r) == sorted(list(p) + ["interactions"]) and np.array_equal(p["phi"], r["phi"]) and len(r["interactions"]) == len(r["zoom"])
        for rank, x in enumerate(r["interactions"]):
            n = int((r["rank"] == rank).sum())
            assert x.shape == (n, n, 2) and np.array_equal(x[np.arange(n), np.arange(n)], r["phi"][r["rank"] == rank])      # sii: phi on the diagonal
    # a game that would be sampled has no index
    with pytest.raises(ValueError, match="20 players"):
        next(model.mark_window_shapley_dataset(ds, genes=sub, width=1, interactions="sii"))
    with pytest.raises(ValueError, match="25 fine players"):
        next(model.mark_fine_window_shapley_dataset(ds, genes=sub, region=1, coarse_width=5, width=4, interactions="sii"))
    with pytest.raises(ValueError, match="sii"):
        next(model.mark_shapley_dataset(ds, genes=sub, interactions="shap"))
