"""The window game on the GPU (cf_mark_window_coalitions / cf_mark_window_shapley / cf_mark_window_shapley_sampled, the
ChromoformerBase methods mark_window_*, attribution.mark_window_shapley, predict --window-shapley-out / --window-donor-shapley-out).

  * the two identities of the definition: one absent single-region player is the perturbation scan's window, bit for bit; windows that
    cover the regions give the rows of mark_coalitions_wide, under both rules;
  * the bits of a row with mark x promoter-window players (70 players, three words) against the plain forward on the batch edited by
    tests/window_oracle.py (s = 0 and the donor rule: bit for bit; s = 2.5: the project's logit bound against the CPU oracle);
    overlapping absent players change an element once;
  * the sampled rows, phi, stderr and delta within the bounds tests/test_mark_sampled_gpu.py derives (the estimator kernel and its
    operation counts are the same), null players exactly 0, all 3! orders against the exact call, the exact call against float64;
  * the same bits whatever max_batch is and call after call; other model shapes; the launch contract and every refusal by name; no side
    effects on training; the dataset walker and the CLI."""
import ctypes as C
import itertools
import os
import types

import numpy as np
import pandas as pd
import pytest
import torch

from chromoformer_amd import _lib
from chromoformer_amd.attribution import mark_wide_words, shapley_permutations, window_players
from oracle import chromoformer_oracle as orc
from tests import donor_oracle as do
from tests import perm_oracle as po
from tests import scan_oracle as so
from tests import window_oracle as wo
from tests.coalition_oracle import shapley_fp64
from tests.test_input_grads_gpu import _model
from tests.test_mark_coalitions_gpu import GENES, SHAPES
from tests.test_mark_donor_gpu import _dev, _feats
from tests.test_mark_sampled_gpu import _args, _cell_words, _check_estimate, _g, _host, _plain
from tests.test_pcre_coalitions_gpu import U, _gamma

pytestmark = pytest.mark.gpu
ALL = tuple(range(7))
SEED = 5
TOL = 1e-4      # the project's logit bound
CELLS2 = wo.players_promoter_cells(7, 20, 2)      # 70 players
REGIONS4 = wo.players_regions(7, 8, 20, 4)        # 45 players: windows past a pCRE's end, dummy slots
THREE = [(ALL, (0,), (0, 10)), (ALL, (0,), (10, 20)), (ALL, (8,), (0, 20))]      # two halves of the promoter, pCRE slot 7 (a dummy of gene 2)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """The three genes (a mirrored narrowed promoter, a '+' strand gene, a gene with dummy slots alone) and the donor cell type: host and
    device batches and the promoter flips, built once, never written."""
    ds = so.scan_dataset(str(tmp_path_factory.mktemp("windows")), w_prom=39000)
    dn = do.donor_dataset(ds.npy_dir, str(tmp_path_factory.mktemp("donor")), do.DONOR_SEED, w_prom=39000)
    cpu, dcpu = so.dataset_batch(ds, GENES), so.dataset_batch(dn, GENES)
    flips = [ds.genes[g]["tss"][2] != "+" for g in GENES]
    assert any(flips) and not ds.genes[GENES[2]]["pcres"]
    return types.SimpleNamespace(cpu=cpu, dev=_dev(cpu), dcpu=dcpu, ddev=_dev(dcpu), flips=flips)


@pytest.fixture(scope="module")
def small():
    """The seed-42 classifier (the golden's weights) at max_batch = 4."""
    return _model(None, False, orc.init_params(None, 42, False), 4)


@pytest.fixture(scope="module")
def wide64():
    return _model(None, False, orc.init_params(None, 42, False), 64)


@pytest.fixture(scope="module")
def cells2(data, small):
    """(phi, info) of small.mark_window_shapley_sampled, mark x promoter window at width 2, two orders, s = 0: 3 x 140 rows in 105 chunks."""
    phi, info = small.mark_window_shapley_sampled(*_args(data.dev), players="promoter_cells", width=2, n_perm=2, seed=SEED, flip=data.flips,
                                                  return_rows=True)
    torch.cuda.synchronize()
    return phi.cpu(), _host(info)


@pytest.fixture(scope="module")
def cells2_donor(data, small):
    phi, info = small.mark_window_shapley_sampled(*_args(data.dev), players="promoter_cells", width=2, n_perm=2, seed=SEED, flip=data.flips,
                                                  donor=_feats(data.ddev), return_rows=True)
    torch.cuda.synchronize()
    return phi.cpu(), _host(info)


def _edited(model, data, players, word, scale=0.0, donor=False):
    """The plain forward on the batch the CPU oracle edits for coalition `word`."""
    return _plain(model, _dev(wo.edited_batch(data.cpu, players, word, scale, donor=data.dcpu if donor else None, flip=data.flips)))


def _absent(P, *gone):
    return wo.full_word(P) & ~sum(1 << p for p in gone)


def _words70():
    """The full word, the empty word, players 31 / 32 and 63 / 64 alone absent (the two sides of the word boundaries), six seeded words."""
    rng = np.random.default_rng(17)
    rand = [int("".join("1" if x else "0" for x in rng.random(70) < 0.5), 2) for _ in range(6)]
    return [wo.full_word(70), 0, _absent(70, 31, 32), _absent(70, 63, 64)] + rand


@pytest.mark.parametrize("region", [0, 1])
def test_one_absent_player_is_the_scan_window_bit_for_bit(data, wide64, region):
    """Identity (a).  The promoter of gene 0 is mirrored and narrowed (19.5 coarse bins); pCRE slot 0 holds 7 / 1 / 0 coarse bins: the
    windows at 5 (width 3) and 18 overhang n_c or lie past it."""
    starts = (0, 5, 6, 18, 19)
    for s in (0.0, 2.5):
        for width in (1, 3):
            scan = wide64.perturbation_scan(*_args(data.dev), region=region, scale=s, width=width, mark_sets=[(1, 4)],
                                            flip=data.flips if region == 0 else None).cpu()      # (a pCRE is never stored mirrored)
            players = [((1, 4), (region,), (lo, min(lo + width, 20))) for lo in starts] + [(ALL, (0, 1), (0, 20))]
            words = [_absent(6, p) for p in range(5)] + [wo.full_word(6)]
            got = wide64.mark_window_coalitions(*_args(data.dev), keep=words, players=players, scale=s, flip=data.flips).cpu()
            assert got.shape == (3, 6, 2) and not got.requires_grad
            assert torch.equal(got[:, 5], scan[:, 0])
            for p, lo in enumerate(starts):
                assert torch.equal(got[:, p], scan[:, 1 + lo]), (region, s, width, lo)
            assert not torch.equal(got[:2, 0], scan[:2, 0])
            if region == 1:      # gene 1's pCRE is one coarse bin long, gene 2 has none: null windows
                assert torch.equal(got[1:, 1:5], scan[1:, :1].expand(2, 4, 2)) and torch.equal(got[2, 0], scan[2, 0])
    if region == 0:      # without the flips the mirrored promoter's rows differ
        wrong = wide64.mark_window_coalitions(*_args(data.dev), keep=words, players=players, scale=2.5).cpu()
        for i in range(3):
            assert torch.equal(wrong[i], got[i]) == (not data.flips[i]), i


@pytest.mark.parametrize("rule", ["scale", "donor"])
def test_whole_region_windows_are_the_wide_game(data, small, rule):
    """Identity (b): the dataset's padded rows hold zeros, and the donor is built at the same coordinates."""
    players = [((f,), (rho,), (0, 20)) for rho in range(9) for f in range(7)]
    words = _cell_words()
    for kw in ((dict(scale=0.0), dict(scale=2.5)) if rule == "scale" else (dict(donor=_feats(data.ddev)),)):
        got = small.mark_window_coalitions(*_args(data.dev), keep=words, players=players, flip=data.flips, **kw).cpu()
        ref = small.mark_coalitions_wide(*_args(data.dev), keep=words, players="cells", **kw).cpu()
        assert got.shape == (3, 10, 2) and torch.equal(got, ref), kw.keys()
    assert torch.equal(got[:, 0], _plain(small, data.dev)) and not torch.equal(got[:, 1], got[:, 0])


@pytest.mark.parametrize("rule", ["scale", "donor"])
def test_70_players_rows_are_the_plain_forward_on_the_edited_batch(data, small, rule):
    words = _words70()
    kw = dict(donor=_feats(data.ddev)) if rule == "donor" else {}
    got = small.mark_window_coalitions(*_args(data.dev), keep=words, players="promoter_cells", width=2, flip=data.flips, **kw).cpu()
    base = _plain(small, data.dev)
    assert got.shape == (3, 10, 2) and torch.equal(got[:, 0], base)
    for c, m in enumerate(words):
        assert torch.equal(got[:, c], _edited(small, data, CELLS2, m, 0.0, rule == "donor")), (rule, c, hex(m))
    assert len({tuple(got[0, c].tolist()) for c in range(10)}) == 10
    bits = np.array([[bool(m >> p & 1) for p in range(70)] for m in words])
    assert torch.equal(small.mark_window_coalitions(*_args(data.dev), keep=bits, players="promoter_cells", width=2, flip=data.flips, **kw).cpu(), got)
    assert torch.equal(small.mark_window_coalitions(small.pack_batch(data.dev), keep=words, players=CELLS2, flip=data.flips, **kw).cpu(), got)


def test_70_players_scaled_rows_against_the_cpu_oracle(data, small):
    words = _words70()
    got = small.mark_window_coalitions(*_args(data.dev), keep=words, players="promoter_cells", width=2, scale=2.5, flip=data.flips).cpu()
    P = orc.init_params(None, 42, False)
    for c, m in enumerate(words):
        with torch.no_grad():
            ref = orc.forward(P, wo.edited_batch(data.cpu, CELLS2, m, 2.5, flip=data.flips))
        d = (got[:, c] - ref).abs().max().item()
        print("word %d: |gpu - oracle| %.2e" % (c, d))
        assert d <= TOL, (c, d)
    assert (got[:, 1] - got[:, 0]).abs().max().item() > 100 * TOL


def test_overlapping_absent_players_change_an_element_once(data, small):
    pair = [((1, 4), (0, 1), (2, 7)), ((1, 4), (0, 1), (5, 12))]
    union = [((1, 4), (0, 1), (2, 12))]
    got = small.mark_window_coalitions(*_args(data.dev), keep=[0, 1, 2, 3], players=pair, scale=2.5, flip=data.flips).cpu()
    ref = small.mark_window_coalitions(*_args(data.dev), keep=[0, 1], players=union, scale=2.5, flip=data.flips).cpu()
    assert torch.equal(got[:, 0], ref[:, 0]) and torch.equal(got[:, 3], ref[:, 1])
    assert not torch.equal(got[:, 1], got[:, 0]) and not torch.equal(got[:, 2], got[:, 0])
    twice = small.mark_window_coalitions(*_args(data.dev), keep=[0], players=[((1, 4), (0, 1), (5, 7))], scale=2.5 * 2.5, flip=data.flips).cpu()
    assert not torch.equal(twice[:, 0], got[:, 0])


@pytest.mark.parametrize("rule", ["scale", "donor"])
def test_sampled_rows_are_the_prefix_coalitions_bit_for_bit(data, small, cells2, cells2_donor, rule):
    phi, info = cells2 if rule == "scale" else cells2_donor
    perms, rows = info["permutations"], info["rows"]
    assert perms.dtype == np.uint8 and perms.shape == (2, 70) and np.array_equal(perms, shapley_permutations(70, 2, SEED))
    assert rows.shape == (3, 2 + 2 * 69, 2) and phi.shape == info["stderr"].shape == (3, 70, 2) and not phi.requires_grad
    assert info["names"] == window_players("promoter_cells", 7, 8, 20, 2)[4] and info["names"][17] == "mark3@promoter[4:6]"
    base = _plain(small, data.dev)
    assert torch.equal(rows[:, 1], base) and torch.equal(info["logits"], base)
    assert torch.equal(rows[:, 0], _edited(small, data, CELLS2, 0, 0.0, rule == "donor")) and torch.equal(info["absent"], rows[:, 0])
    words = po.prefix_words(perms)
    kw = dict(donor=_feats(data.ddev)) if rule == "donor" else {}
    got = small.mark_window_coalitions(*_args(data.dev), keep=words, players="promoter_cells", width=2, flip=data.flips, **kw).cpu()
    assert got.shape == rows.shape and torch.equal(got, rows)
    assert len({tuple(rows[0, c].tolist()) for c in range(2, 71)}) > 60


@pytest.mark.parametrize("rule", ["scale", "donor"])
def test_phi_stderr_and_delta(cells2, cells2_donor, rule):
    phi, info = cells2 if rule == "scale" else cells2_donor
    _check_estimate(phi, info)
    assert float((phi != 0).any(-1).float().mean()) > 0.9 and bool((info["stderr"] > 0).any())
    cells = phi.view(3, 10, 7, 2)      # [B, window, mark, n_out]
    assert torch.equal(cells[:, 2, 3], phi[:, 17])


@pytest.mark.parametrize("rule", ["scale", "donor"])
def test_null_players_are_exactly_zero(data, wide64, rule):
    """All marks per (region, window of 4 coarse bins): a window past the pCRE's real bins and every window of a dummy slot is null."""
    kw = dict(donor=_feats(data.ddev)) if rule == "donor" else {}
    phi, info = wide64.mark_window_shapley_sampled(*_args(data.dev), players="regions", width=4, n_perm=2, seed=SEED, flip=data.flips,
                                                   return_rows=True, **kw)
    null = np.zeros((3, 45), dtype=bool)
    masks = so.centre_row(data.cpu["pcre_pad_masks"][2000], 3 * 8, 20).reshape(3, 8, 20)
    for i in range(3):
        for p, (_, (rho,), (lo, _)) in enumerate(REGIONS4):
            null[i, p] = rho > 0 and lo >= so.extent(masks[i, rho - 1])[1]
    assert null[2, 5:].all() and not null[:, :5].any() and null[0].any() and not null[0].all() and not null[:2, 5].any()
    _check_estimate(phi, info, null)
    assert float((phi.cpu()[torch.from_numpy(~null)] != 0).any(-1).float().mean()) > 0.9
    assert info["names"][5] == "pcre0[0:4]" and info["names"][44] == "pcre7[16:20]"


def test_all_orders_give_the_exact_call_and_the_exact_call_float64(data, small):
    """Three explicit players, all 3! = 6 orders: the estimator is the Shapley value; the bound is tests/test_mark_sampled_gpu.py's.  The
    exact call against shapley_fp64 on its own rows within k_shapley's bound (tests/test_pcre_coalitions_gpu.py)."""
    every = np.array(list(itertools.permutations(range(3))), dtype=np.uint8)
    for kw in (dict(scale=0.0), dict(scale=2.5), dict(donor=_feats(data.ddev))):
        ref, rinfo = small.mark_window_shapley(*_args(data.dev), players=THREE, flip=data.flips, return_coalitions=True, **kw)
        table = rinfo["coalitions"].cpu()
        absent = "donor" if "donor" in kw else "erased"
        assert sorted(rinfo) == sorted(["coalitions", "delta", absent, "logits", "players"]) and table.shape == (3, 8, 2)
        assert torch.equal(table[:, 7], _plain(small, data.dev)) and torch.equal(rinfo[absent].cpu(), table[:, 0])
        assert torch.equal(table, small.mark_window_coalitions(*_args(data.dev), keep=list(range(8)), players=THREE, flip=data.flips, **kw).cpu())
        phi64, scale = shapley_fp64(table.numpy())
        err = np.abs(ref.cpu().numpy().astype(np.float64) - phi64)
        print("exact %s: max err %.3e, max bound %.3e" % (sorted(kw), err.max(), (_gamma(3) * scale).max()))
        assert (err <= _gamma(3) * scale).all()
        dbound = 3 * (_gamma(3) * scale).max(1) + 4 * U * np.abs(table.numpy()).max(1)
        assert (np.abs(rinfo["delta"].cpu().numpy()) <= dbound).all()
        phi, info = small.mark_window_shapley_sampled(*_args(data.dev), players=THREE, permutations=every, flip=data.flips, return_rows=True, **kw)
        assert torch.equal(info["rows"].cpu(), table[:, [int(m) for m in po.prefix_words(every)]])      # the same row bits
        _check_estimate(phi, info)
        d = po.marginals(info["rows"].cpu().numpy(), every, np.float32)
        bound = _g(6 + 1) * np.abs(d.astype(np.float64)).mean(1) + _gamma(3) * scale
        err = np.abs(phi.cpu().numpy().astype(np.float64) - ref.cpu().numpy().astype(np.float64))
        print("exactness %s: max err %.3e, max bound %.3e" % (sorted(kw), err.max(), bound.max()))
        assert (err <= bound).all(), (err.max(), bound.max())
        assert bool((ref[2, 2] == 0).all()) and bool((phi[2, 2] == 0).all()) and bool((ref[:, :2] != 0).all())      # gene 2's slot 7 is a dummy


def test_same_bits_for_every_max_batch_and_call_after_call(data, cells2, cells2_donor, wide64):
    for cap in (7, 64):
        model = wide64 if cap == 64 else _model(None, False, orc.init_params(None, 42, False), cap)
        for (phi, info), kw in ((cells2, {}), (cells2_donor, dict(donor=_feats(data.ddev)))):
            p, i = model.mark_window_shapley_sampled(*_args(data.dev), players="promoter_cells", width=2, n_perm=2, seed=SEED, flip=data.flips,
                                                     return_rows=True, **kw)
            assert torch.equal(p.cpu(), phi) and torch.equal(i["stderr"].cpu(), info["stderr"]) and torch.equal(i["rows"].cpu(), info["rows"]), cap
            assert torch.equal(i["delta"].cpu(), info["delta"])
    again, info2 = wide64.mark_window_shapley_sampled(*_args(data.dev), players="promoter_cells", width=2, n_perm=2, seed=SEED, flip=data.flips,
                                                      return_rows=True)
    assert torch.equal(again.cpu(), cells2[0]) and torch.equal(info2["rows"].cpu(), cells2[1]["rows"])
    other = wide64.mark_window_shapley_sampled(*_args(data.dev), players="promoter_cells", width=2, n_perm=2, seed=SEED + 1, flip=data.flips)[0]
    assert not torch.equal(other.cpu(), cells2[0])
    exact = [m.mark_window_shapley(*_args(data.dev), players=THREE, scale=2.5, flip=data.flips)[0].cpu()
             for m in (wide64, _model(None, False, orc.init_params(None, 42, False), 7), wide64)]
    assert torch.equal(exact[0], exact[1]) and torch.equal(exact[0], exact[2])


@pytest.mark.parametrize("name", ["d_emb_64", "embed_2_layers", "reg_layer_by_layer", "regressor", "i_max16", "odd_lengths"])
def test_other_shapes(name):
    """One order of the (region, window) players on two genes, in chunks of 5: the end rows and a few prefixes against the plain forward
    on the oracle-edited batch, the estimate against float64.  i_max16: 17 regions x 7 windows of 3 = 119 players, four words;
    odd_lengths: L F is no multiple of 4 floats, the element-by-element path."""
    from tests.test_mark_donor_gpu import SHAPES as DONOR_SHAPES
    over, regression = dict(SHAPES, odd_lengths=DONOR_SHAPES["odd_lengths"])[name]
    cfg = orc._cfg(over)
    S, W = cfg["i_max"], cfg["w_max"] // max(cfg["binsizes"])
    width = 3 if name == "i_max16" else 4
    cpu = orc.synthetic_batch(2, cfg=cfg, seed=13, regime="realistic")
    batch = _dev(cpu)
    if name == "embed_2_layers":      # the reference's full [B, 1, L, L] promoter mask: the chunk rows carry all L rows
        assert all(m.numel() == 2 * L * L for m, L in zip(batch["promoter_pad_masks"].values(), (20, 80, 400)))
    model = _model(cfg, regression, orc.init_params(cfg, 3, regression), 5)
    players = wo.players_regions(7, S, W, width)
    flips = [True, False]
    phi, info = model.mark_window_shapley_sampled(*_args(batch), players="regions", width=width, n_perm=1, seed=2, flip=flips, return_rows=True)
    P = len(players)
    assert P == (119 if name == "i_max16" else (S + 1) * -(-W // width)) and info["names"] == window_players("regions", 7, S, W, width)[4]
    rows = info["rows"].cpu()
    assert rows.shape == (2, P + 1, 1 if regression else 2) and phi.shape == (2, P, rows.shape[-1])
    words = po.prefix_words(info["permutations"])
    for c in sorted({c for c in (0, 1, 2, 31, 32, 33, P // 2, P - 1, P) if c <= P}):
        ref = _plain(model, _dev(wo.edited_batch(cpu, players, words[c], 0.0, flip=flips)))
        assert torch.equal(rows[:, c], ref), (name, c)
    _check_estimate(phi, info)
    assert bool((phi != 0).any())
    don = orc.synthetic_batch(2, cfg=cfg, seed=14, regime="realistic")
    got = model.mark_window_coalitions(*_args(batch), keep=[words[P // 2], 0], players=players, donor=_feats(_dev(don)), flip=flips).cpu()
    for c, m in enumerate((words[P // 2], 0)):
        assert torch.equal(got[:, c], _plain(model, _dev(wo.edited_batch(cpu, players, m, donor=don, flip=flips)))), (name, c)


@pytest.mark.parametrize("cap", [64, 7])
def test_launch_contract(data, cap, wide64):
    """fwd = ceil(B n_coal / max_batch) (1 + n_fwd), n_fwd those of cf_forward(save = 0); the Shapley calls add their reducer."""
    model = wide64 if cap == 64 else _model(None, False, orc.init_params(None, 42, False), cap)
    _plain(model, data.dev)
    n_fwd = model.launch_counts()[0]
    chunks = lambda rows: -(-rows // cap)      # noqa: E731
    model.mark_window_coalitions(*_args(data.dev), keep=_words70(), players="promoter_cells", width=2, flip=data.flips)
    assert model.launch_counts()[0] == chunks(3 * 10) * (1 + n_fwd)
    model.mark_window_coalitions(*_args(data.dev), keep=[0, 5], players="promoter", width=4, donor=_feats(data.ddev))
    assert model.launch_counts()[0] == chunks(3 * 2) * (1 + n_fwd)
    model.mark_window_shapley(*_args(data.dev), players="promoter", width=5)
    assert model.launch_counts()[0] == chunks(3 * 16) * (1 + n_fwd) + 1
    model.mark_window_shapley_sampled(*_args(data.dev), players="promoter", n_perm=3)
    assert model.launch_counts()[0] == chunks(3 * (2 + 3 * 19)) * (1 + n_fwd) + 1
    model.mark_window_shapley_sampled(*_args(data.dev), players=[(ALL, (0,), (3, 4))], n_perm=4, donor=_feats(data.ddev))
    assert model.launch_counts()[0] == chunks(3 * 2) * (1 + n_fwd) + 1


def _raw_opts(game, scale=0.0, flip=None, don_p=(None,) * 3, don_c=(None,) * 3, n_players=None, **over):
    pm, pr, lo, hi = (over.get(k, v) for k, v in zip(("marks", "regions", "lo", "hi"), game[:4]))
    o = _lib.cf_mark_window_opts()
    o.n_players, o.scale = len(game[0]) if n_players is None else n_players, scale
    o.player_marks, o.player_regions = (a.ctypes.data if a is not None else None for a in (pm, pr))
    o.player_lo, o.player_hi = (a.ctypes.data if a is not None else None for a in (lo, hi))
    o.flip = flip
    for r in range(3):
        o.donor_promoter_feats[r], o.donor_pcre_feats[r] = don_p[r], don_c[r]
    return o, (pm, pr, lo, hi)


def test_null_stderr_and_the_handle_owned_rows_through_the_c_abi(data, small, cells2):
    L = _lib.lib()
    bs, keep_alive = small.pack_batch(data.dev)
    st = torch.cuda.current_stream().cuda_stream
    flip = torch.tensor(data.flips, dtype=torch.uint8, device="cuda")
    o, alive = _raw_opts(window_players("promoter_cells", 7, 8, 20, 2), flip=flip.data_ptr())
    perms = shapley_permutations(70, 2, SEED)
    phi = torch.full((3, 70, 2), float("nan"), device="cuda")
    se = torch.full((3, 70, 2), float("nan"), device="cuda")
    assert L.cf_mark_window_shapley_sampled(small._handle, C.byref(bs), C.byref(o), perms.ctypes.data, 2, phi.data_ptr(), None, None, st) == 0, L.cf_last_error()
    assert torch.equal(phi.cpu(), cells2[0])
    phi.fill_(float("nan"))
    assert L.cf_mark_window_shapley_sampled(small._handle, C.byref(bs), C.byref(o), perms.ctypes.data, 2, phi.data_ptr(), se.data_ptr(), None, st) == 0, L.cf_last_error()
    assert torch.equal(phi.cpu(), cells2[0]) and torch.equal(se.cpu(), cells2[1]["stderr"])
    o3, alive3 = _raw_opts(window_players(THREE, 7, 8, 20), scale=2.5, flip=flip.data_ptr())
    ref = small.mark_window_shapley((bs, keep_alive), players=THREE, scale=2.5, flip=data.flips)[0]
    phi3 = torch.full((3, 3, 2), float("nan"), device="cuda")
    assert L.cf_mark_window_shapley(small._handle, C.byref(bs), C.byref(o3), phi3.data_ptr(), None, st) == 0, L.cf_last_error()
    assert torch.equal(phi3, ref)
    del keep_alive, alive, alive3


def test_refusals_by_name_with_nothing_launched(data):
    L = _lib.lib()
    model = _model(None, False, orc.init_params(None, 42, False), 4)
    bs, keep_alive = model.pack_batch(data.dev)
    dbs, donor_alive = model.pack_batch(data.ddev)
    _plain(model, data.dev)
    f0 = model.launch_counts()
    st = torch.cuda.current_stream().cuda_stream
    out = torch.full((3, 256, 2), float("nan"), device="cuda")
    game = window_players("promoter_cells", 7, 8, 20, 2)
    small_game = window_players("promoter", 7, 8, 20, 4)
    words = mark_wide_words([0, 1, (1 << 70) - 1, 1 << 69], 70)
    perms = shapley_permutations(70, 2, 0)
    big = _lib.cf_batch.from_buffer_copy(bs)
    big.B = 5
    dp, dc = tuple(dbs.promoter_feats[r] for r in range(3)), tuple(dbs.pcre_feats[r] for r in range(3))

    def edited(a, p, v):
        a = a.copy()
        a[p] = v
        return a

    many = np.ones(129, dtype=np.uint32)
    bad_opts = [(dict(n_players=0), b"n_players = 0 outside 1..128"),
                (dict(n_players=129, marks=many, regions=many, lo=np.zeros(129, np.int32), hi=np.ones(129, np.int32)), b"n_players = 129 outside 1..128"),
                (dict(marks=None), b"null player_marks"), (dict(regions=None), b"null player_marks / player_regions"),
                (dict(lo=None), b"null player_lo / player_hi"), (dict(hi=None), b"null player_lo / player_hi"),
                (dict(marks=edited(game[0], 40, 0)), b"player_marks[40] = 0"), (dict(regions=edited(game[1], 62, 0)), b"player_regions[62] = 0"),
                (dict(marks=edited(game[0], 1, 0x80)), b"n_feats"), (dict(regions=edited(game[1], 6, 0x200)), b"i_max"),
                (dict(lo=edited(game[2], 33, -1)), b"player 33 has the window [-1,"), (dict(hi=edited(game[3], 69, 21)), b"player 69 has the window [18, 21)"),
                (dict(lo=edited(game[2], 7, 4)), b"player 7 has the window [4, 4)"),
                (dict(scale=-0.5), b"scale"), (dict(scale=float("inf")), b"scale"), (dict(scale=float("nan")), b"scale"),
                (dict(don_p=dp), b"donor_promoter_feats / donor_pcre_feats"), (dict(don_p=dp, don_c=(dc[0], None, dc[2])), b"donor_promoter_feats / donor_pcre_feats"),
                (dict(don_c=(None, dc[1], None)), b"are null")]
    entries = [(b"cf_mark_window_coalitions", game, lambda h, b, o, dst: L.cf_mark_window_coalitions(h, b, o, words.ctypes.data, 4, dst, st)),
               (b"cf_mark_window_shapley_sampled", game, lambda h, b, o, dst: L.cf_mark_window_shapley_sampled(h, b, o, perms.ctypes.data, 2, dst, None, None, st))]

    def refused(rc, *needles):
        err = L.cf_last_error()
        assert rc != 0 and all(n in err for n in needles), err

    for name, g, fn in entries:
        good, alive = _raw_opts(g)
        refused(fn(None, C.byref(bs), C.byref(good), out.data_ptr()), name, b"null handle")
        refused(fn(model._handle, None, C.byref(good), out.data_ptr()), name, b"null batch")
        refused(fn(model._handle, C.byref(bs), None, out.data_ptr()), name, b"null opts")
        refused(fn(model._handle, C.byref(bs), C.byref(good), None), name, b"null logits" if b"coalitions" in name else b"null phi")
        refused(fn(model._handle, C.byref(big), C.byref(good), out.data_ptr()), name, b"max_batch")
        for kw, msg in bad_opts:
            o, alive = _raw_opts(g, **kw)
            refused(fn(model._handle, C.byref(bs), C.byref(o), out.data_ptr()), name, msg)
    good, alive = _raw_opts(game)
    name = b"cf_mark_window_coalitions"
    refused(L.cf_mark_window_coalitions(model._handle, C.byref(bs), C.byref(good), None, 4, out.data_ptr(), st), name, b"null keep")
    refused(L.cf_mark_window_coalitions(model._handle, C.byref(bs), C.byref(good), words.ctypes.data, 0, out.data_ptr(), st), name, b"n_coal")
    bad = words.copy()
    bad[3, 2] |= 1 << 6      # player 70 of 70
    refused(L.cf_mark_window_coalitions(model._handle, C.byref(bs), C.byref(good), bad.ctypes.data, 4, out.data_ptr(), st), name, b"keep[3]", b"n_players = 70")
    name = b"cf_mark_window_shapley_sampled"
    refused(L.cf_mark_window_shapley_sampled(model._handle, C.byref(bs), C.byref(good), None, 2, out.data_ptr(), None, None, st), name, b"null perms")
    refused(L.cf_mark_window_shapley_sampled(model._handle, C.byref(bs), C.byref(good), perms.ctypes.data, 0, out.data_ptr(), None, None, st), name, b"n_perm = 0")
    twice = perms.copy()
    twice[1, 5] = twice[1, 6]
    refused(L.cf_mark_window_shapley_sampled(model._handle, C.byref(bs), C.byref(good), twice.ctypes.data, 2, out.data_ptr(), None, None, st), name, b"perms[1]", b"not a permutation")
    name = b"cf_mark_window_shapley"      # the exact call: at most 16 players
    refused(L.cf_mark_window_shapley(model._handle, C.byref(bs), C.byref(good), out.data_ptr(), None, st), name, b"n_players = 70 outside 1..16")
    five, alive5 = _raw_opts(small_game)
    refused(L.cf_mark_window_shapley(model._handle, C.byref(bs), C.byref(five), None, None, st), name, b"null phi")
    refused(L.cf_mark_window_shapley(model._handle, C.byref(bs), C.byref(_raw_opts(small_game, hi=edited(small_game[3], 4, 40))[0]), out.data_ptr(), None, st),
            name, b"player 4 has the window [16, 40)")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and model.launch_counts() == f0      # nothing was launched
    # geometry: bin counts that do not nest, in the scan's wording, and a coarsest resolution of more than 64 bins
    for over, msg in ((dict(binsizes=[2000, 800, 100], w_max=40000), b"n_bins[1] = 50 is not a multiple of the coarsest resolution's 20 bins"),
                      (dict(binsizes=[500, 250, 125], w_max=40000), b"W = 80 bins")):
        cfg = orc._cfg(over)
        odd = _model(cfg, False, orc.init_params(cfg, 3, False), 2)
        ob, odd_alive = odd.pack_batch(_dev(orc.synthetic_batch(2, cfg=cfg, seed=1, regime="realistic")))
        g1 = window_players("promoter", 7, 8, 20, 4)
        o, alive = _raw_opts(g1)
        odd_out = torch.full((2, 4, 2), float("nan"), device="cuda")
        w4 = mark_wide_words([0, 1], 5)
        n0 = odd.launch_counts()
        refused(L.cf_mark_window_coalitions(odd._handle, C.byref(ob), C.byref(o), w4.ctypes.data, 2, odd_out.data_ptr(), st), b"cf_mark_window_coalitions", msg)
        torch.cuda.synchronize()
        assert bool(torch.isnan(odd_out).all()) and odd.launch_counts() == n0
        del odd_alive
    # the donor rule does not read the scale
    o, alive = _raw_opts(game, scale=-1.0, don_p=dp, don_c=dc)
    assert L.cf_mark_window_coalitions(model._handle, C.byref(bs), C.byref(o), words.ctypes.data, 1, out.data_ptr(), st) == 0, L.cf_last_error()
    torch.cuda.synchronize()
    out.fill_(float("nan"))
    # armed riders (a training step in flight): refused; the handle is not used again
    assert L.cf_rider_arm(model._handle, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, 0, 8) == 0, L.cf_last_error()
    for name, g, fn in entries:
        refused(fn(model._handle, C.byref(bs), C.byref(good), out.data_ptr()), name, b"riders")
    refused(L.cf_mark_window_shapley(model._handle, C.byref(bs), C.byref(five), out.data_ptr(), None, st), b"cf_mark_window_shapley", b"riders")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    for kw in (dict(players="cells"), dict(players="promoter_cells"), dict(players=[((7,), (0,), (0, 1))]), dict(players=[(ALL, (0,), (3, 3))]),
               dict(keep=[1 << 20]), dict(keep=[-1])):      # (raised before the library is called)
        with pytest.raises(ValueError, match="window_players|mark_window_coalitions"):
            model.mark_window_coalitions((bs, keep_alive), **dict(dict(keep=[0]), **kw))
    with pytest.raises(ValueError, match="keep is required"):
        model.mark_window_coalitions((bs, keep_alive))
    with pytest.raises(ValueError, match="mark_window_shapley: 20 players"):
        model.mark_window_shapley((bs, keep_alive))
    with pytest.raises(ValueError, match="mark_window_shapley_sampled: permutations"):
        model.mark_window_shapley_sampled((bs, keep_alive), permutations=np.zeros((2, 19), dtype=np.int64))
    with pytest.raises(ValueError, match="flip has 2 entries"):
        model.mark_window_coalitions((bs, keep_alive), keep=[0], flip=[True, False])
    with pytest.raises(ValueError, match="mark_window_shapley_sampled: the donor holds"):
        model.mark_window_shapley_sampled((bs, keep_alive), donor=big)
    del keep_alive, donor_alive, alive, alive5


def test_no_side_effects_on_training():
    from chromoformer_amd.engine import Trainer
    batches = [orc.synthetic_batch(8, seed=41 + i, regime="realistic") for i in range(3)]
    P = orc.init_params(None, 42, False)

    def run(interpose):
        model = _model(None, False, P, 8)
        tr = Trainer(model, lr=1e-3)
        slots = [tr.stage(b) for b in batches]
        tr.step(slots[0])
        torch.cuda.synchronize()
        snap = [t.clone() for t in (model._flat, model._gflat, model._mflat, model._vflat)]
        if interpose:
            dev = _dev(batches[2])
            model.mark_window_shapley_sampled(*_args(dev), players="promoter", width=2, n_perm=2, scale=2.0)
            model.mark_window_shapley(*_args(dev), players="promoter", width=7, donor=_feats(_dev(batches[1])))
            model.mark_window_coalitions(*_args(dev), keep=[0, 1 << 40], players="promoter_cells", width=2, flip=[True] * 8)
            torch.cuda.synchronize()
            for x, y in zip(snap, (model._flat, model._gflat, model._mflat, model._vflat)):
                assert torch.equal(x, y)
        tr.step(slots[1])
        tr.step(slots[2])
        torch.cuda.synchronize()
        sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        sd["<exp_avg>"], sd["<exp_avg_sq>"] = model._mflat.cpu().clone(), model._vflat.cpu().clone()
        return sd

    ref, got = run(False), run(True)
    assert all(torch.equal(ref[k], got[k]) for k in ref)


def test_a_pending_backward_is_refused():
    b = _dev(orc.synthetic_batch(4, seed=41, regime="realistic"))
    model = _model(None, False, orc.init_params(None, 42, False), 8)
    with torch.enable_grad():
        for method, kw in (("mark_window_shapley_sampled", dict(players="promoter", width=5, n_perm=1)), ("mark_window_shapley", dict(players="promoter", width=10)),
                           ("mark_window_coalitions", dict(keep=[0]))):
            out = model(*_args(b))
            res = getattr(model, method)(*_args(b), **kw)
            assert not (res if torch.is_tensor(res) else res[0]).requires_grad
            with pytest.raises(RuntimeError, match=method):
                out[:, 1].sum().backward()
        model(*_args(b))[:, 1].sum().backward()      # a fresh forward trains as before
    assert float(model._gflat.abs().sum()) > 0


def test_dataset_walker_and_cli(tmp_path):
    from chromoformer_amd import ChromoformerClassifier, predict
    from chromoformer_amd.data import ChromoformerDataset, GeneStore
    from tests.synth_data import make_dataset
    from tests.test_mark_sampled_gpu import _subset
    npy, dnpy = str(tmp_path / "npy"), str(tmp_path / "donor")
    meta = make_dataset(npy, n_genes=20, seed=11)
    dn = do.donor_dataset(npy, dnpy, do.DONOR_SEED, w_prom=40000)
    genes = pd.read_csv(meta).gene_id.tolist()
    P = orc.init_params(seed=7)
    ck = str(tmp_path / "w.pt")
    torch.save({"net": P}, ck)
    out, dout = str(tmp_path / "win.npz"), str(tmp_path / "win_donor.npz")
    assert predict.main(["-m", meta, "-d", npy, "-w", ck, "-o", str(tmp_path / "p.csv"), "--window-shapley-out", out, "--window-players", "regions",
                         "--window-width", "10", "--window-perms", "2", "--window-seed", "9", "--window-scale", "0.5", "--donor-npy-dir", dnpy,
                         "--window-donor-shapley-out", dout]) == 0
    ds = ChromoformerDataset(meta, npy, genes)
    flips = [ds.genes[g]["tss"][2] != "+" for g in genes]
    assert any(flips) and not all(flips)
    model = ChromoformerClassifier(seed=123, max_batch=32).cuda(0)
    model.load_state_dict(P)
    store, dstore = GeneStore(ds, device=model._device, resident=True), GeneStore(dn, device=model._device, resident=True)
    d, dd = store.batch(list(range(20))), dstore.batch(list(range(20)))
    names = window_players("regions", 7, 8, 20, 10)[4]
    for path, kw in ((out, dict(scale=0.5)), (dout, dict(donor=_feats(dd)))):
        z = np.load(path)
        assert sorted(z.files) == ["absent", "chroms", "estimator", "gene_ids", "logits", "null", "permutations", "phi", "players", "stderr", "windows"]
        assert list(z["gene_ids"]) == genes and list(z["players"]) == names and str(z["estimator"]) == "sampled"
        assert np.array_equal(z["permutations"], shapley_permutations(18, 2, 9))
        assert z["phi"].shape == z["stderr"].shape == z["null"].shape == (20, 18) and z["windows"].shape == (20, 18, 2)
        phi, info = model.mark_window_shapley_sampled(*_args(d), players="regions", width=10, n_perm=2, seed=9, flip=flips, return_rows=True, **kw)
        _check_estimate(phi, info, z["null"])
        assert np.array_equal(z["phi"], phi.cpu()[..., 1].numpy()) and np.array_equal(z["stderr"], info["stderr"].cpu()[..., 1].numpy())
        assert np.array_equal(z["logits"], info["logits"].cpu()[:, 1].numpy()) and np.array_equal(z["absent"], info["absent"].cpu()[:, 1].numpy())
        for i, g in enumerate(genes):      # genomic coordinates: the promoter's two halves, each pCRE's windows from its own start
            chrom, tss, _ = ds.genes[g]["tss"]
            assert z["windows"][i, 0].tolist() == [tss - 20000, tss] and z["windows"][i, 1].tolist() == [tss, tss + 20000] and z["chroms"][i, 0] == chrom
            for j in range(8):
                pc = ds.genes[g]["pcres"][j] if j < len(ds.genes[g]["pcres"]) else None
                first, second = 2 + 2 * j, 3 + 2 * j
                assert bool(z["null"][i, first]) == (pc is None) and bool(z["null"][i, second]) == (pc is None or pc[2] - pc[1] <= 20000)
                if pc is not None:
                    assert z["windows"][i, first].tolist() == [pc[1], min(pc[1] + 20000, pc[2])] and z["chroms"][i, first] == pc[0]
                else:
                    assert z["windows"][i, first].tolist() == [-1, -1] and z["chroms"][i, first] == ""
    sig = torch.sigmoid(torch.from_numpy(np.load(out)["logits"])).numpy()
    assert np.abs(sig - pd.read_csv(str(tmp_path / "p.csv"))["prediction"].to_numpy()).max() <= 2.0 ** -23
    # the walker, in chunks of 7 genes: the exact call's bits (5 players), with and without the donor
    sub = genes[3:13]
    for donor_ds in (None, dn):
        res = list(model.mark_window_shapley_dataset(ds, donor_ds, genes=sub, players="promoter", width=4, scale=0.25, bsz=7))
        assert [r["gene_id"] for r in res] == sub
        src = GeneStore(_subset(ds, sub), device=model._device, resident=True)
        dsrc = GeneStore(_subset(dn, sub), device=model._device, resident=True) if donor_ds is not None else None
        for lo in (0, 7):
            n = min(7, 10 - lo)
            b = src.batch(list(range(lo, lo + n)))
            kw = dict(donor=_feats(dsrc.batch(list(range(lo, lo + n))))) if dsrc is not None else dict(scale=0.25)
            phi, info = model.mark_window_shapley(*_args(b), players="promoter", width=4, flip=flips[3 + lo:3 + lo + n], **kw)
            for i in range(n):
                r = res[lo + i]
                assert sorted(r) == ["absent", "estimator", "gene_id", "logits", "null", "phi", "players", "stderr", "windows"] and r["estimator"] == "exact"
                assert r["players"] == ["promoter[%d:%d]" % (g, g + 4) for g in range(0, 20, 4)] and not r["null"].any() and not r["stderr"].any()
                tss = ds.genes[r["gene_id"]]["tss"][1]
                assert [w[0][2:] for w in r["windows"]] == [(tss - 20000 + 8000 * k, tss - 12000 + 8000 * k) for k in range(5)]
                assert np.array_equal(r["phi"], phi[i].cpu().numpy()) and np.array_equal(r["logits"], info["logits"][i].cpu().numpy())
                assert np.array_equal(r["absent"], info["donor" if dsrc is not None else "erased"][i].cpu().numpy())
    with pytest.raises(ValueError, match="window_players"):
        next(model.mark_window_shapley_dataset(ds, genes=sub, players="cells"))
    far = ChromoformerDataset(os.path.join(dnpy, "meta.csv"), dnpy, genes, w_prom=38000)
    with pytest.raises(ValueError, match="same_regions: .*w_prom"):
        next(model.mark_window_shapley_dataset(ds, far, genes=sub))
