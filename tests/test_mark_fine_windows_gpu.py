"""The fine window game on the GPU (cf_mark_fine_coalitions, cf_mark_fine_shapley, cf_mark_fine_shapley_sampled; model.mark_fine_window_*):

  * bit-for-bit identities: one absent player is perturbation_scan_fine's row and feats_out; players whose windows are unions of whole
    coarse bins give mark_window_coalitions' rows, for both rules; every row is the plain forward on the batch with feats_out
    substituted; sampled rows are the prefix coalitions; the same bits whatever max_batch is, call after call, for the packed forms;
  * feats_out within the bounds of tests/test_mark_fine_windows_cpu.py of the CPU oracle (tests/fine_window_oracle.py), logits within
    1e-4 of it and of the golden, classifier and regressor, both rules; another nested shape;
  * the game: overlapping absent players change an element once, efficiency, all P! orders give the exact call, the exact call against
    float64, null players exactly 0, the all-absent tiling of a coarse window is perturbation_scan's row;
  * the launch contract, every refusal by its message with nothing launched, no side effects on training, a stale backward, the
    dataset walker and the CLI.

The three genes of so.scan_dataset(w_prom=39000): 390 real finest promoter bins, the '-' strand promoter stored mirrored, pCREs of
12,201 and 1,800 samples, a gene without partners; max_batch 4 unless stated, at most a few dozen rows per gene."""
import ctypes as C
import itertools
import os
import types

import numpy as np
import pandas as pd
import pytest
import torch

from chromoformer_amd import _lib
from chromoformer_amd.attribution import fine_window_players, mark_wide_words, shapley_permutations
from oracle import chromoformer_oracle as orc
from tests import donor_oracle as do
from tests import fine_window_oracle as fw
from tests import perm_oracle as po
from tests import scan_oracle as so
from tests.coalition_oracle import shapley_fp64
from tests.test_fine_scan_cpu import WHOLE_TOL
from tests.test_input_grads_gpu import _model
from tests.test_mark_coalitions_gpu import GENES
from tests.test_mark_donor_gpu import _dev, _feats
from tests.test_mark_fine_windows_cpu import ABSENT, FINE_PART_C, PLAYERS, golden_case
from tests.test_mark_sampled_gpu import _args, _check_estimate, _g, _host, _plain
from tests.test_pcre_coalitions_gpu import U, _gamma

pytestmark = pytest.mark.gpu
BINS = (2000, 500, 100)
ALL = tuple(range(7))
SEED = 5
TOL = 1e-4      # the project's logit bound
#: (per-gene start, per-gene length) per region: the promoter's tail and both strands, the 12,201-sample pCRE's one-sample last bin
ZOOMS = {0: ([350, 0, 17], [39000] * 3), 1: ([90, 0, 3], [12201, 1800, 0])}
KEEP = np.array([[p not in a for p in range(len(PLAYERS))] for a in ABSENT])
CELLS = fw.cells_players(7, 2, 3)      # 21 players: mark x three 200-bp windows


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """The three genes and the donor cell type: host and device batches and the promoter flips, built once, never written."""
    ds = so.scan_dataset(str(tmp_path_factory.mktemp("fine_windows")), w_prom=39000)
    dn = do.donor_dataset(ds.npy_dir, str(tmp_path_factory.mktemp("donor")), do.DONOR_SEED, w_prom=39000)
    cpu, dcpu = so.dataset_batch(ds, GENES), so.dataset_batch(dn, GENES)
    flips = [ds.genes[g]["tss"][2] != "+" for g in GENES]
    assert flips[0] and not ds.genes[GENES[2]]["pcres"]
    return types.SimpleNamespace(cpu=cpu, dev=_dev(cpu), dcpu=dcpu, ddev=_dev(dcpu), flips=flips)


@pytest.fixture(scope="module")
def small():
    """The seed-42 classifier (the golden's weights) at max_batch = 4."""
    return _model(None, False, orc.init_params(None, 42, False), 4)


@pytest.fixture(scope="module")
def wide64():
    return _model(None, False, orc.init_params(None, 42, False), 64)


@pytest.fixture(scope="module")
def cells(data, small):
    """(phi, info) of small.mark_fine_window_shapley_sampled, mark x three fine windows at each gene's own start, two orders, both rules."""
    out = {}
    for rule, kw in (("scale", {}), ("donor", dict(donor=_feats(data.ddev)))):
        phi, info = small.mark_fine_window_shapley_sampled(*_args(data.dev), **_cells_kw(data), return_rows=True, **kw)
        torch.cuda.synchronize()
        out[rule] = (phi.cpu(), _host(info))
    return out


def _cells_kw(data):
    return dict(players="cells", width=2, n_windows=3, start=ZOOMS[0][0], lengths=ZOOMS[0][1], flip=data.flips, n_perm=2, seed=SEED)


def _sub(batch, key, b, value):
    out = dict(batch)
    out[key] = dict(batch[key])
    out[key][b] = value
    return out


def _with_region(batch, region, feats, c):
    """The (device) batch with the region's features replaced by feats[b][:, c]."""
    out = batch
    for b in BINS:
        f = feats[b][:, c]
        if region == 0:
            out = _sub(out, "promoter_feats", b, f[:, None].contiguous())
        else:
            t = batch["pcre_feats"][b].clone()
            t[:, region - 1] = f
            out = _sub(out, "pcre_feats", b, t)
    return out


def _src(batch, region, b):
    return batch["promoter_feats"][b][:, 0] if region == 0 else batch["pcre_feats"][b][:, region - 1]


def _one_absent(P):
    return np.array([[q != p for q in range(P)] for p in range(P)] + [[True] * P])


@pytest.mark.parametrize("region", [0, 1])
def test_one_absent_player_is_the_fine_scan_row_and_feats_bit_for_bit(data, small, region):
    start, lengths = ZOOMS[region]
    fl = data.flips if region == 0 else None
    players = [((1, 4), (3 * g, 3 * g + 7)) for g in range(7)]
    for s in (0.0, 2.5):
        scan, sf = small.perturbation_scan_fine(*_args(data.dev), region=region, scale=s, width=7, stride=3, n_windows=7, start=start, lengths=lengths,
                                                mark_sets=[(1, 4)], flip=fl, return_feats=True)
        got, gf = small.mark_fine_window_coalitions(*_args(data.dev), keep=_one_absent(7), region=region, players=players, start=start,
                                                    lengths=lengths, scale=s, flip=fl, return_feats=True)
        assert got.shape == (3, 8, 2) and not got.requires_grad
        order = list(range(1, 8)) + [0]
        assert torch.equal(got, scan[:, order]), (region, s)
        for b in BINS:
            assert gf[b].shape == sf[b].shape and torch.equal(gf[b], sf[b][:, order]), (region, s, b)
        assert not torch.equal(got[:2, 0], got[:2, 7])
    if region == 1:      # bins 121 and 122 of the 12,201-sample pCRE: its last bin holds one sample, so lengths re-weights the 500-bp bin
        kw = dict(keep=_one_absent(1), region=1, players=[(ALL, (0, 2))], start=[121, 0, 3], scale=0.0)
        full = small.mark_fine_window_coalitions(*_args(data.dev), **kw)
        true = small.mark_fine_window_coalitions(*_args(data.dev), lengths=lengths, **kw)
        ref = small.perturbation_scan_fine(*_args(data.dev), region=1, scale=0.0, width=2, n_windows=1, start=[121, 0, 3], lengths=lengths, mark_sets=[ALL])
        assert torch.equal(true, ref[:, [1, 0]]) and not torch.equal(full[0], true[0])


@pytest.mark.parametrize("rule", ["scale", "donor"])
def test_whole_coarse_bin_players_are_the_window_game_bit_for_bit(data, small, rule):
    fine = [((1, 4), (0, 40)), (ALL, (40, 60)), ((3,), (20, 100)), ((0, 6), (340, 380))]      # start 20: coarse bins 1..3, 3..4, 2..6, 18..20
    words = [0, 1, 2, 4, 8, 5, 10, 15]
    for region in (0, 1):
        coarse = [(ms, (region,), (1 + lo // 20, 1 + hi // 20)) for ms, (lo, hi) in fine]
        for kw in ((dict(scale=0.0), dict(scale=2.5)) if rule == "scale" else (dict(donor=_feats(data.ddev)),)):
            got = small.mark_fine_window_coalitions(*_args(data.dev), keep=words, region=region, players=fine, start=20,
                                                    flip=data.flips if region == 0 else None, **kw).cpu()      # (flip is the scan's: it mirrors the region it is given)
            ref = small.mark_window_coalitions(*_args(data.dev), keep=words, players=coarse, flip=data.flips, **kw).cpu()
            assert got.shape == (3, 8, 2) and torch.equal(got, ref), (region, sorted(kw))
        assert not torch.equal(got[:2, 0], got[:2, 7])


@pytest.mark.parametrize("rule", ["scale", "donor"])
def test_features_against_the_cpu_oracle_and_rows_are_the_plain_forward(data, small, rule):
    """Several absent players with different mark sets, overlapping windows, several partly covered bins at once."""
    kw = dict(scale=2.5) if rule == "scale" else dict(donor=_feats(data.ddev))
    okw = dict(scale=2.5) if rule == "scale" else dict(donor=data.dcpu)
    n_part = mixed = 0
    for region, (start, lengths) in ZOOMS.items():
        fl = data.flips if region == 0 else None
        lg, feats = small.mark_fine_window_coalitions(*_args(data.dev), keep=KEEP, region=region, players=PLAYERS, start=start, lengths=lengths,
                                                      flip=fl, return_feats=True, **kw)
        ref, _, kinds, extra = fw.fine_window_rows(data.cpu, PLAYERS, KEEP, region=region, start=start, lengths=lengths, flip=fl, **okw)
        lg = lg.cpu()
        assert lg.shape == (3, 6, 2)
        worst = ratio = 0.0
        for b in BINS:
            got = feats[b].cpu()
            assert not torch.isnan(got).any()
            src = _src(data.cpu, region, b)[:, None].expand_as(got)
            assert torch.equal(got[:, 5], src[:, 5])                              # nobody absent
            assert bool(((got != src) <= (kinds[b] != fw.NONE)).all())            # elements nobody covers keep their bits
            err = (got.double() - ref[b].double()).abs()
            part = kinds[b] == fw.PART
            fac = fw.bound_factor(src, ref[b], kinds[b], extra[b])
            worst = max(worst, err[~part].max().item())
            n_part += int(part.sum())
            mixed += int((kinds[b] != kinds[b][..., :1]).any(-1).sum())
            if part.any():
                ratio = max(ratio, (err[part] / (2.0 ** -24 * fac[part])).max().item())
            assert bool((err <= torch.where(part, FINE_PART_C * 2.0 ** -24 * fac, torch.full_like(fac, WHOLE_TOL))).all()), (region, b)
        print("%s region %d: whole %.3e (bound %.1e), partly covered ratio %.3f (bound %.2f)" % (rule, region, worst, WHOLE_TOL, ratio, FINE_PART_C))
        for c in range(6):
            assert torch.equal(lg[:, c], _plain(small, _with_region(data.dev, region, feats, c))), (region, c)
    assert n_part > 20 and mixed > 0


@pytest.mark.parametrize("regression", [False, True], ids=["classifier", "regressor"])
def test_logits_against_the_oracle_and_the_golden(data, regression):
    from tests.helpers import GOLDEN
    P = orc.init_params(None, 42, regression)
    model = _model(None, regression, P, 4)
    keep = KEEP[[0, 3]]
    for region, (start, lengths) in ZOOMS.items():
        fl = data.flips if region == 0 else None
        for kw, okw in ((dict(scale=0.0), dict(scale=0.0)), (dict(donor=_feats(data.ddev)), dict(donor=data.dcpu))):
            got = model.mark_fine_window_coalitions(*_args(data.dev), keep=keep, region=region, players=PLAYERS, start=start, lengths=lengths, flip=fl,
                                                    **kw).cpu()
            ora = fw.oracle_fine_window(P, data.cpu, PLAYERS, keep, region=region, start=start, lengths=lengths, flip=fl, **okw)[0]
            d = (got - ora).abs().max().item()
            print("region", region, sorted(kw), "vs oracle %.2e" % d)
            assert got.shape == (3, 2, 1 if regression else 2) and d < TOL, (region, d)
    z = np.load(os.path.join(GOLDEN, "fine_window.npz"))
    assert [str(g) for g in z["genes"]] == GENES and int(z["w_prom"]) == 39000 and int(z["donor_seed"]) == do.DONOR_SEED
    for k in range(len(z["scales"])):
        players, present, region, start = golden_case(z, k)
        kw = dict(donor=_feats(data.ddev)) if z["donor"][k] else dict(scale=float(z["scales"][k]))
        got = model.mark_fine_window_coalitions(*_args(data.dev), keep=np.array([present]), region=region, players=players, start=start,
                                                lengths=z["lengths"][k].tolist(), flip=data.flips if region == 0 else None, **kw).cpu()[:, 0]
        gold = torch.from_numpy(z["reg" if regression else "clf"][k])
        d = (got - gold).abs().max().item()
        print("case", k, "vs golden %.2e" % d)
        assert got.shape == gold.shape and d < TOL, (k, d)


def test_another_nested_shape():
    """binsizes 2000 / 1000 / 500: R = 4 and 2, 80 finest bins; features and logits against the oracle.  The features of
    orc.synthetic_batch are drawn per resolution, not binned from one signal, and only s >= 1 keeps 1 + m' > 0 on them; the donor is the
    gene's own signal scaled by 2.5 at every resolution, for the same reason."""
    cfg = orc._cfg(dict(binsizes=[2000, 1000, 500], w_max=40000))
    cpu = orc.synthetic_batch(2, cfg=cfg, seed=13, regime="realistic")
    don = dict(cpu, promoter_feats={b: so.rule(t, 2.5) for b, t in cpu["promoter_feats"].items()},
               pcre_feats={b: so.rule(t, 2.5) for b, t in cpu["pcre_feats"].items()})
    P = orc.init_params(cfg, 3, False)
    model = _model(cfg, False, P, 3)
    players = [((1, 4), (0, 3)), ((0, 1, 2), (2, 9)), (ALL, (9, 10)), ((5,), (70, 90))]
    keep = [0, 5, 10, 15]
    for region, fl in ((0, [True, False]), (2, None)):
        for kw, okw in ((dict(scale=2.5), dict(scale=2.5)), (dict(donor=_feats(_dev(don))), dict(donor=don))):
            lg, feats = model.mark_fine_window_coalitions(*_args(_dev(cpu)), keep=keep, region=region, players=players, start=[1, 6], flip=fl,
                                                          return_feats=True, **kw)
            ora, ref, kinds, extra = fw.oracle_fine_window(P, cpu, players, keep, cfg, region=region, start=[1, 6], flip=fl, **okw)
            d = (lg.cpu() - ora).abs().max().item()
            print("region", region, sorted(kw), "vs oracle %.2e" % d)
            assert d < TOL, (region, d)
            for b in (2000, 1000, 500):
                src = _src(cpu, region, b)[:, None].expand_as(ref[b])
                err = (feats[b].cpu().double() - ref[b].double()).abs()
                fac = fw.bound_factor(src, ref[b], kinds[b], extra[b])
                assert bool((err <= torch.where(kinds[b] == fw.PART, FINE_PART_C * 2.0 ** -24 * fac, torch.full_like(fac, WHOLE_TOL))).all()), (region, b)
            assert any((kinds[b] == fw.PART).any() for b in (2000, 1000))


@pytest.mark.parametrize("rule", ["scale", "donor"])
def test_sampled_rows_are_the_prefix_coalitions_and_the_estimate(data, small, cells, rule):
    phi, info = cells[rule]
    perms, rows = info["permutations"], info["rows"]
    assert perms.shape == (2, 21) and np.array_equal(perms, shapley_permutations(21, 2, SEED))
    assert rows.shape == (3, 2 + 2 * 20, 2) and phi.shape == info["stderr"].shape == (3, 21, 2) and not phi.requires_grad
    assert info["names"] == fine_window_players("cells", 7, 2, 3)[3] and info["names"][8] == "mark1@fine[2:4]"
    assert sorted(info) == ["absent", "delta", "logits", "names", "permutations", "rows", "stderr"]
    assert torch.equal(rows[:, 1], _plain(small, data.dev))
    kw = dict(donor=_feats(data.ddev)) if rule == "donor" else {}
    got = small.mark_fine_window_coalitions(*_args(data.dev), keep=po.prefix_words(perms), players=CELLS, start=ZOOMS[0][0], lengths=ZOOMS[0][1],
                                            flip=data.flips, **kw).cpu()
    assert torch.equal(got, rows)
    _check_estimate(phi, info)
    assert float((phi != 0).any(-1).float().mean()) > 0.9


def test_same_bits_for_every_max_batch_call_after_call_and_packed_forms(data, small, cells, wide64):
    from chromoformer_amd.engine import Slot
    for cap in (7, 64):
        model = wide64 if cap == 64 else _model(None, False, orc.init_params(None, 42, False), cap)
        for rule, kw in (("scale", {}), ("donor", dict(donor=_feats(data.ddev)))):
            p, i = model.mark_fine_window_shapley_sampled(*_args(data.dev), **_cells_kw(data), return_rows=True, **kw)
            ref, rinfo = cells[rule]
            assert torch.equal(p.cpu(), ref) and torch.equal(i["stderr"].cpu(), rinfo["stderr"]) and torch.equal(i["rows"].cpu(), rinfo["rows"]), cap
    for packed in (small.pack_batch(data.dev), Slot(small, 3).fill(small, data.dev)):
        p, i = small.mark_fine_window_shapley_sampled(packed, **_cells_kw(data), return_rows=True)
        assert torch.equal(p.cpu(), cells["scale"][0]) and torch.equal(i["rows"].cpu(), cells["scale"][1]["rows"])
    kw = dict(players=PLAYERS[:4], start=ZOOMS[0][0], flip=data.flips, scale=2.5)
    exact = [m.mark_fine_window_shapley(*_args(data.dev), **kw)[0].cpu() for m in (wide64, small, wide64)]
    assert torch.equal(exact[0], exact[1]) and torch.equal(exact[0], exact[2])


def test_overlapping_absent_players_change_an_element_once(data, small):
    pair = [((1, 4), (3, 31)), ((1, 4), (17, 52))]
    kw = dict(start=ZOOMS[0][0], flip=data.flips, scale=2.5, return_feats=True)
    got, gf = small.mark_fine_window_coalitions(*_args(data.dev), keep=[0, 1, 2, 3], players=pair, **kw)
    ref, rf = small.mark_fine_window_coalitions(*_args(data.dev), keep=[0, 1], players=[((1, 4), (3, 52))], **kw)
    assert torch.equal(got[:, 0], ref[:, 0]) and torch.equal(got[:, 3], ref[:, 1])
    assert all(torch.equal(gf[b][:, 0], rf[b][:, 0]) for b in BINS)
    assert not torch.equal(got[:2, 1], got[:2, 0]) and not torch.equal(got[:2, 2], got[:2, 0])


def test_all_orders_give_the_exact_call_and_the_exact_call_float64(data, small):
    four = PLAYERS[:4]
    every = np.array(list(itertools.permutations(range(4))), dtype=np.uint8)
    for kw in (dict(scale=0.0), dict(scale=2.5), dict(donor=_feats(data.ddev))):
        kw = dict(kw, players=four, start=ZOOMS[0][0], lengths=ZOOMS[0][1], flip=data.flips)
        ref, rinfo = small.mark_fine_window_shapley(*_args(data.dev), return_coalitions=True, **kw)
        table = rinfo["coalitions"].cpu()
        absent = "donor" if "donor" in kw else "erased"
        assert sorted(rinfo) == sorted(["coalitions", "delta", absent, "logits", "players"]) and table.shape == (3, 16, 2)
        assert torch.equal(table[:, 15], _plain(small, data.dev)) and torch.equal(rinfo[absent].cpu(), table[:, 0])
        assert torch.equal(table, small.mark_fine_window_coalitions(*_args(data.dev), keep=list(range(16)), **kw).cpu())
        phi64, scale = shapley_fp64(table.numpy())
        err = np.abs(ref.cpu().numpy().astype(np.float64) - phi64)
        assert (err <= _gamma(4) * scale).all()
        dbound = 4 * (_gamma(4) * scale).max(1) + 4 * U * np.abs(table.numpy()).max(1)
        assert (np.abs(rinfo["delta"].cpu().numpy()) <= dbound).all()      # phi.sum(1) = logits - absent up to rounding
        phi, info = small.mark_fine_window_shapley_sampled(*_args(data.dev), permutations=every, return_rows=True, **kw)
        assert torch.equal(info["rows"].cpu(), table[:, [int(m) for m in po.prefix_words(every)]])
        _check_estimate(phi, info)
        d = po.marginals(info["rows"].cpu().numpy(), every, np.float32)
        bound = _g(24 + 1) * np.abs(d.astype(np.float64)).mean(1) + _gamma(4) * scale
        err = np.abs(phi.cpu().numpy().astype(np.float64) - ref.cpu().numpy().astype(np.float64))
        assert (err <= bound).all(), (err.max(), bound.max())
        assert bool((ref[:2] != 0).any(-1).all())


def test_null_players_are_exactly_zero(data, small):
    # windows past bin 390, beside real ones
    players = [(ALL, (0, 5)), ((1, 4), (40, 47)), (ALL, (45, 60))]      # start 350: [350, 355), [390, 397), [395, 410)
    for fn in ("exact", "sampled"):
        kw = dict(players=players, start=350, flip=data.flips)
        if fn == "exact":
            phi, info = small.mark_fine_window_shapley(*_args(data.dev), **kw)
        else:
            phi, info = small.mark_fine_window_shapley_sampled(*_args(data.dev), n_perm=3, **kw)
            assert bool((info["stderr"][:, 1:] == 0).all())
        assert bool((phi[:, 1:] == 0).all()) and bool((phi[:, 0] != 0).all())
    # start = 2^31 - 1: every window is past the region, no overflow
    phi, info = small.mark_fine_window_shapley_sampled(*_args(data.dev), players="windows", width=2, n_windows=3, start=[2 ** 31 - 1, 0, 2 ** 31 - 1],
                                                       n_perm=2, flip=data.flips)
    assert bool((phi[[0, 2]] == 0).all()) and bool((info["stderr"][[0, 2]] == 0).all()) and bool((phi[1] != 0).all())
    assert torch.equal(info["absent"][[0, 2]], info["logits"][[0, 2]])
    # pCRE slot 7 is a dummy slot of gene 2 (and of every gene here without eight partners)
    phi, info = small.mark_fine_window_shapley(*_args(data.dev), region=8, players="windows", width=4, n_windows=3)
    assert bool((phi[2] == 0).all())
    phi, info = small.mark_fine_window_shapley(*_args(data.dev), region=1, players="windows", width=4, n_windows=3)
    assert bool((phi[2] == 0).all()) and bool((phi[:2] != 0).all())
    # a donor equal to the gene inside the window: wholly and partly covered bins keep their bits
    don = {b: t.clone() for b, t in data.ddev["promoter_feats"].items()}
    for b in BINS:      # genomic finest bins [40, 60) of the '+' strand gene 1: every resolution's rows that hold them
        R, q = b // 100, so.extent(so.centre_row(data.cpu["promoter_pad_masks"][b], 3, 40000 // b)[1])[0]
        don[b][1, 0, q + 40 // R:q - (-60 // R)] = data.dev["promoter_feats"][b][1, 0, q + 40 // R:q - (-60 // R)]
    players = [(ALL, (43, 57)), ((2,), (100, 110))]
    phi, info = small.mark_fine_window_shapley_sampled(*_args(data.dev), players=players, n_perm=2, flip=data.flips,
                                                       donor=(don, data.ddev["pcre_feats"]))
    assert bool((phi[1, 0] == 0).all()) and bool((info["stderr"][1, 0] == 0).all()) and bool((phi[1, 1] != 0).all()) and bool((phi[0, 0] != 0).all())


def test_players_tiling_a_coarse_window_sum_to_the_scan_effect(data, small):
    scan = small.perturbation_scan(*_args(data.dev), region=0, scale=0.0, width=1, mark_sets=[ALL], flip=data.flips).cpu()
    zoom = [19, 4, 11]      # gene 0: the narrowed promoter's short last coarse bin (ten children)
    phi, info = small.mark_fine_window_shapley_sampled(*_args(data.dev), players="windows", width=4, n_windows=5, start=[20 * z for z in zoom],
                                                       lengths=[39000] * 3, n_perm=2, seed=SEED, flip=data.flips, return_rows=True)
    row = torch.stack([scan[i, 1 + z] for i, z in enumerate(zoom)])
    assert torch.equal(info["absent"].cpu(), row) and torch.equal(info["logits"].cpu(), scan[:, 0])
    _check_estimate(phi, _host(info))      # delta: phi.sum(1) = logits - the scan's row, up to rounding
    assert bool((phi[0, 3:] == 0).all()) and bool((phi[0, :3] != 0).all())      # windows 3 and 4 lie past bin 390


@pytest.mark.parametrize("cap", [64, 7])
def test_launch_contract(data, cap, wide64):
    model = wide64 if cap == 64 else _model(None, False, orc.init_params(None, 42, False), cap)
    _plain(model, data.dev)
    n_fwd = model.launch_counts()[0]
    chunks = lambda rows: -(-rows // cap)      # noqa: E731
    model.mark_fine_window_coalitions(*_args(data.dev), keep=KEEP, players=PLAYERS, start=ZOOMS[0][0], lengths=ZOOMS[0][1], return_feats=True)
    assert model.launch_counts()[0] == chunks(3 * 6) * (1 + n_fwd)
    model.mark_fine_window_coalitions(*_args(data.dev), keep=[0, 5], region=1, players=PLAYERS[:3], donor=_feats(data.ddev))
    assert model.launch_counts()[0] == chunks(3 * 2) * (1 + n_fwd)
    model.mark_fine_window_shapley(*_args(data.dev), players="windows", width=5, n_windows=4)
    assert model.launch_counts()[0] == chunks(3 * 16) * (1 + n_fwd) + 1
    model.mark_fine_window_shapley_sampled(*_args(data.dev), players="cells", width=2, n_windows=3, n_perm=3)
    assert model.launch_counts()[0] == chunks(3 * (2 + 3 * 20)) * (1 + n_fwd) + 1


def _ints(*v):
    return (C.c_int * len(v))(*v)


def _raw_opts(game, region=0, scale=0.0, n_players=None, start=None, lengths=None, don_p=(None,) * 3, don_c=(None,) * 3, **over):
    pm, lo, hi = (over.get(k, v) for k, v in zip(("marks", "lo", "hi"), game[:3]))
    o = _lib.cf_mark_fine_opts()
    o.region, o.n_players, o.scale = region, len(game[0]) if n_players is None else n_players, scale
    o.player_marks, o.player_lo, o.player_hi = (a.ctypes.data if a is not None else None for a in (pm, lo, hi))
    o.start = C.cast(start, C.c_void_p) if start is not None else None
    o.lengths = C.cast(lengths, C.c_void_p) if lengths is not None else None
    for r in range(3):
        o.donor_promoter_feats[r], o.donor_pcre_feats[r] = don_p[r], don_c[r]
    return o, (pm, lo, hi, start, lengths)


def test_refusals_by_name_with_nothing_launched(data):
    L = _lib.lib()
    model = _model(None, False, orc.init_params(None, 42, False), 4)
    bs, keep_alive = model.pack_batch(data.dev)
    dbs, donor_alive = model.pack_batch(data.ddev)
    _plain(model, data.dev)
    f0 = model.launch_counts()
    st = torch.cuda.current_stream().cuda_stream
    out = torch.full((3, 64, 2), float("nan"), device="cuda")
    game = fine_window_players("cells", 7, 2, 3)
    words = mark_wide_words([0, 1, (1 << 21) - 1, 1 << 20], 21)
    perms = shapley_permutations(21, 2, 0)
    big = _lib.cf_batch.from_buffer_copy(bs)
    big.B = 5
    dp, dc = tuple(dbs.promoter_feats[r] for r in range(3)), tuple(dbs.pcre_feats[r] for r in range(3))

    def edited(a, p, v):
        a = a.copy()
        a[p] = v
        return a

    many = np.ones(129, dtype=np.uint32)
    bad_opts = [(dict(n_players=0), b"n_players = 0 outside 1..128"),
                (dict(n_players=129, marks=many, lo=np.zeros(129, np.int32), hi=np.ones(129, np.int32)), b"n_players = 129 outside 1..128"),
                (dict(marks=None), b"null player_marks"), (dict(lo=None), b"null player_lo / player_hi"), (dict(hi=None), b"null player_lo / player_hi"),
                (dict(marks=edited(game[0], 12, 0)), b"player_marks[12] = 0"), (dict(marks=edited(game[0], 1, 0x80)), b"n_feats"),
                (dict(lo=edited(game[1], 13, -1)), b"player 13 has the window [-1,"), (dict(lo=edited(game[1], 7, 4)), b"player 7 has the window [4, 4)"),
                (dict(hi=edited(game[2], 20, 3)), b"player 20 has the window [4, 3)"),
                (dict(region=-1), b"region = -1 outside [0, i_max = 8]"), (dict(region=9), b"region = 9 outside"),
                (dict(start=_ints(0, -3, 0)), b"start[1] = -3"), (dict(lengths=_ints(39000, 39000, 38900)), b"lengths[2] = 38900 outside"),
                (dict(lengths=_ints(39001, 39000, 39000)), b"lengths[0] = 39001 outside"),
                (dict(scale=-0.5), b"scale"), (dict(scale=float("inf")), b"scale"), (dict(scale=float("nan")), b"scale"),
                (dict(don_p=dp), b"donor_promoter_feats / donor_pcre_feats"), (dict(don_p=dp, don_c=(dc[0], None, dc[2])), b"donor_promoter_feats / donor_pcre_feats"),
                (dict(don_c=(None, dc[1], None)), b"are null")]
    entries = [(b"cf_mark_fine_coalitions", lambda h, b, o, dst: L.cf_mark_fine_coalitions(h, b, o, words.ctypes.data, 4, dst, st)),
               (b"cf_mark_fine_shapley_sampled", lambda h, b, o, dst: L.cf_mark_fine_shapley_sampled(h, b, o, perms.ctypes.data, 2, dst, None, None, st))]

    def refused(rc, *needles):
        err = L.cf_last_error()
        assert rc != 0 and all(n in err for n in needles), err

    for name, fn in entries:
        good, alive = _raw_opts(game)
        refused(fn(None, C.byref(bs), C.byref(good), out.data_ptr()), name, b"null handle")
        refused(fn(model._handle, None, C.byref(good), out.data_ptr()), name, b"null batch")
        refused(fn(model._handle, C.byref(bs), None, out.data_ptr()), name, b"null opts")
        refused(fn(model._handle, C.byref(bs), C.byref(good), None), name, b"null logits" if b"coalitions" in name else b"null phi")
        refused(fn(model._handle, C.byref(big), C.byref(good), out.data_ptr()), name, b"max_batch")
        for kw, msg in bad_opts:
            o, alive = _raw_opts(game, **kw)
            refused(fn(model._handle, C.byref(bs), C.byref(o), out.data_ptr()), name, msg)
    good, alive = _raw_opts(game)
    name = b"cf_mark_fine_coalitions"
    refused(L.cf_mark_fine_coalitions(model._handle, C.byref(bs), C.byref(good), None, 4, out.data_ptr(), st), name, b"null keep")
    refused(L.cf_mark_fine_coalitions(model._handle, C.byref(bs), C.byref(good), words.ctypes.data, 0, out.data_ptr(), st), name, b"n_coal")
    bad = words.copy()
    bad[3, 0] |= 1 << 21      # player 21 of 21
    refused(L.cf_mark_fine_coalitions(model._handle, C.byref(bs), C.byref(good), bad.ctypes.data, 4, out.data_ptr(), st), name, b"keep[3]", b"n_players = 21")
    name = b"cf_mark_fine_shapley_sampled"
    refused(L.cf_mark_fine_shapley_sampled(model._handle, C.byref(bs), C.byref(good), None, 2, out.data_ptr(), None, None, st), name, b"null perms")
    refused(L.cf_mark_fine_shapley_sampled(model._handle, C.byref(bs), C.byref(good), perms.ctypes.data, 0, out.data_ptr(), None, None, st), name, b"n_perm = 0")
    twice = perms.copy()
    twice[1, 5] = twice[1, 6]
    refused(L.cf_mark_fine_shapley_sampled(model._handle, C.byref(bs), C.byref(good), twice.ctypes.data, 2, out.data_ptr(), None, None, st), name, b"perms[1]",
            b"not a permutation")
    name = b"cf_mark_fine_shapley"      # the exact call: at most 16 players
    refused(L.cf_mark_fine_shapley(model._handle, C.byref(bs), C.byref(good), out.data_ptr(), None, st), name, b"n_players = 21 outside 1..16")
    four = fine_window_players("windows", 7, 5, 4)
    refused(L.cf_mark_fine_shapley(model._handle, C.byref(bs), C.byref(_raw_opts(four)[0]), None, None, st), name, b"null phi")
    refused(L.cf_mark_fine_shapley(model._handle, C.byref(bs), C.byref(_raw_opts(four, lo=edited(four[1], 2, 15))[0]), out.data_ptr(), None, st), name,
            b"player 2 has the window [15, 15)")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and model.launch_counts() == f0      # nothing was launched
    # geometry: bin counts that do not nest, and more than 512 finest bins
    for over, msg in ((dict(binsizes=[2000, 800, 100], w_max=40000), b"n_bins[1] = 50 is not a multiple of the coarsest resolution's 20 bins"),
                      (dict(binsizes=[2000, 500, 50], w_max=40000), b"n_bins[2] = 800 bins; the window table holds at most 512")):
        cfg = orc._cfg(over)
        odd = _model(cfg, False, orc.init_params(cfg, 3, False), 2)
        ob, odd_alive = odd.pack_batch(_dev(orc.synthetic_batch(2, cfg=cfg, seed=1, regime="realistic")))
        o, alive = _raw_opts(four)
        odd_out = torch.full((2, 4, 2), float("nan"), device="cuda")
        w4 = mark_wide_words([0, 1], 4)
        n0 = odd.launch_counts()
        refused(L.cf_mark_fine_coalitions(odd._handle, C.byref(ob), C.byref(o), w4.ctypes.data, 2, odd_out.data_ptr(), st), b"cf_mark_fine_coalitions", msg)
        torch.cuda.synchronize()
        assert bool(torch.isnan(odd_out).all()) and odd.launch_counts() == n0
        del odd_alive
    # accepted: the largest start, a length at the edge, the donor rule with a scale it does not read; a dummy slot's length is not read
    for kw in (dict(start=_ints(2 ** 31 - 1, 0, 5)), dict(lengths=_ints(38901, 39000, 39000)), dict(scale=-1.0, don_p=dp, don_c=dc),
               dict(region=1, lengths=_ints(12201, 1800, -7))):
        o, alive = _raw_opts(game, **kw)
        assert L.cf_mark_fine_coalitions(model._handle, C.byref(bs), C.byref(o), words.ctypes.data, 1, out.data_ptr(), st) == 0, L.cf_last_error()
    torch.cuda.synchronize()
    out.fill_(float("nan"))
    # armed riders (a training step in flight): refused; the handle is not used again
    assert L.cf_rider_arm(model._handle, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, 0, 8) == 0, L.cf_last_error()
    for name, fn in entries:
        refused(fn(model._handle, C.byref(bs), C.byref(good), out.data_ptr()), name, b"riders")
    refused(L.cf_mark_fine_shapley(model._handle, C.byref(bs), C.byref(_raw_opts(four)[0]), out.data_ptr(), None, st), b"cf_mark_fine_shapley", b"riders")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    for kw in (dict(players="promoter"), dict(players="cells", n_windows=20), dict(players=[((7,), (0, 1))]), dict(players=[(ALL, (3, 3))]), dict(keep=[1 << 20]),
               dict(keep=[-1]), dict(start=[0, 1])):      # (raised before the library is called)
        with pytest.raises(ValueError, match="fine_window_players|mark_fine_window_coalitions"):
            model.mark_fine_window_coalitions((bs, keep_alive), **dict(dict(keep=[0], n_windows=4), **kw))
    with pytest.raises(ValueError, match="keep is required"):
        model.mark_fine_window_coalitions((bs, keep_alive))
    with pytest.raises(ValueError, match="mark_fine_window_shapley: 20 players"):
        model.mark_fine_window_shapley((bs, keep_alive), n_windows=20)
    with pytest.raises(ValueError, match="mark_fine_window_shapley_sampled: permutations"):
        model.mark_fine_window_shapley_sampled((bs, keep_alive), n_windows=20, permutations=np.zeros((2, 19), dtype=np.int64))
    with pytest.raises(ValueError, match="flip has 2 entries"):
        model.mark_fine_window_coalitions((bs, keep_alive), keep=[0], n_windows=2, flip=[True, False])
    with pytest.raises(ValueError, match="lengths has 2 entries"):
        model.mark_fine_window_coalitions((bs, keep_alive), keep=[0], n_windows=2, lengths=[1, 2])
    del keep_alive, donor_alive, alive


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
            model.mark_fine_window_shapley_sampled(*_args(dev), players="windows", width=3, n_windows=5, start=40, n_perm=2, scale=2.0)
            model.mark_fine_window_shapley(*_args(dev), region=2, players="windows", width=7, n_windows=3, donor=_feats(_dev(batches[1])))
            model.mark_fine_window_coalitions(*_args(dev), keep=[0, 1 << 20], players="cells", width=2, n_windows=3, flip=[True] * 8)
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
        for method, kw in (("mark_fine_window_shapley_sampled", dict(n_windows=3, n_perm=1)), ("mark_fine_window_shapley", dict(width=10, n_windows=2)),
                           ("mark_fine_window_coalitions", dict(keep=[0], n_windows=2))):
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
    ds = ChromoformerDataset(meta, npy, genes)
    model = ChromoformerClassifier(seed=123, max_batch=32).cuda(0)
    model.load_state_dict(P)
    sub = genes[3:9]
    flips = [ds.genes[g]["tss"][2] != "+" for g in sub]
    # the walker with zoom = 1 on pCRE slot 1, in chunks of 4 genes, coarse windows of 5 bins (4 players: exact), fine windows of 25 bins
    for donor_ds in (None, dn):
        res = list(model.mark_fine_window_shapley_dataset(ds, donor_ds, genes=sub, region=1, zoom=1, coarse_width=5, width=25, scale=0.25, bsz=4))
        assert [r["gene_id"] for r in res] == sub
        src = GeneStore(_subset(ds, sub), device=model._device, resident=True)
        dsrc = GeneStore(_subset(dn, sub), device=model._device, resident=True) if donor_ds is not None else None
        seen = 0
        for lo in (0, 4):
            n = min(4, 6 - lo)
            b = src.batch(list(range(lo, lo + n)))
            kw = dict(donor=_feats(dsrc.batch(list(range(lo, lo + n))))) if dsrc is not None else dict(scale=0.25)
            coarse = [(ALL, (2,), (g, g + 5)) for g in range(0, 20, 5)]
            cphi, cinfo = model.mark_window_shapley(*_args(b), players=coarse, flip=[False] * n, **kw)
            starts = [100 * int(x["zoom"][0]) if len(x["zoom"]) else 400 for x in res[lo:lo + n]]
            lengths = [x["region"][2] - x["region"][1] if x["region"] else 0 for x in res[lo:lo + n]]
            phi, info = model.mark_fine_window_shapley(*_args(b), region=2, players="windows", width=25, n_windows=4, start=starts, lengths=lengths, **kw)
            for i in range(n):
                r = res[lo + i]
                assert sorted(r) == ["absent", "coarse_phi", "coarse_windows", "exact", "gene_id", "index", "logits", "phi", "players", "rank", "region",
                                     "stderr", "windows", "zoom"]
                pcs = ds.genes[r["gene_id"]]["pcres"]
                if len(pcs) < 2:      # a gene without the slot yields no players
                    assert r["region"] is None and r["players"] == [] and r["windows"] == [] and r["phi"].shape == (0, 2) and len(r["zoom"]) == 0
                    continue
                seen += 1
                chrom, s, e = pcs[1]
                n_cw = -(-(-(-(e - s) // 2000)) // 5)
                assert r["region"] == (chrom, s, e) and r["exact"] and r["stderr"] is None and r["coarse_phi"].shape == (n_cw, 2)
                assert np.array_equal(r["coarse_phi"], cphi[i, :n_cw].cpu().numpy())
                z = int(r["zoom"][0])
                assert len(r["zoom"]) == 1 and z == int(np.argmax(np.abs(r["coarse_phi"][:, 1])))      # the chosen coarse window: argmax |coarse_phi|
                assert r["coarse_windows"][z] == (chrom, s + z * 10000, min(s + (z + 1) * 10000, e))
                first = s + z * 10000
                real = [g for g in range(4) if first + g * 2500 < e]
                assert r["players"] == ["fine[%d:%d]" % (25 * g, 25 * g + 25) for g in real] and r["index"].tolist() == real
                assert r["windows"] == [(chrom, first + g * 2500, min(first + (g + 1) * 2500, e)) for g in real]      # genomic coordinates
                assert np.array_equal(r["phi"], phi[i, real].cpu().numpy()) and np.array_equal(r["logits"], info["logits"][i].cpu().numpy())
                assert np.array_equal(r["absent"][0], info["donor" if dsrc is not None else "erased"][i].cpu().numpy())
        assert 0 < seen
    del flips
    with pytest.raises(ValueError, match="fine_window_players"):
        next(model.mark_fine_window_shapley_dataset(ds, genes=sub, players="cells", width=1))
    with pytest.raises(ValueError, match="region"):
        next(model.mark_fine_window_shapley_dataset(ds, genes=sub, region=8))
    far = ChromoformerDataset(os.path.join(dnpy, "meta.csv"), dnpy, genes, w_prom=38000)
    with pytest.raises(ValueError, match="same_regions: .*w_prom"):
        next(model.mark_fine_window_shapley_dataset(ds, far, genes=sub))
    # the CLI: the promoter, cells at width 20 (7 players, exact), the coarse game sampled with two orders
    out, dout = str(tmp_path / "fw.npz"), str(tmp_path / "fw_donor.npz")
    assert predict.main(["-m", meta, "-d", npy, "-w", ck, "-o", str(tmp_path / "p.csv"), "--fine-window-shapley-out", out, "--fine-window-players", "cells",
                         "--fine-window-width", "20", "--fine-window-perms", "2", "--fine-window-seed", "9", "--fine-window-scale", "0.5",
                         "--donor-npy-dir", dnpy, "--fine-window-donor-shapley-out", dout]) == 0
    names = fine_window_players("cells", 7, 20, 1)[3]
    for path in (out, dout):
        z = np.load(path)
        assert sorted(z.files) == ["absent", "chroms", "coarse_phi", "exact", "gene_ids", "logits", "null", "phi", "players", "stderr", "windows", "zoom"]
        assert list(z["gene_ids"]) == genes and list(z["players"]) == names and bool(z["exact"])
        assert z["phi"].shape == z["stderr"].shape == z["null"].shape == (20, 1, 7) and z["windows"].shape == (20, 1, 7, 2) and z["zoom"].shape == (20, 1)
        assert z["coarse_phi"].shape == (20, 20) and not z["null"].any() and not np.isnan(z["coarse_phi"]).any() and not z["stderr"].any()
        for i, g in enumerate(genes):
            chrom, tss, _ = ds.genes[g]["tss"]
            zi = int(z["zoom"][i, 0])
            assert zi == int(np.argmax(np.abs(z["coarse_phi"][i]))) and z["chroms"][i] == chrom
            assert z["windows"][i, 0, 0].tolist() == z["windows"][i, 0, 6].tolist() == [tss - 20000 + 2000 * zi, tss - 18000 + 2000 * zi]
        gap = np.abs(z["phi"].sum(-1)[:, 0] - (z["logits"] - z["absent"][:, 0]))
        assert gap.max() < 1e-5
    sig = torch.sigmoid(torch.from_numpy(np.load(out)["logits"])).numpy()
    assert np.abs(sig - pd.read_csv(str(tmp_path / "p.csv"))["prediction"].to_numpy()).max() <= 2.0 ** -23
    for bad in (["--fine-window-width", "3"], ["--fine-window-shapley-out", out, "--fine-window-width", "0"], ["--fine-window-donor-shapley-out", dout],
                ["--fine-window-shapley-out", out, "--fine-window-players", "cells", "--fine-window-width", "1"],
                ["--fine-window-donor-shapley-out", dout, "--donor-npy-dir", dnpy, "--fine-window-scale", "0.5"],
                ["--fine-window-shapley-out", out, "--fine-window-region", "9"], ["--fine-window-shapley-out", out, "--fine-window-zoom", "0"],
                ["--fine-window-shapley-out", out, "--fine-window-scale", "-1"]):
        with pytest.raises(SystemExit) as e:
            predict.main(["-m", meta, "-d", npy, "-o", str(tmp_path / "q.csv")] + bad)
        assert e.value.code == 2, bad
