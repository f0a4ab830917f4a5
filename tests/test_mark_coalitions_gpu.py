"""Histone-mark coalitions on the GPU (cf_mark_coalitions / cf_mark_shapley / cf_mark_epistasis, the ChromoformerBase methods of the
same names, attribution.mark_shapley, predict --mark-shapley-out / --mark-epistasis-out): row (b, m) is the inference forward of gene
b with the raw signal of every absent player's marks scaled by s over the player's regions.

  * the bits of a row: the full word is the plain forward; at s = 0 a row is the plain forward on the batch with the gone columns
    zeroed; at s = 2.5 one absent player is the whole-region window of the perturbation scan;
  * logits against the CPU oracle and the reference's golden, classifier and regressor;
  * phi against the float64 Shapley values of the call's own rows, the efficiency gap, null players exactly 0, epistasis symmetric
    with the leave-one-out effects on the diagonal;
  * the same bits whatever max_batch is, call after call, for the packed forms; other model shapes; the launch contract and every
    refusal by name; no side effects; the dataset generator and the CLI.

Three genes of the 20-gene synthetic dataset read at w_prom = 39000: a '-' strand gene whose promoter is stored mirrored, a '+' strand
gene with an 1,800-sample pCRE, a gene without partners.  With the seven marks as players the three genes are 384 rows: 96 chunks at
max_batch = 4; at max_batch = 7 the chunks straddle the genes."""
import ctypes as C
import os

import numpy as np
import pandas as pd
import pytest
import torch

from chromoformer_amd import _lib
from chromoformer_amd.attribution import coalition_table, mark_players
from oracle import chromoformer_oracle as orc
from tests import mark_oracle as mo
from tests import scan_oracle as so
from tests.coalition_oracle import epistasis_fp32, shapley_fp64
from tests.helpers import GOLDEN
from tests.test_input_grads_gpu import _model
from tests.test_pcre_coalitions_gpu import U, _gamma

pytestmark = pytest.mark.gpu
BINS = (2000, 500, 100)
GENES = ["ENSGSYN00001", "ENSGSYN00000", "ENSGSYN00002"]
ALL = tuple(range(7))
TOL = 1e-4      # the project's logit bound
OVERLAP = [((0, 1), (0, 1)), ((1, 2), (0, 2))]
UNION = [((0, 1, 2), (0,)), ((0, 1), (1,)), ((1, 2), (2,))]      # gone(rho) of OVERLAP's empty word, one player per region


def _args(batch):
    return tuple(batch[k] for k in so.KEYS)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """-> (dataset, the three genes' batch, their promoter flips): built once, shared, never written."""
    ds = so.scan_dataset(str(tmp_path_factory.mktemp("marks")), w_prom=39000)
    return ds, so.dataset_batch(ds, GENES), [ds.genes[g]["tss"][2] != "+" for g in GENES]


@pytest.fixture(scope="module")
def small():
    """The seed-42 classifier (the golden's weights) at max_batch = 4."""
    return _model(None, False, orc.init_params(None, 42, False), 4)


@pytest.fixture(scope="module")
def marks128(data, small):
    """(phi, info) of small.mark_shapley on the three genes, the seven marks as players, s = 0: computed once, never written."""
    phi, info = small.mark_shapley(*_args(data[1]), return_coalitions=True)
    torch.cuda.synchronize()
    return phi.cpu(), {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in info.items()}


def _zeroed(batch, gone):
    """The batch with the columns of the marks of gone[rho] zeroed in region rho (x * 0 per column, every row, every resolution)."""
    out = dict(batch)
    out["promoter_feats"], out["pcre_feats"] = {}, {}
    F = next(iter(batch["promoter_feats"].values())).shape[-1]
    for b, t in batch["promoter_feats"].items():
        out["promoter_feats"][b] = t * torch.tensor([0.0 if gone[0] >> f & 1 else 1.0 for f in range(F)], device=t.device)
    for b, t in batch["pcre_feats"].items():
        S = t.shape[1]
        keep = torch.tensor([[0.0 if gone[1 + j] >> f & 1 else 1.0 for f in range(F)] for j in range(S)], device=t.device)
        out["pcre_feats"][b] = t * keep[None, :, None, :]
    return out


def _plain(model, batch):
    with torch.no_grad():
        return model(*_args(batch)).cpu()


def test_the_full_word_and_zeroed_columns_bit_for_bit(data, small, marks128):
    ds, batch, flips = data
    base = _plain(small, batch)
    rows = marks128[1]["coalitions"]
    assert rows.shape == (3, 128, 2) and torch.equal(rows[:, 127], base) and torch.equal(marks128[1]["logits"], base)
    cases = [("marks", [0x7F, 0x00, 0x7F & ~(1 << 3), 0x25, 0x40, 0x3F]),
             ("compartments", [0x3FFF, 0x0000, 0x3FFF & ~(1 << 1) & ~(1 << 11) & ~(1 << 12), 0x007F, 0x3F80, 0x1555]),
             ("regions", [0x1FF & ~1, 0x001, 0x1FF & ~(1 << 1), 0x0AA]),
             (OVERLAP, [0b00, 0b01, 0b10, 0b11])]
    for spec, words in cases:
        marks, regions, _ = mark_players(spec, 7, 8)
        got = small.mark_coalitions(*_args(batch), keep=words, players=spec).cpu()
        assert got.shape == (3, len(words), 2) and not got.requires_grad
        for c, m in enumerate(words):
            ref = _plain(small, _zeroed(batch, mo.gone_words(marks, regions, m, 9)))
            assert torch.equal(got[:, c], ref), (spec, hex(m))
        if spec == "marks":
            assert torch.equal(got, rows[:, words])
            assert not torch.equal(got[:, 1], base)
    # the overlapping pair with nobody present is the union player: mark 1 of the promoter is scaled once
    for s in (0.0, 2.5):
        a = small.mark_coalitions(*_args(batch), keep=[0], players=OVERLAP, scale=s).cpu()
        b = small.mark_coalitions(*_args(batch), keep=[0], players=UNION, scale=s).cpu()
        assert torch.equal(a, b), s


def test_one_absent_player_is_the_whole_region_scan_window(data, small):
    ds, batch, flips = data
    for region, marks, fl in ((0, (1, 4), flips), (0, ALL, flips), (1, (2, 5), None), (1, ALL, None)):
        got = small.mark_coalitions(*_args(batch), keep=[0, 1], players=[(marks, (region,))], scale=2.5).cpu()
        scan = small.perturbation_scan(*_args(batch), region=region, width=20, mark_sets=[marks], scale=2.5, flip=fl).cpu()
        assert torch.equal(got[:, 0], scan[:, 1]) and torch.equal(got[:, 1], scan[:, 0]), (region, marks)
        assert not torch.equal(got[:2, 0], got[:2, 1])


@pytest.mark.parametrize("regression", [False, True], ids=["classifier", "regressor"])
def test_logits_against_the_oracle_and_the_golden(data, regression):
    ds, batch, flips = data
    P = orc.init_params(None, 42, regression)
    model = _model(None, regression, P, 4)
    g = np.load(os.path.join(GOLDEN, "mark_coalitions.npz"))
    head = "reg" if regression else "clf"
    assert [str(x) for x in g["genes"]] == GENES and int(g["w_prom"]) == 39000
    for k in range(len(g["words"])):
        n, word, scale = int(g["n_players"][k]), int(g["words"][k]), float(g["scales"][k])
        pm, pr = g["player_marks"][k][:n], g["player_regions"][k][:n]
        spec = [([f for f in range(7) if pm[p] >> f & 1], [r for r in range(9) if pr[p] >> r & 1]) for p in range(n)]
        words = [word, (1 << n) - 1, (1 << n) - 2]
        got = model.mark_coalitions(*_args(batch), keep=words, players=spec, scale=scale).cpu()
        assert got.shape == (3, 3, 1 if regression else 2)
        d_gold = max((got[:, 0] - torch.from_numpy(g[head][k])).abs().max().item(), (got[:, 1] - torch.from_numpy(g["base." + head])).abs().max().item())
        d_ora = (got - mo.oracle_mark_coalitions(P, batch, (pm, pr), words, scale)).abs().max().item()
        print("case", k, "vs golden %.2e, vs oracle %.2e" % (d_gold, d_ora))
        assert d_gold < TOL and d_ora < TOL, (k, d_gold, d_ora)


def _check_phi(phi, info, P):
    """phi against shapley_fp64 of the returned coalition logits, elementwise within the fp32 rounding bound of k_shapley (any summation
    order; tests/test_pcre_coalitions_gpu.py); info["delta"] within P times that bound plus 4 u max|v|."""
    v = info["coalitions"].cpu().numpy()
    phi64, scale = shapley_fp64(v)
    bound = _gamma(P) * scale
    err = np.abs(phi.cpu().numpy().astype(np.float64) - phi64)
    print("phi: max err %.3e, max bound %.3e" % (err.max(), bound.max()))
    assert (err <= bound).all(), (err.max(), bound.max())
    dbound = P * bound.max(1) + 4 * U * np.abs(v).max(1)
    delta = np.abs(info["delta"].cpu().numpy())
    print("delta: max %.3e, max bound %.3e" % (delta.max(), dbound.max()))
    assert delta.shape == dbound.shape and (delta <= dbound).all(), (delta.max(), dbound.max())
    assert torch.equal(info["logits"], info["coalitions"][:, -1]) and torch.equal(info["erased"], info["coalitions"][:, 0])


def test_shapley_values_null_players_and_epistasis(data, small, marks128):
    ds, batch, flips = data
    phi, info = marks128
    assert phi.shape == (3, 7, 2) and info["players"] == ["mark%d" % f for f in range(7)] and not phi.requires_grad
    _check_phi(phi, info, 7)
    assert bool((phi != 0).any(-1).all())
    # a player that covers only a dummy slot: every slot of the third gene, which has no partners
    spec = [(ALL, (0,)), (ALL, (1,)), (ALL, (8,))]
    p3, i3 = small.mark_shapley(*_args(batch), players=spec, return_coalitions=True)
    _check_phi(p3, i3, 3)
    p3 = p3.cpu()
    assert bool((p3[2, 1:] == 0).all()) and bool((p3[:, 0] != 0).all()) and bool((p3[:2] != 0).all())
    # the gene without partners: every distal player of "compartments" is exactly 0 (16,384 rows)
    wide = _model(None, False, orc.init_params(None, 42, False), 64)
    lone = {k: ({b: t[2:3] for b, t in v.items()} if isinstance(v, dict) else v[2:3]) for k, v in batch.items()}
    pc, ic = wide.mark_shapley(*_args(lone), players="compartments")
    pc = pc.cpu()
    assert pc.shape == (1, 14, 2) and bool((pc[0, 7:] == 0).all()) and bool((pc[0, :7] != 0).all())
    assert ic["players"][7] == "mark0@pcres"
    # epistasis: its definition on the pair rows, exactly symmetric, the leave-one-out effects on the diagonal
    eps, ie = small.mark_epistasis(*_args(batch))
    eps = eps.cpu()
    assert eps.shape == (3, 7, 7, 2) and torch.equal(eps, eps.transpose(1, 2))
    pairs = coalition_table("pairs", 7)
    rows = info["coalitions"][:, pairs.astype(np.int64)]
    assert torch.equal(eps, torch.from_numpy(epistasis_fp32(rows.numpy())))
    assert torch.equal(ie["logits"].cpu(), rows[:, 0]) and torch.equal(ie["single"].cpu(), rows[:, 1:8])
    for i in range(7):
        assert torch.equal(eps[:, i, i], ie["logits"].cpu() - ie["single"].cpu()[:, i]), i
    assert bool((eps != 0).any())


def test_same_bits_for_every_max_batch_call_after_call_and_packed_forms(data, small, marks128):
    from chromoformer_amd.engine import Slot
    ds, batch, flips = data
    P = orc.init_params(None, 42, False)
    phi, info = marks128
    again, info2 = small.mark_shapley(*_args(batch), return_coalitions=True)
    assert torch.equal(again.cpu(), phi) and torch.equal(info2["coalitions"].cpu(), info["coalitions"])
    eps = small.mark_epistasis(*_args(batch), scale=2.5)[0].cpu()
    words = [0x7F, 0x12, 0x00]
    lg = small.mark_coalitions(*_args(batch), keep=words, players="compartments", scale=0.5).cpu()
    for cap in (7, 64):
        model = _model(None, False, P, cap)
        p, i = model.mark_shapley(*_args(batch), return_coalitions=True)
        assert torch.equal(p.cpu(), phi) and torch.equal(i["coalitions"].cpu(), info["coalitions"]), cap
        assert torch.equal(model.mark_epistasis(*_args(batch), scale=2.5)[0].cpu(), eps), cap
        assert torch.equal(model.mark_coalitions(*_args(batch), keep=words, players="compartments", scale=0.5).cpu(), lg), cap
    packed = small.pack_batch(batch)
    slot = Slot(small, 3).fill(small, batch)
    for p in (packed, slot):
        assert torch.equal(small.mark_shapley(p)[0].cpu(), phi)
        assert torch.equal(small.mark_epistasis(p, scale=2.5)[0].cpu(), eps)
        assert torch.equal(small.mark_coalitions(p, keep=words, players="compartments", scale=0.5).cpu(), lg)
    bits = torch.tensor([[bool(m >> p & 1) for p in range(14)] for m in words])
    assert torch.equal(small.mark_coalitions(packed, keep=bits, players="compartments", scale=0.5).cpu(), lg)


REG_4x128 = dict(n_layers=6, n_heads=4, d_model=128, d_ff=256)
SHAPES = {
    "i_max16": (dict(i_max=16), False),
    "d_emb_64": (dict(d_emb=64, embed=dict(n_layers=1, n_heads=2, d_model=64, d_ff=128),
                      pairwise_interaction=dict(n_layers=2, n_heads=2, d_model=64, d_ff=256), regulation=REG_4x128), False),
    "embed_2_layers": (dict(embed=dict(n_layers=2, n_heads=2, d_model=128, d_ff=128)), False),
    "reg_layer_by_layer": (dict(regulation=REG_4x128), False),
    "regressor": (None, True),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_other_shapes_are_the_plain_forward_bit_for_bit(name):
    """All 128 coalitions of the seven marks on two genes (256 rows in chunks of 5) against the plain forward on the zeroed columns."""
    over, regression = SHAPES[name]
    cfg = orc._cfg(over)
    batch = orc.synthetic_batch(2, cfg=cfg, seed=13, regime="realistic")
    if name == "embed_2_layers":      # the reference's full [B, 1, L, L] promoter mask: the chunk rows carry all L rows
        assert all(m.numel() == 2 * L * L for m, L in zip(batch["promoter_pad_masks"].values(), (20, 80, 400)))
    dev = {k: ({b: t.cuda() for b, t in v.items()} if isinstance(v, dict) else v.cuda()) for k, v in batch.items()}
    model = _model(cfg, regression, orc.init_params(cfg, 3, regression), 5)
    T = cfg["i_max"] + 1
    marks, regions, _ = mark_players("marks", 7, cfg["i_max"])
    phi, info = model.mark_shapley(*_args(dev), return_coalitions=True)
    rows = info["coalitions"].cpu()
    assert rows.shape == (2, 128, 1 if regression else 2)
    for m in range(128):
        ref = _plain(model, _zeroed(dev, mo.gone_words(marks, regions, m, T)))
        assert torch.equal(rows[:, m], ref), (name, hex(m))
    _check_phi(phi, info, 7)


@pytest.mark.parametrize("cap,n_coal", [(64, 20), (7, 5), (4, 128)])
def test_launch_contract(data, cap, n_coal):
    """fwd = ceil(B n_coal / max_batch) (1 + n_fwd), n_fwd those of cf_forward(save = 0); Shapley and epistasis add their reducer."""
    ds, batch, flips = data
    model = _model(None, False, orc.init_params(None, 42, False), cap)
    _plain(model, batch)
    n_fwd = model.launch_counts()[0]
    chunks = lambda rows: -(-rows // cap)      # noqa: E731
    if n_coal < 128:
        model.mark_coalitions(*_args(batch), keep=list(range(n_coal)))
        assert model.launch_counts()[0] == chunks(3 * n_coal) * (1 + n_fwd)
    else:
        model.mark_shapley(*_args(batch))
        assert model.launch_counts()[0] == chunks(3 * 128) * (1 + n_fwd) + 1 == 96 * (1 + n_fwd) + 1
    model.mark_epistasis(*_args(batch))
    assert model.launch_counts()[0] == chunks(3 * 29) * (1 + n_fwd) + 1
    model.mark_shapley(*_args(batch), players=OVERLAP)
    assert model.launch_counts()[0] == chunks(3 * 4) * (1 + n_fwd) + 1


def test_refusals_by_name_with_nothing_launched(data):
    ds, batch, flips = data
    L = _lib.lib()
    model = _model(None, False, orc.init_params(None, 42, False), 4)
    bs, keep_alive = model.pack_batch(batch)
    _plain(model, batch)
    f0 = model.launch_counts()
    st = torch.cuda.current_stream().cuda_stream
    out = torch.full((3, 128, 2), float("nan"), device="cuda")
    pm, pr, _ = mark_players("marks", 7, 8)
    words = np.arange(4, dtype=np.uint32)
    big = _lib.cf_batch.from_buffer_copy(bs)
    big.B = 5

    def opts(n_players=7, marks=pm, regions=pr, scale=0.0):
        o = _lib.cf_mark_opts()
        o.n_players, o.scale = n_players, scale
        o.player_marks = marks.ctypes.data if marks is not None else None
        o.player_regions = regions.ctypes.data if regions is not None else None
        return o

    def edited(a, p, v):
        a = a.copy()
        a[p] = v
        return a

    bad_opts = [(dict(n_players=0), b"n_players"), (dict(n_players=17), b"n_players"), (dict(marks=None), b"null player_marks"),
                (dict(regions=None), b"null player_marks / player_regions"), (dict(marks=edited(pm, 2, 0)), b"player_marks[2] = 0"),
                (dict(regions=edited(pr, 5, 0)), b"player_regions[5] = 0"), (dict(marks=edited(pm, 1, 0x80)), b"n_feats"),
                (dict(regions=edited(pr, 6, 0x200)), b"i_max"), (dict(scale=-0.5), b"scale"), (dict(scale=float("inf")), b"scale"),
                (dict(scale=float("nan")), b"scale")]
    entries = [(b"cf_mark_coalitions", lambda h, b, o, dst: L.cf_mark_coalitions(h, b, o, words.ctypes.data, 4, dst, st)),
               (b"cf_mark_shapley", lambda h, b, o, dst: L.cf_mark_shapley(h, b, o, dst, None, st)),
               (b"cf_mark_epistasis", lambda h, b, o, dst: L.cf_mark_epistasis(h, b, o, dst, None, st))]

    def refused(rc, *needles):
        err = L.cf_last_error()
        assert rc != 0 and all(n in err for n in needles), err

    for name, fn in entries:
        good = opts()
        refused(fn(None, C.byref(bs), C.byref(good), out.data_ptr()), name, b"null handle")
        refused(fn(model._handle, None, C.byref(good), out.data_ptr()), name, b"null batch")
        refused(fn(model._handle, C.byref(bs), None, out.data_ptr()), name, b"null opts")
        refused(fn(model._handle, C.byref(bs), C.byref(good), None), name, b"null")
        refused(fn(model._handle, C.byref(big), C.byref(good), out.data_ptr()), name, b"max_batch")
        for kw, msg in bad_opts:
            refused(fn(model._handle, C.byref(bs), C.byref(opts(**kw)), out.data_ptr()), name, msg)
    good = opts()
    name = b"cf_mark_coalitions"
    refused(L.cf_mark_coalitions(model._handle, C.byref(bs), C.byref(good), None, 4, out.data_ptr(), st), name, b"null keep")
    refused(L.cf_mark_coalitions(model._handle, C.byref(bs), C.byref(good), words.ctypes.data, 0, out.data_ptr(), st), name, b"n_coal")
    bad = edited(words, 3, 0x80)
    refused(L.cf_mark_coalitions(model._handle, C.byref(bs), C.byref(good), bad.ctypes.data, 4, out.data_ptr(), st), name, b"keep[3]", b"n_players")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and model.launch_counts() == f0      # nothing was launched
    # armed riders (a training step in flight): refused; the handle is not used again
    assert L.cf_rider_arm(model._handle, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, 0, 8) == 0, L.cf_last_error()
    for name, fn in entries:
        refused(fn(model._handle, C.byref(bs), C.byref(good), out.data_ptr()), name, b"riders")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    for kw in (dict(players="genes"), dict(players=[((7,), (0,))]), dict(keep=[128])):      # (raised before the library is called)
        with pytest.raises(ValueError, match="mark_players|mark_coalitions"):
            model.mark_coalitions((bs, keep_alive), **dict(dict(keep=[0]), **kw))
    with pytest.raises(ValueError, match="keep is required"):
        model.mark_coalitions((bs, keep_alive))
    del keep_alive


def test_a_pending_backward_is_refused_and_the_order_of_calls_does_not_matter():
    batches = [orc.synthetic_batch(4, seed=41 + i, regime="realistic") for i in range(2)]
    P = orc.init_params(None, 42, False)
    model = _model(None, False, P, 8)
    b = batches[0]
    with torch.enable_grad():
        for method, kw in (("mark_shapley", {}), ("mark_epistasis", {}), ("mark_coalitions", dict(keep=[127, 0]))):
            out = model(*_args(b))
            res = getattr(model, method)(*_args(batches[1]), **kw)
            assert not (res if torch.is_tensor(res) else res[0]).requires_grad
            with pytest.raises(RuntimeError, match=method):
                out[:, 1].sum().backward()
        model(*_args(b))[:, 1].sum().backward()      # a fresh forward trains as before
    assert float(model._gflat.abs().sum()) > 0
    # the C ABI itself refuses a backward without a new saving forward
    bs, keep = model.pack_batch(b)
    st = torch.cuda.current_stream().cuda_stream
    lgt = torch.empty(4, 2, device="cuda")
    _lib.check(_lib.lib().cf_forward(model._handle, C.byref(bs), lgt.data_ptr(), 1, st), "cf_forward")
    model.mark_coalitions((bs, keep), keep=[5])
    dl = torch.zeros(4, 2, device="cuda")
    assert _lib.lib().cf_backward_from(model._handle, C.byref(bs), dl.data_ptr(), st) != 0
    assert b"must follow cf_forward" in _lib.lib().cf_last_error()

    def others(m):
        ig = m.integrated_gradients(*_args(b), n_steps=3)
        return [m.pcre_shapley(*_args(b))[0].cpu(), ig[0]["interaction_freq"].cpu(), ig[1]["delta"].cpu(),
                m.perturbation_scan_regions(*_args(b), regions=[0, 2], mark_sets=[ALL, (3,)])[0].cpu()]

    def mine(m):
        return [m.mark_shapley(*_args(b), scale=0.5)[0].cpu(), m.mark_epistasis(*_args(b), players="regions")[0].cpu(),
                m.mark_coalitions(*_args(b), keep=[0, 9, 127]).cpu()]

    fresh = _model(None, False, P, 8)
    ref_mine, ref_others = mine(fresh), others(_model(None, False, P, 8))
    mixed = _model(None, False, P, 8)
    a = mixed.pcre_shapley(*_args(b))[0].cpu()
    s = mixed.mark_shapley(*_args(b), scale=0.5)[0].cpu()
    ig = mixed.integrated_gradients(*_args(b), n_steps=3)
    e = mixed.mark_epistasis(*_args(b), players="regions")[0].cpu()
    sc = mixed.perturbation_scan_regions(*_args(b), regions=[0, 2], mark_sets=[ALL, (3,)])[0].cpu()
    c = mixed.mark_coalitions(*_args(b), keep=[0, 9, 127]).cpu()
    assert all(torch.equal(x, y) for x, y in zip([s, e, c], ref_mine))
    assert all(torch.equal(x, y) for x, y in zip([a, ig[0]["interaction_freq"].cpu(), ig[1]["delta"].cpu(), sc], ref_others))
    assert all(torch.equal(x, y) for x, y in zip(others(fresh), ref_others))      # ... and after the mark calls alone


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
            model.mark_shapley(*_args(batches[2]), scale=2.0)
            model.mark_epistasis(*_args(batches[2]), players="compartments")
            model.mark_coalitions(*_args(batches[2]), keep=[0, 1], players=OVERLAP)
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


def test_dataset_generator_and_cli(tmp_path):
    from chromoformer_amd import ChromoformerClassifier, pack, predict
    from chromoformer_amd.data import ChromoformerDataset, GeneStore
    from tests.synth_data import make_dataset
    npy = str(tmp_path / "npy")
    meta = make_dataset(npy, n_genes=20, seed=11)
    table = pd.read_csv(meta)
    genes = table.gene_id.tolist()
    P = orc.init_params(seed=7)
    ck = str(tmp_path / "w.pt")
    torch.save({"net": P}, ck)
    out, eout = str(tmp_path / "marks.npz"), str(tmp_path / "eps.npy")
    assert predict.main(["-m", meta, "-d", npy, "-w", ck, "-o", str(tmp_path / "p.csv"), "--mark-shapley-out", out, "--mark-epistasis-out", eout,
                         "--mark-players", "regions", "--mark-scale", "0.5"]) == 0
    z = np.load(out)
    assert sorted(z.files) == ["erased", "gene_ids", "logits", "phi", "players"]
    assert list(z["gene_ids"]) == genes and list(z["players"]) == ["promoter"] + ["pcre%d" % j for j in range(8)]
    assert z["phi"].shape == (20, 9) and z["phi"].dtype == np.float32 and z["logits"].shape == z["erased"].shape == (20,)
    eps = np.load(eout)
    assert eps.shape == (20, 9, 9) and eps.dtype == np.float32 and np.array_equal(eps, eps.transpose(0, 2, 1))
    # the per-batch calls on the store predict() builds: the same bits
    ds = ChromoformerDataset(meta, npy, genes)
    model = ChromoformerClassifier(seed=123, max_batch=32).cuda(0)
    model.load_state_dict(P)
    store = GeneStore(ds, device=model._device, resident=True)
    d = store.batch(list(range(20)))
    phi, info = model.mark_shapley(*_args(d), players="regions", scale=0.5)
    assert np.array_equal(z["phi"], phi.cpu()[..., 1].numpy()) and np.array_equal(z["logits"], info["logits"].cpu()[:, 1].numpy())
    assert np.array_equal(z["erased"], info["erased"].cpu()[:, 1].numpy())
    assert np.array_equal(eps, model.mark_epistasis(*_args(d), players="regions", scale=0.5)[0].cpu()[..., 1].numpy())
    sig = torch.sigmoid(torch.from_numpy(z["logits"])).numpy()
    assert np.abs(sig - pd.read_csv(str(tmp_path / "p.csv"))["prediction"].to_numpy()).max() <= 2.0 ** -23
    n_pcres = np.array([min(len(ds.genes[g]["pcres"]), 8) for g in genes])
    for i in range(20):      # a dummy slot's player is a null player
        assert (z["phi"][i, 1 + n_pcres[i]:] == 0).all() and (z["phi"][i, :1 + n_pcres[i]] != 0).all(), i
    # the generator, in chunks of 7 genes from the raw files, then from a packed store: the per-batch calls' bits
    sub = genes[3:13]
    for packed in (False, True):
        st = None
        if packed:
            path = str(tmp_path / "genes.cfstore")
            pack.pack(meta, npy, path)
            st = pack.PackedStore(path).store(sub, device=model._device, regression=False)
        res = list(model.mark_shapley_dataset(ds, genes=sub, epistasis=True, bsz=7, store=st))
        assert [r["gene_id"] for r in res] == sub
        src = st if packed else GeneStore(_subset(ds, sub), device=model._device, resident=True)
        for lo in (0, 7):
            n = min(7, 10 - lo)
            dd = src.batch(list(range(lo, lo + n)))
            phi, info = model.mark_shapley(*_args(dd))
            e = model.mark_epistasis(*_args(dd))[0].cpu().numpy()
            for i in range(n):
                r = res[lo + i]
                assert sorted(r) == ["eps", "erased", "gene_id", "logits", "phi", "players"] and r["players"] == ["mark%d" % f for f in range(7)]
                assert r["phi"].shape == (7, 2) and r["phi"].dtype == np.float32 and r["eps"].shape == (7, 7, 2)
                assert np.array_equal(r["phi"], phi[i].cpu().numpy()) and np.array_equal(r["eps"], e[i])
                assert np.array_equal(r["logits"], info["logits"][i].cpu().numpy()) and np.array_equal(r["erased"], info["erased"][i].cpu().numpy())
    with pytest.raises(ValueError, match="mark_players"):
        next(model.mark_shapley_dataset(ds, genes=sub, players="genes"))


def _subset(ds, genes):
    import copy
    sub = copy.copy(ds)
    sub.target_genes = list(genes)
    return sub
