"""Histone-mark coalitions against a donor cell type on the GPU (cf_mark_donor_coalitions / cf_mark_donor_shapley /
cf_mark_donor_epistasis, the ChromoformerBase methods of those names, attribution.mark_donor_shapley, predict
--mark-donor-shapley-out / --mark-donor-epistasis-out): row (b, m) is the inference forward of gene b with every absent player's marks
taken, bit for bit, from the same gene's features in another cell type, over the player's regions.

  * the bits of a row: with the batch as its own donor every row is the plain forward and phi is exactly 0; with a donor of zeros a
    row is mark_coalitions(scale = 0); with the donor dataset's batch a row is the plain forward on rows built with torch.where;
  * logits against the CPU oracle and the reference's golden, classifier and regressor;
  * phi against the float64 Shapley values of the call's own rows, the efficiency gap, null players exactly 0, epistasis symmetric
    with the leave-one-out effects on the diagonal;
  * the same bits whatever max_batch is, call after call, for the packed forms of batch and donor; other model shapes, one of them
    with n_bins * n_feats no multiple of 4 (the scalar path and the float4 that straddles two regions); the launch contract and
    every refusal by name; the shared workspace; no side effects; the dataset generator and the CLI.

The three genes of tests/test_mark_coalitions_gpu.py and a second synthetic cell type over the same regions
(tests.donor_oracle.donor_dataset)."""
import ctypes as C
import os

import numpy as np
import pandas as pd
import pytest
import torch

from chromoformer_amd import _lib
from chromoformer_amd.attribution import coalition_table, mark_players
from oracle import chromoformer_oracle as orc
from tests import donor_oracle as do
from tests import mark_oracle as mo
from tests import scan_oracle as so
from tests.coalition_oracle import epistasis_fp32, shapley_fp64
from tests.helpers import GOLDEN
from tests.test_input_grads_gpu import _model
from tests.test_mark_coalitions_gpu import GENES, OVERLAP, SHAPES, UNION
from tests.test_pcre_coalitions_gpu import U, _gamma

pytestmark = pytest.mark.gpu
ALL = tuple(range(7))
TOL = 1e-4      # the project's logit bound
SHAPES = dict(SHAPES, odd_lengths=(dict(binsizes=[4000, 800, 160], w_max=40000), False))      # L F = 70 / 350 / 1750: no multiple of 4
CASES = [("marks", [0x7F, 0x00, 0x7F & ~(1 << 3), 0x25, 0x40, 0x3F]),
         ("compartments", [0x3FFF, 0x0000, 0x3FFF & ~(1 << 1) & ~(1 << 11) & ~(1 << 12), 0x007F, 0x3F80, 0x1555]),
         ("regions", [0x1FF & ~1, 0x001, 0x1FF & ~(1 << 1), 0x0AA]),
         (OVERLAP, [0b00, 0b01, 0b10, 0b11])]


def _args(batch):
    return tuple(batch[k] for k in so.KEYS)


def _dev(batch):
    return {k: ({b: t.cuda() for b, t in v.items()} if isinstance(v, dict) else v.cuda()) for k, v in batch.items() if k in so.KEYS}


def _feats(batch):
    """The donor argument from a device batch dict."""
    return batch["promoter_feats"], batch["pcre_feats"]


def _plain(model, batch):
    with torch.no_grad():
        return model(*_args(batch)).cpu()


def _selected(batch, donor, gone):
    """The device batch with the elements of the marks of gone[rho] in region rho taken from `donor` (torch.where per column)."""
    out = dict(batch)
    out["promoter_feats"], out["pcre_feats"] = {}, {}
    F = next(iter(batch["promoter_feats"].values())).shape[-1]
    for b, t in batch["promoter_feats"].items():
        take = torch.tensor([bool(gone[0] >> f & 1) for f in range(F)], device=t.device)
        out["promoter_feats"][b] = torch.where(take, donor["promoter_feats"][b].reshape(t.shape), t)
    for b, t in batch["pcre_feats"].items():
        take = torch.tensor([[bool(gone[1 + j] >> f & 1) for f in range(F)] for j in range(t.shape[1])], device=t.device)
        out["pcre_feats"][b] = torch.where(take[None, :, None, :], donor["pcre_feats"][b].reshape(t.shape), t)
    return out


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """-> (the three genes' batch, the donor cell type's batch, both on the device, and their host copies): built once, never written."""
    ds = so.scan_dataset(str(tmp_path_factory.mktemp("marks")), w_prom=39000)
    dn = do.donor_dataset(ds.npy_dir, str(tmp_path_factory.mktemp("donor")), do.DONOR_SEED, w_prom=39000)
    host, dhost = so.dataset_batch(ds, GENES), so.dataset_batch(dn, GENES)
    return _dev(host), _dev(dhost), host, dhost


@pytest.fixture(scope="module")
def small():
    """The seed-42 classifier (the golden's weights) at max_batch = 4."""
    return _model(None, False, orc.init_params(None, 42, False), 4)


@pytest.fixture(scope="module")
def donor128(data, small):
    """(phi, info) of small.mark_donor_shapley on the three genes against the donor, the seven marks as players: once, never written."""
    phi, info = small.mark_donor_shapley(*_args(data[0]), donor=_feats(data[1]), return_coalitions=True)
    torch.cuda.synchronize()
    return phi.cpu(), {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in info.items()}


def test_the_batch_as_its_own_donor_is_the_plain_forward_and_phi_is_zero(data, small):
    batch = data[0]
    base = _plain(small, batch)
    phi, info = small.mark_donor_shapley(*_args(batch), donor=_feats(batch), return_coalitions=True)
    rows = info["coalitions"].cpu()
    assert rows.shape == (3, 128, 2) and torch.equal(rows, base[:, None].expand(3, 128, 2))
    assert phi.shape == (3, 7, 2) and bool((phi == 0).all()) and bool((info["delta"] == 0).all())
    packed = small.pack_batch(batch)      # the donor's pointers ARE the batch's
    phi, info = small.mark_donor_shapley(packed, donor=packed, players="regions", return_coalitions=True)
    assert torch.equal(info["coalitions"].cpu(), base[:, None].expand(3, 512, 2)) and bool((phi == 0).all())
    eps = small.mark_donor_epistasis(packed, donor=packed)[0]
    assert eps.shape == (3, 7, 7, 2) and bool((eps == 0).all())


def test_a_donor_of_zeros_is_the_erased_mark(data, small):
    """The fixture's features are non-negative and finite: log1p(0 expm1(u)) = +0, the bits of the zero donor."""
    batch = data[0]
    assert all(bool((t >= 0).all()) and bool(torch.isfinite(t).all()) for k in ("promoter_feats", "pcre_feats") for t in batch[k].values())
    zeros = tuple({b: torch.zeros_like(t) for b, t in batch[k].items()} for k in ("promoter_feats", "pcre_feats"))
    for spec, words in CASES:
        got = small.mark_donor_coalitions(*_args(batch), donor=zeros, keep=words, players=spec).cpu()
        ref = small.mark_coalitions(*_args(batch), keep=words, players=spec, scale=0.0).cpu()
        assert got.shape == (3, len(words), 2) and torch.equal(got, ref), spec
    phi, info = small.mark_donor_shapley(*_args(batch), donor=zeros)
    ref, rinfo = small.mark_shapley(*_args(batch))
    assert torch.equal(phi, ref) and torch.equal(info["donor"], rinfo["erased"]) and torch.equal(info["logits"], rinfo["logits"])
    assert torch.equal(small.mark_donor_epistasis(*_args(batch), donor=zeros)[0], small.mark_epistasis(*_args(batch))[0])


def test_rows_are_the_plain_forward_on_selected_features_bit_for_bit(data, small, donor128):
    batch, donor = data[0], data[1]
    base = _plain(small, batch)
    rows = donor128[1]["coalitions"]
    assert rows.shape == (3, 128, 2) and torch.equal(rows[:, 127], base) and torch.equal(donor128[1]["logits"], base)
    marks, regions, _ = mark_players("marks", 7, 8)
    for m in range(128):
        ref = _plain(small, _selected(batch, donor, mo.gone_words(marks, regions, m, 9)))
        assert torch.equal(rows[:, m], ref), hex(m)
    # word 0: the donor's features under the gene's masks and frequencies
    swapped = dict(batch, promoter_feats=donor["promoter_feats"], pcre_feats=donor["pcre_feats"])
    assert torch.equal(rows[:, 0], _plain(small, swapped)) and torch.equal(donor128[1]["donor"], rows[:, 0])
    assert not torch.equal(rows[:, 0], base)
    for spec, words in CASES[1:]:
        marks, regions, _ = mark_players(spec, 7, 8)
        got = small.mark_donor_coalitions(*_args(batch), donor=_feats(donor), keep=words, players=spec).cpu()
        assert got.shape == (3, len(words), 2) and not got.requires_grad
        for c, m in enumerate(words):
            ref = _plain(small, _selected(batch, donor, mo.gone_words(marks, regions, m, 9)))
            assert torch.equal(got[:, c], ref), (spec, hex(m))
    got = small.mark_donor_coalitions(*_args(batch), donor=_feats(donor), keep=CASES[0][1]).cpu()
    assert torch.equal(got, rows[:, CASES[0][1]])
    # the overlapping pair with nobody present is the union player: mark 1 of the promoter is taken once
    a = small.mark_donor_coalitions(*_args(batch), donor=_feats(donor), keep=[0], players=OVERLAP).cpu()
    b = small.mark_donor_coalitions(*_args(batch), donor=_feats(donor), keep=[0], players=UNION).cpu()
    assert torch.equal(a, b) and not torch.equal(a[:, 0], base)


def test_nan_payloads_negative_zero_and_inf_pass_through(data, small):
    """A select, not arithmetic: the row that takes odd bit patterns from the donor is the plain forward on exactly those bits."""
    batch, donor = data[0], data[1]
    odd = {k: {b: t.clone() for b, t in donor[k].items()} for k in ("promoter_feats", "pcre_feats")}
    bits = torch.tensor([0x7FC12345, -0x80000000, 0x7F800000, -0x00800000, 0x7F812345], dtype=torch.int32, device="cuda")
    odd["pcre_feats"][500].view(torch.int32).reshape(-1)[7:12] = bits
    odd["promoter_feats"][100].view(torch.int32).reshape(-1)[700:705] = bits
    got = small.mark_donor_coalitions(*_args(batch), donor=_feats(odd), keep=[0, 0x7F]).cpu()
    ref = _plain(small, dict(batch, promoter_feats=odd["promoter_feats"], pcre_feats=odd["pcre_feats"]))
    assert torch.equal(got[:, 0].view(torch.int32), ref.view(torch.int32)) and torch.equal(got[:, 1], _plain(small, batch))


@pytest.mark.parametrize("regression", [False, True], ids=["classifier", "regressor"])
def test_logits_against_the_oracle_and_the_golden(data, regression):
    batch, donor, host, dhost = data
    P = orc.init_params(None, 42, regression)
    model = _model(None, regression, P, 4)
    g = np.load(os.path.join(GOLDEN, "mark_donor.npz"))
    head = "reg" if regression else "clf"
    assert [str(x) for x in g["genes"]] == GENES and int(g["w_prom"]) == 39000 and int(g["donor_seed"]) == do.DONOR_SEED
    for k in range(len(g["words"])):
        n, word = int(g["n_players"][k]), int(g["words"][k])
        pm, pr = g["player_marks"][k][:n], g["player_regions"][k][:n]
        spec = [([f for f in range(7) if pm[p] >> f & 1], [r for r in range(9) if pr[p] >> r & 1]) for p in range(n)]
        words = [word, (1 << n) - 1, (1 << n) - 2]
        got = model.mark_donor_coalitions(*_args(batch), donor=_feats(donor), keep=words, players=spec).cpu()
        assert got.shape == (3, 3, 1 if regression else 2)
        d_gold = max((got[:, 0] - torch.from_numpy(g[head][k])).abs().max().item(), (got[:, 1] - torch.from_numpy(g["base." + head])).abs().max().item())
        d_ora = (got - do.oracle_donor_coalitions(P, host, dhost, (pm, pr), words)).abs().max().item()
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
    assert torch.equal(info["logits"].cpu(), info["coalitions"].cpu()[:, -1]) and torch.equal(info["donor"].cpu(), info["coalitions"].cpu()[:, 0])
    return dbound


def test_shapley_values_null_players_and_epistasis(data, small, donor128):
    batch, donor = data[0], data[1]
    phi, info = donor128
    assert phi.shape == (3, 7, 2) and info["players"] == ["mark%d" % f for f in range(7)] and not phi.requires_grad
    assert sorted(info) == ["coalitions", "delta", "donor", "logits", "players"]
    _check_phi(phi, info, 7)
    assert bool((phi != 0).any(-1).all())
    # a player that covers only a slot that is a dummy in both cell types: every slot of the third gene, which has no partners
    spec = [(ALL, (0,)), (ALL, (1,)), (ALL, (8,))]
    p3, i3 = small.mark_donor_shapley(*_args(batch), donor=_feats(donor), players=spec, return_coalitions=True)
    _check_phi(p3, i3, 3)
    p3 = p3.cpu()
    assert bool((p3[2, 1:] == 0).all()) and bool((p3[:, 0] != 0).all()) and bool((p3[:2, 1] != 0).all())
    pr, ir = small.mark_donor_shapley(*_args(batch), donor=_feats(donor), players="regions")
    assert ir["players"][:2] == ["promoter", "pcre0"] and bool((pr[2, 1:] == 0).all()) and bool((pr[2, 0] != 0).all())
    # epistasis: its definition on the pair rows, exactly symmetric, the leave-one-out effects on the diagonal
    eps, ie = small.mark_donor_epistasis(*_args(batch), donor=_feats(donor))
    eps = eps.cpu()
    assert eps.shape == (3, 7, 7, 2) and torch.equal(eps, eps.transpose(1, 2)) and sorted(ie) == ["logits", "players", "single"]
    pairs = coalition_table("pairs", 7)
    rows = info["coalitions"][:, pairs.astype(np.int64)]
    assert torch.equal(eps, torch.from_numpy(epistasis_fp32(rows.numpy())))
    assert torch.equal(ie["logits"].cpu(), rows[:, 0]) and torch.equal(ie["single"].cpu(), rows[:, 1:8])
    for i in range(7):
        assert torch.equal(eps[:, i, i], ie["logits"].cpu() - ie["single"].cpu()[:, i]), i
    off = eps[:, ~torch.eye(7, dtype=torch.bool)]
    assert bool((off != 0).any()) and bool((phi != 0).any())


def test_same_bits_for_every_max_batch_call_after_call_and_packed_forms(data, small, donor128):
    from chromoformer_amd.engine import Slot
    batch, donor = data[0], data[1]
    P = orc.init_params(None, 42, False)
    phi, info = donor128
    dn = _feats(donor)
    again, info2 = small.mark_donor_shapley(*_args(batch), donor=dn, return_coalitions=True)
    assert torch.equal(again.cpu(), phi) and torch.equal(info2["coalitions"].cpu(), info["coalitions"])
    eps = small.mark_donor_epistasis(*_args(batch), donor=dn, players="regions")[0].cpu()
    words = [0x3FFF, 0x12, 0x00]
    lg = small.mark_donor_coalitions(*_args(batch), donor=dn, keep=words, players="compartments").cpu()
    for cap in (7, 64):
        model = _model(None, False, P, cap)
        p, i = model.mark_donor_shapley(*_args(batch), donor=dn, return_coalitions=True)
        assert torch.equal(p.cpu(), phi) and torch.equal(i["coalitions"].cpu(), info["coalitions"]), cap
        assert torch.equal(model.mark_donor_epistasis(*_args(batch), donor=dn, players="regions")[0].cpu(), eps), cap
        assert torch.equal(model.mark_donor_coalitions(*_args(batch), donor=dn, keep=words, players="compartments").cpu(), lg), cap
    packed, dpacked = small.pack_batch(batch), small.pack_batch(donor)
    slot, dslot = Slot(small, 3).fill(small, batch), Slot(small, 3).fill(small, donor)
    lists = ([donor["promoter_feats"][b] for b in small.binsizes], [donor["pcre_feats"][b] for b in small.binsizes])
    for p, d in ((packed, dn), (slot, dn), (packed, dpacked), (slot, dslot), (packed, dpacked[0]), (packed, lists)):
        assert torch.equal(small.mark_donor_shapley(p, donor=d)[0].cpu(), phi)
        assert torch.equal(small.mark_donor_epistasis(p, donor=d, players="regions")[0].cpu(), eps)
        assert torch.equal(small.mark_donor_coalitions(p, donor=d, keep=words, players="compartments").cpu(), lg)
    bits = torch.tensor([[bool(m >> p & 1) for p in range(14)] for m in words])
    assert torch.equal(small.mark_donor_coalitions(packed, donor=dpacked, keep=bits, players="compartments").cpu(), lg)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_other_shapes_are_the_plain_forward_bit_for_bit(name):
    """All 128 coalitions of the seven marks on two genes (256 rows in chunks of 5) against the plain forward on the selected features."""
    over, regression = SHAPES[name]
    cfg = orc._cfg(over)
    batch = _dev(orc.synthetic_batch(2, cfg=cfg, seed=13, regime="realistic"))
    donor = _dev(orc.synthetic_batch(2, cfg=cfg, seed=14, regime="realistic"))
    if name == "embed_2_layers":      # the reference's full [B, 1, L, L] promoter mask: the chunk rows carry all L rows
        assert all(m.numel() == 2 * L * L for m, L in zip(batch["promoter_pad_masks"].values(), (20, 80, 400)))
    if name == "odd_lengths":         # the promoter segment takes the scalar path, a pCRE float4 straddles two regions
        assert all((L * 7) % 4 and (8 * L * 7) % 4 == 0 for L in (t.shape[-2] for t in batch["promoter_feats"].values()))
    model = _model(cfg, regression, orc.init_params(cfg, 3, regression), 5)
    T = cfg["i_max"] + 1
    marks, regions, _ = mark_players("marks", 7, cfg["i_max"])
    phi, info = model.mark_donor_shapley(*_args(batch), donor=_feats(donor), return_coalitions=True)
    rows = info["coalitions"].cpu()
    assert rows.shape == (2, 128, 1 if regression else 2)
    for m in range(128):
        ref = _plain(model, _selected(batch, donor, mo.gone_words(marks, regions, m, T)))
        assert torch.equal(rows[:, m], ref), (name, hex(m))
    assert not torch.equal(rows[:, 0], rows[:, 127])
    _check_phi(phi, info, 7)
    if name == "odd_lengths":         # one region at a time: a float4 that straddles regions rho and rho + 1 takes each lane's own word
        words = [0x1FF & ~(1 << r) for r in (0, 1, 4, 8)]
        got = model.mark_donor_coalitions(*_args(batch), donor=_feats(donor), keep=words, players="regions").cpu()
        marks, regions, _ = mark_players("regions", 7, 8)
        for c, m in enumerate(words):
            assert torch.equal(got[:, c], _plain(model, _selected(batch, donor, mo.gone_words(marks, regions, m, 9)))), hex(m)


@pytest.mark.parametrize("cap,n_coal", [(64, 20), (7, 5), (4, 128)])
def test_launch_contract(data, cap, n_coal):
    """fwd = ceil(B n_coal / max_batch) (1 + n_fwd), n_fwd those of cf_forward(save = 0); Shapley and epistasis add their reducer."""
    batch, dn = data[0], _feats(data[1])
    model = _model(None, False, orc.init_params(None, 42, False), cap)
    _plain(model, batch)
    n_fwd = model.launch_counts()[0]
    chunks = lambda rows: -(-rows // cap)      # noqa: E731
    if n_coal < 128:
        model.mark_donor_coalitions(*_args(batch), donor=dn, keep=list(range(n_coal)))
        assert model.launch_counts()[0] == chunks(3 * n_coal) * (1 + n_fwd)
    else:
        model.mark_donor_shapley(*_args(batch), donor=dn)
        assert model.launch_counts()[0] == chunks(3 * 128) * (1 + n_fwd) + 1 == 96 * (1 + n_fwd) + 1
    model.mark_donor_epistasis(*_args(batch), donor=dn)
    assert model.launch_counts()[0] == chunks(3 * 29) * (1 + n_fwd) + 1
    model.mark_donor_shapley(*_args(batch), donor=dn, players=OVERLAP)
    assert model.launch_counts()[0] == chunks(3 * 4) * (1 + n_fwd) + 1


def test_refusals_by_name_with_nothing_launched(data):
    batch, donor = data[0], data[1]
    L = _lib.lib()
    model = _model(None, False, orc.init_params(None, 42, False), 4)
    bs, keep_alive = model.pack_batch(batch)
    ds_, donor_alive = model.pack_batch(donor)
    _plain(model, batch)
    f0 = model.launch_counts()
    st = torch.cuda.current_stream().cuda_stream
    out = torch.full((3, 128, 2), float("nan"), device="cuda")
    pm, pr, _ = mark_players("marks", 7, 8)
    words = np.arange(4, dtype=np.uint32)
    big = _lib.cf_batch.from_buffer_copy(bs)
    big.B = 5

    def opts(n_players=7, marks=pm, regions=pr, null_p=None, null_c=None):
        o = _lib.cf_mark_donor_opts()
        o.n_players = n_players
        o.player_marks = marks.ctypes.data if marks is not None else None
        o.player_regions = regions.ctypes.data if regions is not None else None
        for r in range(3):
            o.donor_promoter_feats[r] = None if r == null_p else ds_.promoter_feats[r]
            o.donor_pcre_feats[r] = None if r == null_c else ds_.pcre_feats[r]
        return o

    def edited(a, p, v):
        a = a.copy()
        a[p] = v
        return a

    bad_opts = [(dict(n_players=0), b"n_players"), (dict(n_players=17), b"n_players"), (dict(marks=None), b"null player_marks"),
                (dict(regions=None), b"null player_marks / player_regions"), (dict(marks=edited(pm, 2, 0)), b"player_marks[2] = 0"),
                (dict(regions=edited(pr, 5, 0)), b"player_regions[5] = 0"), (dict(marks=edited(pm, 1, 0x80)), b"n_feats"),
                (dict(regions=edited(pr, 6, 0x200)), b"i_max"), (dict(null_p=0), b"null donor_promoter_feats / donor_pcre_feats[0]"),
                (dict(null_p=2), b"donor_pcre_feats[2]"), (dict(null_c=1), b"null donor_promoter_feats / donor_pcre_feats[1]")]
    entries = [(b"cf_mark_donor_coalitions", lambda h, b, o, dst: L.cf_mark_donor_coalitions(h, b, o, words.ctypes.data, 4, dst, st)),
               (b"cf_mark_donor_shapley", lambda h, b, o, dst: L.cf_mark_donor_shapley(h, b, o, dst, None, st)),
               (b"cf_mark_donor_epistasis", lambda h, b, o, dst: L.cf_mark_donor_epistasis(h, b, o, dst, None, st))]

    def refused(rc, *needles):
        err = L.cf_last_error()
        assert rc != 0 and all(n in err for n in needles), err

    for name, fn in entries:
        good = opts()
        refused(fn(None, C.byref(bs), C.byref(good), out.data_ptr()), name + b":", b"null handle")
        refused(fn(model._handle, None, C.byref(good), out.data_ptr()), name + b":", b"null batch")
        refused(fn(model._handle, C.byref(bs), None, out.data_ptr()), name + b":", b"null opts")
        refused(fn(model._handle, C.byref(bs), C.byref(good), None), name + b":", b"null")
        refused(fn(model._handle, C.byref(big), C.byref(good), out.data_ptr()), name + b":", b"max_batch")
        for kw, msg in bad_opts:
            refused(fn(model._handle, C.byref(bs), C.byref(opts(**kw)), out.data_ptr()), name + b":", msg)
    good = opts()
    name = b"cf_mark_donor_coalitions:"
    refused(L.cf_mark_donor_coalitions(model._handle, C.byref(bs), C.byref(good), None, 4, out.data_ptr(), st), name, b"null keep")
    refused(L.cf_mark_donor_coalitions(model._handle, C.byref(bs), C.byref(good), words.ctypes.data, 0, out.data_ptr(), st), name, b"n_coal")
    bad = edited(words, 3, 0x80)
    refused(L.cf_mark_donor_coalitions(model._handle, C.byref(bs), C.byref(good), bad.ctypes.data, 4, out.data_ptr(), st), name, b"keep[3]", b"n_players")
    # the Python layer: the donor is checked before the library is called, by the method's name
    pf, cf = _feats(donor)
    wide = torch.zeros(3, 1, 20, 14, device="cuda")
    bad_donors = [(None, "donor is required"), ((pf,), "donor must be"), (5, "donor must be"), (({2000: pf[2000]}, cf), "donor must be"),
                  (({**pf, 500: pf[500][:2]}, cf), r"donor promoter_feats\[500\] has shape"),
                  ((pf, {**cf, 100: cf[100][:, :7]}), r"donor pcre_feats\[100\] has shape"),
                  (({**pf, 2000: pf[2000].double()}, cf), r"donor promoter_feats\[2000\] is torch.float64"),
                  (({**pf, 2000: wide[..., ::2]}, cf), r"donor promoter_feats\[2000\] is not contiguous"),
                  ((pf, {**cf, 500: cf[500].cpu()}), r"donor pcre_feats\[500\] is on cpu"),
                  ((pf, {**cf, 500: cf[500].cpu().numpy()}), r"donor pcre_feats\[500\] is not a tensor"),
                  (model.pack_batch(_two(donor)), "the donor holds 2 genes")]
    for method, kw in (("mark_donor_coalitions", dict(keep=[0])), ("mark_donor_shapley", {}), ("mark_donor_epistasis", {})):
        for d, msg in bad_donors:
            with pytest.raises(ValueError, match=method + ": " + msg):
                getattr(model, method)((bs, keep_alive), donor=d, **kw)
    for kw in (dict(players="genes"), dict(players=[((7,), (0,))]), dict(keep=[128])):
        with pytest.raises(ValueError, match="mark_players|mark_donor_coalitions"):
            model.mark_donor_coalitions((bs, keep_alive), donor=(pf, cf), **dict(dict(keep=[0]), **kw))
    with pytest.raises(ValueError, match="mark_donor_coalitions: keep is required"):
        model.mark_donor_coalitions((bs, keep_alive), donor=(pf, cf))
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and model.launch_counts() == f0      # nothing was launched
    # armed riders (a training step in flight): refused; the handle is not used again
    assert L.cf_rider_arm(model._handle, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, 0, 8) == 0, L.cf_last_error()
    for name, fn in entries:
        refused(fn(model._handle, C.byref(bs), C.byref(good), out.data_ptr()), name, b"riders")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    del keep_alive, donor_alive


def _two(batch):
    return {k: ({b: t[:2] for b, t in v.items()} if isinstance(v, dict) else v[:2]) for k, v in batch.items()}


def test_a_pending_backward_is_refused_and_the_workspace_is_shared_in_any_order():
    batches = [_dev(orc.synthetic_batch(4, seed=41 + i, regime="realistic")) for i in range(2)]
    P = orc.init_params(None, 42, False)
    model = _model(None, False, P, 8)
    b, dn = batches[0], _feats(batches[1])
    with torch.enable_grad():
        for method, kw in (("mark_donor_shapley", {}), ("mark_donor_epistasis", {}), ("mark_donor_coalitions", dict(keep=[127, 0]))):
            out = model(*_args(b))
            res = getattr(model, method)(*_args(batches[1]), donor=_feats(b), **kw)
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
    model.mark_donor_coalitions((bs, keep), donor=dn, keep=[5])
    dl = torch.zeros(4, 2, device="cuda")
    assert _lib.lib().cf_backward_from(model._handle, C.byref(bs), dl.data_ptr(), st) != 0
    assert b"must follow cf_forward" in _lib.lib().cf_last_error()

    def others(m):
        ig = m.integrated_gradients(*_args(b), n_steps=3)
        return [m.pcre_shapley(*_args(b))[0].cpu(), ig[0]["interaction_freq"].cpu(), ig[1]["delta"].cpu(),
                m.perturbation_scan_regions(*_args(b), regions=[0, 2], mark_sets=[ALL, (3,)])[0].cpu(),
                m.mark_shapley(*_args(b), scale=0.5)[0].cpu()]

    def mine(m):      # (a donor call is the first call on a fresh handle: it allocates the workspace)
        return [m.mark_donor_shapley(*_args(b), donor=dn)[0].cpu(), m.mark_donor_epistasis(*_args(b), donor=dn, players="regions")[0].cpu(),
                m.mark_donor_coalitions(*_args(b), donor=dn, keep=[0, 9, 127]).cpu()]

    fresh = _model(None, False, P, 8)
    ref_mine, ref_others = mine(fresh), others(_model(None, False, P, 8))
    assert bool((ref_mine[0] != 0).any())
    mixed = _model(None, False, P, 8)
    a = mixed.pcre_shapley(*_args(b))[0].cpu()
    s = mixed.mark_donor_shapley(*_args(b), donor=dn)[0].cpu()
    ig = mixed.integrated_gradients(*_args(b), n_steps=3)
    e = mixed.mark_donor_epistasis(*_args(b), donor=dn, players="regions")[0].cpu()
    sc = mixed.perturbation_scan_regions(*_args(b), regions=[0, 2], mark_sets=[ALL, (3,)])[0].cpu()
    c = mixed.mark_donor_coalitions(*_args(b), donor=dn, keep=[0, 9, 127]).cpu()
    ms = mixed.mark_shapley(*_args(b), scale=0.5)[0].cpu()
    assert all(torch.equal(x, y) for x, y in zip([s, e, c], ref_mine))
    assert all(torch.equal(x, y) for x, y in zip([a, ig[0]["interaction_freq"].cpu(), ig[1]["delta"].cpu(), sc, ms], ref_others))
    assert all(torch.equal(x, y) for x, y in zip(others(fresh), ref_others))      # ... and after the donor calls alone
    assert all(torch.equal(x, y) for x, y in zip(mine(mixed), ref_mine))          # ... and the donor calls after everything else


def test_no_side_effects_on_training():
    from chromoformer_amd.engine import Trainer
    batches = [orc.synthetic_batch(8, seed=41 + i, regime="realistic") for i in range(4)]
    P = orc.init_params(None, 42, False)
    dn = _feats(_dev(batches[3]))

    def run(interpose):
        model = _model(None, False, P, 8)
        tr = Trainer(model, lr=1e-3)
        slots = [tr.stage(b) for b in batches[:3]]
        tr.step(slots[0])
        torch.cuda.synchronize()
        snap = [t.clone() for t in (model._flat, model._gflat, model._mflat, model._vflat)]
        grads = [None if p.grad is None else p.grad.clone() for p in model.parameters()]
        if interpose:
            model.mark_donor_shapley(*_args(batches[2]), donor=dn)
            model.mark_donor_epistasis(*_args(batches[2]), donor=dn, players="compartments")
            model.mark_donor_coalitions(*_args(batches[2]), donor=dn, keep=[0, 1], players=OVERLAP)
            torch.cuda.synchronize()
            for x, y in zip(snap, (model._flat, model._gflat, model._mflat, model._vflat)):
                assert torch.equal(x, y)
            for x, p in zip(grads, model.parameters()):
                assert (x is None and p.grad is None) or torch.equal(x, p.grad)
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
    npy, dnpy = str(tmp_path / "npy"), str(tmp_path / "donor")
    meta = make_dataset(npy, n_genes=20, seed=11)
    dn = do.donor_dataset(npy, dnpy, do.DONOR_SEED, w_prom=40000)
    genes = pd.read_csv(meta).gene_id.tolist()
    P = orc.init_params(seed=7)
    ck = str(tmp_path / "w.pt")
    torch.save({"net": P}, ck)
    out, eout = str(tmp_path / "donor.npz"), str(tmp_path / "eps.npy")
    assert predict.main(["-m", meta, "-d", npy, "-w", ck, "-o", str(tmp_path / "p.csv"), "--donor-npy-dir", dnpy, "--mark-donor-shapley-out", out,
                         "--mark-donor-epistasis-out", eout, "--mark-players", "regions"]) == 0
    z = np.load(out)
    assert sorted(z.files) == ["donor", "donor_prediction", "gene_ids", "logits", "phi", "players"]
    assert list(z["gene_ids"]) == genes and list(z["players"]) == ["promoter"] + ["pcre%d" % j for j in range(8)]
    assert z["phi"].shape == (20, 9) and z["phi"].dtype == np.float32 and z["logits"].shape == z["donor"].shape == z["donor_prediction"].shape == (20,)
    eps = np.load(eout)
    assert eps.shape == (20, 9, 9) and eps.dtype == np.float32 and np.array_equal(eps, eps.transpose(0, 2, 1))
    # the per-batch calls on the stores predict() builds: the same bits
    ds = ChromoformerDataset(meta, npy, genes)
    model = ChromoformerClassifier(seed=123, max_batch=32).cuda(0)
    model.load_state_dict(P)
    store, dstore = GeneStore(ds, device=model._device, resident=True), GeneStore(dn, device=model._device, resident=True)
    d, dd = store.batch(list(range(20))), dstore.batch(list(range(20)))
    phi, info = model.mark_donor_shapley(*_args(d), donor=_feats(dd), players="regions", return_coalitions=True)
    dbound = _check_phi(phi, info, 9)
    assert np.array_equal(z["phi"], phi.cpu()[..., 1].numpy()) and np.array_equal(z["logits"], info["logits"].cpu()[:, 1].numpy())
    assert np.array_equal(z["donor"], info["donor"].cpu()[:, 1].numpy())
    assert np.array_equal(eps, model.mark_donor_epistasis(*_args(d), donor=_feats(dd), players="regions")[0].cpu()[..., 1].numpy())
    gap = np.abs(z["phi"].astype(np.float64).sum(1) - (z["logits"].astype(np.float64) - z["donor"]))      # phi.sum(0) = logits - donor per gene
    assert (gap <= dbound[:, 1]).all(), (gap.max(), dbound.max())
    assert np.array_equal(z["donor_prediction"], _plain(model, dd)[:, 1].numpy()) and (z["donor_prediction"] != z["logits"]).all()
    sig = torch.sigmoid(torch.from_numpy(z["logits"])).numpy()
    assert np.abs(sig - pd.read_csv(str(tmp_path / "p.csv"))["prediction"].to_numpy()).max() <= 2.0 ** -23
    n_pcres = np.array([min(len(ds.genes[g]["pcres"]), 8) for g in genes])
    for i in range(20):      # a slot that is a dummy in both cell types is a null player
        assert (z["phi"][i, 1 + n_pcres[i]:] == 0).all() and (z["phi"][i, :1 + n_pcres[i]] != 0).all(), i
    # the generator, in chunks of 7 genes from the raw files, then from packed stores: the per-batch calls' bits
    sub = genes[3:13]
    for packed in (False, True):
        st = dst = None
        if packed:
            path, dpath = str(tmp_path / "genes.cfstore"), str(tmp_path / "donor.cfstore")
            pack.pack(meta, npy, path)
            pack.pack(os.path.join(dnpy, "meta.csv"), dnpy, dpath)
            st = pack.PackedStore(path).store(sub, device=model._device, regression=False)
            dst = pack.PackedStore(dpath).store(sub, device=model._device, regression=False)
        res = list(model.mark_donor_shapley_dataset(ds, dn, genes=sub, epistasis=True, bsz=7, store=st, donor_store=dst))
        assert [r["gene_id"] for r in res] == sub
        src = st if packed else GeneStore(_subset(ds, sub), device=model._device, resident=True)
        dsrc = dst if packed else GeneStore(_subset(dn, sub), device=model._device, resident=True)
        for lo in (0, 7):
            n = min(7, 10 - lo)
            b, db = src.batch(list(range(lo, lo + n))), dsrc.batch(list(range(lo, lo + n)))
            phi, info = model.mark_donor_shapley(*_args(b), donor=_feats(db))
            e = model.mark_donor_epistasis(*_args(b), donor=_feats(db))[0].cpu().numpy()
            pred = _plain(model, db).numpy()
            for i in range(n):
                r = res[lo + i]
                assert sorted(r) == ["donor", "donor_prediction", "eps", "gene_id", "logits", "phi", "players"]
                assert r["players"] == ["mark%d" % f for f in range(7)]
                assert r["phi"].shape == (7, 2) and r["phi"].dtype == np.float32 and r["eps"].shape == (7, 7, 2)
                assert np.array_equal(r["phi"], phi[i].cpu().numpy()) and np.array_equal(r["eps"], e[i])
                assert np.array_equal(r["logits"], info["logits"][i].cpu().numpy()) and np.array_equal(r["donor"], info["donor"][i].cpu().numpy())
                assert np.array_equal(r["donor_prediction"], pred[i])
    with pytest.raises(ValueError, match="mark_players"):
        next(model.mark_donor_shapley_dataset(ds, dn, genes=sub, players="genes"))
    far = ChromoformerDataset(os.path.join(dnpy, "meta.csv"), dnpy, genes, w_prom=38000)
    with pytest.raises(ValueError, match="same_regions: .*w_prom"):
        next(model.mark_donor_shapley_dataset(ds, far, genes=sub))


def _subset(ds, genes):
    import copy
    sub = copy.copy(ds)
    sub.target_genes = list(genes)
    return sub
