"""Harsanyi dividends and interaction indices of any order on the GPU (cf_dividends_from_rows, cf_set_interactions_from_dividends,
ChromoformerBase.shapley_dividends / set_interactions / *_dividends, the `dividends=` option of the dataset generators, predict
--*-dividends-out): a Moebius transform (k_moebius, k_moebius_high) of the [B, 2^P, n_out] table the exact Shapley calls reduce, and a
weighted superset sum of it (k_set_index).

  * the transform on random tables at the smallest sizes and on both sides of the 4,096-word tile (P = 12 | 13): the bits of the fp32
    restatement of the recurrence, the float64 subset-sum definition within ((1 + 2^-24)^|S| - 1) mass(S), null players exactly +0,
    one launch up to P = 12 and two above;
  * the set index: the bits of the restatement of k_set_index, the float64 discrete-derivative definition within the bound derived in
    test_set_interactions_on_random_tables, orders 1 and 2 against k_shapley and k_shapley_pairs, the copied sti sets;
  * every refusal by name with nothing launched;
  * the five games end to end: the operator on the sibling's table bit for bit, the sibling's phi, null players, training left alone,
    a dataset generator and the CLI.

Shapes and fixtures are those of tests/test_shapley_interactions_gpu.py."""
import numpy as np
import pandas as pd
import pytest
import torch

from chromoformer_amd import _lib
from chromoformer_amd.attribution import dividend_bound, interaction_sets, set_names
from oracle import chromoformer_oracle as orc
from tests import dividend_oracle as dv
from tests import donor_oracle as do
from tests.coalition_oracle import shapley_fp64
from tests.interaction_oracle import pair_index_fp64
from tests.test_input_grads_gpu import _model
from tests.test_mark_donor_gpu import _dev, _feats
from tests.test_mark_fine_windows_cpu import PLAYERS
from tests.test_mark_fine_windows_gpu import ZOOMS
from tests.test_mark_windows_gpu import THREE
from tests.test_pcre_coalitions_gpu import _dummies, _gamma
from tests.test_shapley_interactions_gpu import _args, _gamma_pairs, _subset, data, models, pcre      # noqa: F401  (module-scoped fixtures)

pytestmark = pytest.mark.gpu
INDICES = ("sii", "sti")


def _table(B, P, n_out):
    g = torch.Generator().manual_seed(1000 * P + 10 * B + n_out)
    return torch.randn(B, 1 << P, n_out, generator=g) * 3 + torch.randn(B, 1, n_out, generator=g)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("n_out", [1, 2])
@pytest.mark.parametrize("P,B", [(1, 3), (2, 3), (7, 3), (12, 3), (13, 3), (16, 3), (16, 2)])
def test_the_transform_on_random_tables(models, P, B, n_out):
    """P = 1, 2: the smallest tables; 7: the marks; 12: exactly one LDS tile; 13: two tiles and one register stage; 16: sixteen tiles and
    four register stages.  The bound: an element passes through |S| rounded subtractions of quantities whose magnitudes sum to at most
    mass(S) = sum over T <= S of |v(T)|, so |div - exact| <= ((1 + 2^-24)^|S| - 1) mass(S).  The bound is sharp: a single subtraction of two numbers of opposite sign can miss by half an ulp of a result as large as
    the mass, and the largest error measured here is 0.999 of it (P = 16)."""
    model = models.small if n_out == 2 else models.reg
    rows = _table(B, P, n_out)
    dev = rows.cuda()
    div, mass = model.shapley_dividends(dev, return_mass=True)
    launches = model.launch_counts()[0]
    alone = model.shapley_dividends(dev)
    assert launches == model.launch_counts()[0] == (1 if P <= 12 else 2)
    torch.cuda.synchronize()
    v = rows.numpy()
    assert not div.requires_grad and torch.equal(dev.cpu(), rows) and torch.equal(alone, div)
    assert _same_bits(div.cpu().numpy(), dv.moebius_fp32(v)) and _same_bits(mass.cpu().numpy(), dv.mass_fp32(v))
    err, bound = np.abs(div.cpu().numpy().astype(np.float64) - dv.moebius_fp64(v)), dv.dividend_bound(v)
    print("P %d: max err %.3e, max bound %.3e, max err / bound %.3f" % (P, err.max(), bound.max(), (err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()
    assert (err <= dividend_bound(mass.cpu().numpy(), P)).all()      # the public bound from the device's own mass
    assert torch.equal(model.shapley_dividends(rows), div)      # (a host table is moved)
    # a null player: its rows bit-equal present and absent -> every set that holds it is exactly +0
    words = np.arange(1 << P)
    for null in sorted({0, P // 2, P - 1}):
        vn = rows[:, torch.from_numpy(words & ~(1 << null))]
        dn = model.shapley_dividends(vn.cuda()).cpu().numpy()
        holds = (words >> null & 1) == 1
        assert _same_bits(dn[:, holds], np.zeros_like(dn[:, holds])) and _same_bits(dn, dv.moebius_fp32(vn.numpy())), null
        assert (dn[:, ~holds] != 0).any(-1).all()


@pytest.mark.parametrize("n_out", [1, 2])
@pytest.mark.parametrize("P,B,orders", [(7, 3, (7, 3)), (16, 2, (3,))])
def test_set_interactions_on_random_tables(models, P, B, orders, n_out):
    """All 127 sets at P = 7 (order 7, and the 63 of order 3), all 696 at P = 16, order 3: up to 2^15 supersets per set, 128 per thread.

    The bound against the float64 discrete-derivative definition (tests/dividend_oracle.py: set_index_bound), from the kernel's
    operation count.  A set with n = 2^(P - |S|) supersets gives a thread n_t = ceil(n / 256) terms.  On a term's way to the result lie
    the rounding of its weight, of its product, at most n_t - 1 additions in the thread (the first is to 0) and the 8 of the tree:
    n_t + 9 factors (1 + e), |e| <= 2^-24.  The term's dividend is itself within ((1 + 2^-24)^|U| - 1) mass(U) of the exact m(U).  So
        |out - exact| <= sum over U >= S of w (g |m(U)| + (1 + g) dividend_bound(U)),      g = (1 + 2^-24)^(n_t + 9) - 1.
    The dividends' share dominates and is a worst case that adds up every high-order dividend's own bound: at P = 16 the fp32
    restatement sits at 3e-4 of it under sii.  The sharp check is the restatement, bit for bit."""
    model = models.small if n_out == 2 else models.reg
    rows = _table(B, P, n_out)
    v = rows.numpy()
    dev = rows.cuda()
    div = model.shapley_dividends(dev)
    d = div.cpu().numpy()
    for order in orders:
        want = interaction_sets(P, order)
        for index in INDICES:
            inter, sets = model.set_interactions(div, order=order, index=index)
            assert model.launch_counts()[0] == 1 and np.array_equal(sets, want) and sets.dtype == np.uint32
            got = inter.cpu().numpy()
            assert got.shape == (B, len(want), n_out) and not inter.requires_grad
            assert _same_bits(got, dv.set_index_fp32(d, want, index, order)), (order, index)
            err, bound = np.abs(got.astype(np.float64) - dv.set_index_fp64(v, want, index, order)), dv.set_index_bound(v, want, index, order)
            print("P %d order %d %s: max err %.3e, max err / bound %.3f" % (P, order, index, err.max(), (err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all(), (order, index)
            if index == "sti":      # below the top order: the dividend's bits
                low = dv.popcount(want) < order
                assert low.sum() == (len(want) - 1 if order == P else len(interaction_sets(P, order - 1))) and _same_bits(got[:, low], d[:, want[low]])
            # listed sets: any order, repeats allowed
            pick = want[::-1][:5].copy()
            some, back = model.set_interactions(div, order=order, index=index, sets=torch.from_numpy(pick.astype(np.int64)))
            assert np.array_equal(back, pick) and _same_bits(some.cpu().numpy(), got[:, ::-1][:, :5])
    # orders 1 and 2 are k_shapley's and k_shapley_pairs's quantities: within the two bounds of each other
    phi64, pscale = shapley_fp64(v)
    players = np.arange(P)
    for index in INDICES:
        pair = model.shapley_interactions(dev, index=index).cpu().numpy()
        _, scale = pair_index_fp64(v, index)
        two, sets = model.set_interactions(div, order=2, index=index)
        two, bound = two.cpu().numpy(), dv.set_index_bound(v, sets, index, 2)
        for k, S in enumerate(int(s) for s in sets):
            p = [b for b in range(P) if S >> b & 1]
            i, j = p[0], p[-1]
            if i == j and index == "sti":
                assert _same_bits(two[:, k], pair[:, i, i])      # v({i}) - v(0): one subtraction in both
                continue
            other = _gamma(P) * pscale[:, i] if i == j else _gamma_pairs(P) * scale[:, i, j]      # the sii diagonal is k_shapley's phi
            assert (np.abs(two[:, k].astype(np.float64) - pair[:, i, j]) <= bound[:, k] + other).all(), (index, S)
    one, sets = model.set_interactions(div, order=1, index="sii")
    phi = model.shapley_interactions(dev, index="sii").cpu().numpy()[:, players, players]      # the sii diagonal carries k_shapley's bits
    assert sets.tolist() == (1 << players).tolist()
    assert (np.abs(one.cpu().numpy().astype(np.float64) - phi) <= dv.set_index_bound(v, sets, "sii", 1) + _gamma(P) * pscale).all()
    assert (np.abs(phi - phi64) <= _gamma(P) * pscale).all()


def test_refusals_by_name_with_nothing_launched(models):
    L, model = _lib.lib(), models.small
    model.shapley_dividends(torch.zeros(1, 2, 2))
    f0 = model.launch_counts()
    st = torch.cuda.current_stream().cuda_stream
    rows = torch.zeros(3, 256, 2, device="cuda")
    out = torch.full((3, 256, 2), float("nan"), device="cuda")
    h, r, o = model._handle, rows.data_ptr(), out.data_ptr()

    def words(*w):
        return np.array(w, dtype=np.uint32)

    def refused(rc, *needles):
        err = L.cf_last_error()
        assert rc != 0 and all(n in err for n in needles), err

    name, fn = b"cf_dividends_from_rows", L.cf_dividends_from_rows
    refused(fn(None, r, 3, 8, o, None, st), name, b"null handle")
    refused(fn(h, None, 3, 8, o, None, st), name, b"null rows")
    refused(fn(h, r, 3, 8, None, o, st), name, b"null div")
    refused(fn(h, r, 0, 8, o, None, st), name, b"B = 0")
    for P in (0, 17, -3):
        refused(fn(h, r, 3, P, o, None, st), name, b"P = %d outside 1..16" % P)
    name, fn = b"cf_set_interactions_from_dividends", L.cf_set_interactions_from_dividends
    good = words(1, 3)
    refused(fn(None, r, 3, 8, good.ctypes.data, 2, 0, 2, o, st), name, b"null handle")
    refused(fn(h, None, 3, 8, good.ctypes.data, 2, 0, 2, o, st), name, b"null div")
    refused(fn(h, r, 3, 8, None, 2, 0, 2, o, st), name, b"null sets")
    refused(fn(h, r, 3, 8, good.ctypes.data, 2, 0, 2, None, st), name, b"null out")
    refused(fn(h, r, 0, 8, good.ctypes.data, 2, 0, 2, o, st), name, b"B = 0")
    for P in (0, 17):
        refused(fn(h, r, 3, P, good.ctypes.data, 2, 0, 1, o, st), name, b"P = %d outside 1..16" % P)
    for n in (0, -1, 65536):
        refused(fn(h, r, 3, 8, good.ctypes.data, n, 0, 2, o, st), name, b"n_sets = %d" % n)
    for order in (0, 9, -1):
        refused(fn(h, r, 3, 8, good.ctypes.data, 2, 0, order, o, st), name, b"order = %d outside 1..P = 8" % order)
    for index in (2, -1):
        refused(fn(h, r, 3, 8, good.ctypes.data, 2, index, 2, o, st), name, b"index = %d" % index)
    for bad, msg in ((words(1, 0), b"sets[1] is the empty set"), (words(1, 2, 1 << 8), b"sets[2] = 0x100 names a player >= P = 8"),
                     (words(3, 7), b"sets[1] = 0x7 holds 3 players, more than order = 2")):
        refused(fn(h, r, 3, 8, bad.ctypes.data, len(bad), 1, 2, o, st), name, msg)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and model.launch_counts() == f0      # nothing was launched
    # the Python layer
    div = torch.zeros(2, 16, 2)
    for kw in (dict(order=0), dict(order=5), dict(sets=[]), dict(sets=[[1, 2]]), dict(sets=[1.5]), dict(sets=[16]), dict(sets=[-1]), dict(index="shap")):
        with pytest.raises(ValueError, match="set_interactions"):
            model.set_interactions(div, **kw)
    with pytest.raises(RuntimeError, match=r"sets\[1\] is the empty set"):
        model.set_interactions(div, sets=[3, 0])
    with pytest.raises(RuntimeError, match="more than order = 2"):
        model.set_interactions(div, sets=[7])
    for bad in (torch.zeros(3, 100, 2), torch.zeros(3, 4, 1), torch.zeros(3, 1 << 17, 2)):
        with pytest.raises(ValueError, match="shapley_dividends"):
            model.shapley_dividends(bad)


def _game(call, sibling, model, operator_model, absent, P):
    """call(model) -> (div, info) against sibling(model) -> (phi, info with the table): the operator on the sibling's table bit for bit,
    the sibling's phi and info, the set names, and the dividends add back up to the prediction within their own bounds."""
    phi, sinfo = sibling(model)
    div, info = call(model)
    assert model.launch_counts()[0] == 1      # the transform was the last call: P <= 12
    table = sinfo["coalitions"]
    assert sorted(info) == sorted(list(sinfo) + ["phi", "mass", "names", "sets"]) and not div.requires_grad
    assert torch.equal(info["coalitions"], table) and torch.equal(info["phi"], phi)
    assert torch.equal(info["logits"], table[:, -1]) and torch.equal(info[absent], table[:, 0]) and torch.equal(info["delta"], sinfo["delta"])
    d2, m2 = operator_model.shapley_dividends(table, return_mass=True)
    assert torch.equal(div, d2) and torch.equal(info["mass"], m2) and div.shape == table.shape
    assert len(info["names"]) == P and info["sets"] == set_names(np.arange(1 << P), info["names"]) and info["sets"][0] == ""
    if "players" in sinfo:
        assert info["names"] == sinfo["players"]
    v, d = table.cpu().numpy(), div.cpu().numpy()
    assert _same_bits(d, dv.moebius_fp32(v)) and _same_bits(d[:, 0], v[:, 0])
    gap = np.abs(d.astype(np.float64).sum(1) - v[:, -1])
    assert (gap <= dividend_bound(info["mass"].cpu().numpy(), P).sum(1)).all()
    return div.cpu(), info


def test_pcre_game(pcre):
    a = _args(pcre.batch)
    div, info = _game(lambda m: m.pcre_dividends(*a), lambda m: m.pcre_shapley(*a, return_coalitions=True), pcre.five, pcre.seven, "promoter_only", 3)
    assert info["names"] == ["pcre0", "pcre1", "pcre2"] and info["sets"][5] == "pcre0*pcre2"
    dummy = _dummies(pcre.batch).numpy()      # a dummy slot is a null player: every set that holds one is exactly 0, the others are not
    assert dummy.sum(1).tolist() == [0, 0, 0, 2, 3]
    holds = ((np.arange(8)[None, :, None] >> np.arange(3)[None, None, :] & 1).astype(bool) & dummy[:, None, :]).any(-1)      # [B, 8]
    assert bool((div[torch.from_numpy(holds)] == 0).all()) and bool((div[torch.from_numpy(~holds)] != 0).any(-1).all())


def test_mark_and_donor_games(data, models):
    a = _args(data.dev)
    div, info = _game(lambda m: m.mark_dividends(*a), lambda m: m.mark_shapley(*a, return_coalitions=True), models.small, models.seven, "erased", 7)
    assert div.shape == (3, 128, 2) and info["sets"][0b1001001] == "mark0*mark3*mark6"
    # orders 1 and 2 from the dividends against the game's own phi and pair index
    inter, sets = models.small.set_interactions(div, order=2)
    pair, pinfo = models.small.mark_shapley_interactions(*a)
    assert torch.equal(pinfo["phi"], info["phi"])
    v = info["coalitions"].cpu().numpy()
    bound = dv.set_index_bound(v, sets, "sii", 2)
    _, scale = pair_index_fp64(v, "sii")
    for k, S in enumerate(int(s) for s in sets):
        p = [b for b in range(7) if S >> b & 1]
        err = np.abs(inter[:, k].cpu().numpy().astype(np.float64) - pair[:, p[0], p[-1]].cpu().numpy())
        assert (err <= bound[:, k] + (_gamma(7) if len(p) == 1 else _gamma_pairs(7)) * scale[:, p[0], p[-1]]).all(), S
    small = [((0, 1), (0,)), ((2, 3), (0, 1)), ((4, 5, 6), (0, 1, 2))]
    packed = models.small.pack_batch(data.dev)
    assert torch.equal(models.small.mark_dividends(packed, players=small, scale=0.5)[0], models.small.mark_dividends(*a, players=small, scale=0.5)[0])
    don = _feats(data.ddev)
    _game(lambda m: m.mark_donor_dividends(*a, donor=don, players=small), lambda m: m.mark_donor_shapley(*a, donor=don, players=small, return_coalitions=True),
          models.small, models.seven, "donor", 3)


def test_window_and_fine_games(data, models):
    a = _args(data.dev)
    kw = dict(players=THREE, flip=data.flips, scale=2.5)
    div, info = _game(lambda m: m.mark_window_dividends(*a, **kw), lambda m: m.mark_window_shapley(*a, return_coalitions=True, **kw), models.small,
                      models.seven, "erased", 3)
    # pCRE slot 7 is a dummy slot of gene 2: player 2 is null there
    assert bool((div[2, 4:] == 0).all()) and bool((div[2, :4] != 0).any(-1).all()) and bool((div[:2] != 0).any(-1).all())
    with pytest.raises(ValueError, match="17 players"):
        models.small.mark_window_dividends(*a, players=[(tuple(range(7)), (0,), (g, g + 1)) for g in range(17)])
    kw = dict(players=PLAYERS[:4], start=ZOOMS[0][0], lengths=ZOOMS[0][1], flip=data.flips, donor=_feats(data.ddev))
    _game(lambda m: m.mark_fine_window_dividends(*a, **kw), lambda m: m.mark_fine_window_shapley(*a, return_coalitions=True, **kw), models.small,
          models.seven, "donor", 4)
    # windows past bin 390, beside a real one (start 350: [350, 355), [390, 397), [395, 410)): players 1 and 2 are null
    players = [(tuple(range(7)), (0, 5)), ((1, 4), (40, 47)), (tuple(range(7)), (45, 60))]
    div = models.small.mark_fine_window_dividends(*a, players=players, start=350, flip=data.flips)[0].cpu()
    assert bool((div[:, 2:] == 0).all()) and bool((div[:, :2] != 0).any(-1).all())


def test_training_is_left_alone_and_the_operators_leave_a_pending_backward():
    from chromoformer_amd.engine import Trainer
    batches = [orc.synthetic_batch(4, seed=41 + i, regime="realistic") for i in range(3)]
    P = orc.init_params(None, 42, False)
    model = _model(None, False, P, 8)
    three = [((0, 1), (0,)), ((2, 3), (0, 1)), ((4, 5, 6), (0, 1, 2))]
    calls = (("pcre_dividends", "pcre_shapley", {}), ("mark_dividends", "mark_shapley", dict(players=three)),
             ("mark_donor_dividends", "mark_donor_shapley", dict(players=three, donor=_feats(_dev(batches[2])))),
             ("mark_window_dividends", "mark_window_shapley", dict(players=THREE)),
             ("mark_fine_window_dividends", "mark_fine_window_shapley", dict(players=PLAYERS[:3])))
    with torch.enable_grad():
        out = model(*_args(batches[0]))
        res = model.mark_dividends(*_args(_dev(batches[1])), players=three)      # the sibling's forwards overwrite the activations
        assert not res[0].requires_grad
        with pytest.raises(RuntimeError, match="mark_shapley"):
            out[:, 1].sum().backward()
        out = model(*_args(batches[0]))
        div = model.shapley_dividends(torch.randn(4, 8, 2))      # the operators run no forward: the pending backward goes through
        model.set_interactions(div, order=3, index="sti")
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
            for method, _sib, kw in calls:
                div, info = getattr(m, method)(*_args(_dev(batches[2])), **kw)
                m.set_interactions(div, order=min(3, len(info["names"])), index="sti")
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
    out = str(tmp_path / "marks.npz")
    assert predict.main(["-m", meta, "-d", npy, "-w", ck, "-o", str(tmp_path / "p.csv"), "--mark-dividends-out", out, "--mark-scale", "0.5"]) == 0
    model = ChromoformerClassifier(seed=123, max_batch=32).cuda(0)
    model.load_state_dict(P)
    store = GeneStore(ds, device=model._device, resident=True)
    a = _args(store.batch(list(range(20))))
    div, info = model.mark_dividends(*a, scale=0.5)
    z = np.load(out)
    assert sorted(z.files) == ["dividends", "gene_ids", "mass", "players", "sets"] and z["gene_ids"].tolist() == genes
    assert _same_bits(z["dividends"], div.cpu()[..., 1].numpy()) and _same_bits(z["mass"], info["mass"].cpu()[..., 1].numpy())
    assert z["sets"].tolist() == info["sets"] and z["players"].tolist() == info["names"] and z["dividends"].shape == (20, 128)
    for argv in (["--mark-donor-dividends-out", out], ["--mark-dividends-out", out, "--mark-scale", "-1"],
                 ["--pcre-dividends-out", out, "--mark-players", "regions"]):
        with pytest.raises(SystemExit) as e:
            predict.main(["-m", meta, "-d", npy, "-w", ck, "-o", str(tmp_path / "q.csv")] + argv)
        assert e.value.code == 2, argv
    # the generators: dividends=False yields the sibling's dict key for key; True adds `dividends` and `mass` from the same forwards
    sub = genes[2:9]
    gs, gd = GeneStore(_subset(ds, sub), device=model._device, resident=True), GeneStore(_subset(dn, sub), device=model._device, resident=True)
    b, bd = gs.batch(list(range(7))), gd.batch(list(range(7)))
    flip = [ds.genes[g]["tss"][2] != "+" for g in sub]
    three = [((0, 1), (0,)), ((2, 3), (0, 1)), ((4, 5, 6), (0, 1, 2))]
    cases = [(lambda **kw: model.mark_shapley_dataset(ds, genes=sub, players=three, bsz=7, **kw), lambda: model.mark_dividends(*_args(b), players=three)),
             (lambda **kw: model.mark_donor_shapley_dataset(ds, dn, genes=sub, players=three, bsz=7, interactions="sti", **kw),
              lambda: model.mark_donor_dividends(*_args(b), donor=_feats(bd), players=three)),
             (lambda **kw: model.mark_window_shapley_dataset(ds, genes=sub, width=5, bsz=7, **kw),
              lambda: model.mark_window_dividends(*_args(b), width=5, flip=flip))]
    for gen, call in cases:
        plain, default, res = list(gen()), list(gen(dividends=False)), list(gen(dividends=True))
        assert [r["gene_id"] for r in res] == sub
        div, info = call()
        for i, (p, q, r) in enumerate(zip(plain, default, res)):
            assert sorted(p) == sorted(q) and sorted(r) == sorted(list(p) + ["dividends", "mass"])
            for k in p:
                same = np.array_equal(p[k], r[k]) if isinstance(p[k], np.ndarray) else p[k] == r[k]
                assert same and (np.array_equal(p[k], q[k]) if isinstance(p[k], np.ndarray) else p[k] == q[k]), k
            assert _same_bits(r["dividends"], div[i].cpu().numpy()) and _same_bits(r["mass"], info["mass"][i].cpu().numpy())
    # the fine generator: per rank the dividends of the whole fine game; the empty set carries v(nobody)
    kw = dict(genes=sub, region=1, zoom=1, coarse_width=5, width=25, scale=0.25, bsz=4)
    plain, res = list(model.mark_fine_window_shapley_dataset(ds, **kw)), list(model.mark_fine_window_shapley_dataset(ds, dividends=True, **kw))
    assert any(len(r["dividends"]) for r in res)
    for p, r in zip(plain, res):
        assert sorted(r) == sorted(list(p) + ["dividends", "mass"]) and np.array_equal(p["phi"], r["phi"])
        assert len(r["dividends"]) == len(r["mass"]) == len(r["zoom"])
        for rank, x in enumerate(r["dividends"]):
            assert x.shape == (16, 2) and _same_bits(x[0], r["absent"][rank]) and r["mass"][rank].shape == (16, 2)
    # a game that would be sampled has no dividends
    with pytest.raises(ValueError, match="20 players"):
        next(model.mark_window_shapley_dataset(ds, genes=sub, width=1, dividends=True))
    with pytest.raises(ValueError, match="25 fine players"):
        next(model.mark_fine_window_shapley_dataset(ds, genes=sub, region=1, coarse_width=5, width=4, dividends=True))
