"""The contact games on the GPU (cf_contact_coalitions / cf_contact_shapley / cf_contact_epistasis / cf_contact_shapley_interactions and
the functions of chromoformer_amd.contact): a player deletes pCRE slots and / or edits their promoter contact frequencies while it is
absent; row (b, m) is the inference forward of gene b on the tensors tests/contact_oracle.contact_batch gives for the word m.

  * every row bit-identical to model(...) on the explicitly edited batch, both rules, on the realistic batch and on dense signed
    frequencies (where a transposed or row-0-only edit would show); players that only drop give the pCRE game's bits;
  * the exact game of the eight contacts: phi within the fp32 rounding bound of its own table, the efficiency gap, the reference's logits;
  * null players exactly 0; the joint game at i_max = 3: `contact j` null next to an absent `pcre j`, its dividends exactly 0, the
    interaction indices, the epistasis and the back-selection on the kept table;
  * chunking, call after call; i_max = 16; a layer-by-layer Regulation shape;
  * the C ABI: launches, refusals by name, the handle-owned row buffer, the packed forms; no side effects on training, a pending
    backward refused;
  * the dataset generator and `predict.py --contact-shapley-out / --contact-donor-shapley-out`."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import chromoformer_oracle as orc
from tests.coalition_oracle import epistasis_fp32, pair_words, shapley_fp64
from tests.contact_oracle import contact_batch
from tests.helpers import GOLDEN, load_npz_batch
from tests.interaction_oracle import pair_index_fp64
from tests.unstructured_inputs import unstructured_batch

pytestmark = pytest.mark.gpu
TOL = 1e-4      # the project's logit bound
U = 2.0 ** -24
ARGS = ("promoter_feats", "promoter_pad_masks", "pcre_feats", "pcre_pad_masks", "interaction_masks", "interaction_freq")
REG_4x128 = dict(n_layers=6, n_heads=4, d_model=128, d_ff=256)


def _args(batch):
    return [batch[k] for k in ARGS]


def _take(batch, idx):
    return {k: ({b: t[idx] for b, t in v.items()} if isinstance(v, dict) else v[idx]) for k, v in batch.items()}


def _model(cfg=None, B=8, regression=False, seed=42):
    from chromoformer_amd import ChromoformerClassifier, ChromoformerRegressor
    c = orc._cfg(cfg)
    Model = ChromoformerRegressor if regression else ChromoformerClassifier
    return Model(c["n_feats"], c["d_emb"], c["d_head"], c["embed"], c["pairwise_interaction"], c["regulation"], binsizes=c["binsizes"],
                 seed=seed, i_max=c["i_max"], w_max=c["w_max"], max_batch=B).cuda(0)


def _players(spec, S):
    from chromoformer_amd.attribution import contact_players
    return contact_players(spec, S)


def _dummies(batch):
    """[B, S]: slots whose interaction-mask column is masked for the promoter row at every resolution (dataset dummies)."""
    return torch.stack([m[:, 0, 0, 1:] for m in batch["interaction_masks"].values()]).all(0)


def _words(P, n, seed):
    """n coalition words of P players: everybody, nobody, each of the first two players alone absent, then seeded draws."""
    full = (1 << P) - 1
    rng = np.random.RandomState(seed)
    return [full, 0, full & ~1, full & ~2] + [int(w) for w in rng.randint(0, 1 << P, n - 4)]


def _gamma(P):
    """n u / (1 - n u), n = 2^(P - 1) + 3: a term of a player's sum passes one rounded subtraction, the rounding of its weight, one
    rounded product and, whatever the order of the summation, at most 2^(P - 1) rounded additions: 2^(P - 1) + 3 factors (1 + e),
    |e| <= u = 2^-24, bound its relative error by gamma_n (Higham, Accuracy and Stability of Numerical Algorithms, Lemma 3.1).  (The
    device fuses product and addition into one rounding: one factor fewer, inside the bound.)"""
    n = 2 ** (P - 1) + 3
    return n * U / (1 - n * U)


def _check_phi(phi, info, P, absent="erased"):
    """phi against shapley_fp64 of the returned table, elementwise within gamma_n times sum w |difference| (the scale shapley_fp64
    returns); info["delta"] = phi.sum(1) - (logits - absent) within P times the largest such bound (the P values' own errors; their
    exact sum IS v(N) - v(0)) plus 4 u max |v| (the roundings of logits - absent and of the final subtraction)."""
    v = info["coalitions"].cpu().numpy()
    phi64, scale = shapley_fp64(v)
    bound = _gamma(P) * scale
    err = np.abs(phi.cpu().numpy().astype(np.float64) - phi64)
    print("phi: max err %.3e, max bound %.3e, max err / bound %.3f" % (err.max(), bound.max(), (err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all(), (err.max(), bound.max())
    dbound = P * bound.max(1) + 4 * U * np.abs(v).max(1)
    delta = np.abs(info["delta"].cpu().numpy())
    print("delta: max %.3e, max bound %.3e" % (delta.max(), dbound.max()))
    assert delta.shape == dbound.shape and (delta <= dbound).all(), (delta.max(), dbound.max())
    assert torch.equal(info["logits"], info["coalitions"][:, -1]) and torch.equal(info[absent], info["coalitions"][:, 0])


def _rows_are_the_forward(model, batch, spec, words, scale=0.0, donor=None):
    """contact_coalitions on `words` against model(...) on contact_batch, row by row, bit for bit -> the rows (host)."""
    from chromoformer_amd import contact
    drop, con, names = _players(spec, model.i_max)
    dev_donor = None if donor is None else donor.cuda().contiguous()
    got = contact.contact_coalitions(model, *_args(batch), keep=words, players=spec, scale=scale, donor_freq=dev_donor).cpu()
    assert not got.requires_grad and got.shape == (batch["interaction_freq"].shape[0], len(words), model.n_out)
    with torch.no_grad():
        for c, m in enumerate(words):
            ref = model(*_args(contact_batch(batch, m, drop, con, scale, donor))).cpu()
            assert torch.equal(got[:, c], ref), (spec, scale, donor is not None, c, hex(m))
    return got


def test_rows_are_the_forward_on_the_edited_batch_bit_for_bit():
    from chromoformer_amd import contact
    batch = orc.synthetic_batch(8, seed=31, regime="realistic")
    model = _model(B=8)
    dummy = _dummies(batch)
    assert any(bool(dummy[:, j].any()) and not bool(dummy[:, j].all()) for j in range(8))      # a slot that is a dummy in some genes only
    donor = torch.roll(batch["interaction_freq"], 3, 0) * 0.75 + 0.125
    w8, w16 = _words(8, 12, 3), _words(16, 12, 4)
    tables = {}
    for scale, don in ((0.0, None), (0.5, None), (1.0, None), (0.0, donor)):
        tables[scale, don is None] = _rows_are_the_forward(model, batch, "contacts", w8, scale, don)
        _rows_are_the_forward(model, batch, "pcres_and_contacts", w16, scale, don)
    zero, half, one, don = tables[0.0, True], tables[0.5, True], tables[1.0, True], tables[0.0, False]
    assert all(torch.equal(one[:, c], one[:, 0]) for c in range(12))      # scale = 1: every row the prediction
    assert not torch.equal(zero[:, 1], zero[:, 0]) and not torch.equal(half[:, 1], zero[:, 1]) and not torch.equal(don[:, 1], zero[:, 1])
    # players that only drop: the pCRE game, rows and Shapley values
    rows = contact.contact_coalitions(model, *_args(batch), keep=w8, players="pcres")
    assert torch.equal(rows, model.pcre_coalitions(*_args(batch), keep=w8))
    phi, info = contact.contact_shapley(model, *_args(batch), players="pcres", return_coalitions=True)
    phi_p, info_p = model.pcre_shapley(*_args(batch), return_coalitions=True)
    assert torch.equal(phi, phi_p) and torch.equal(info["coalitions"], info_p["coalitions"]) and info["players"] == ["pcre%d" % j for j in range(8)]
    # the bool form of keep, and a word naming a player the game does not have
    bits = torch.tensor([[bool(m >> p & 1) for p in range(8)] for m in w8])
    assert torch.equal(contact.contact_coalitions(model, *_args(batch), keep=bits).cpu(), zero)
    with pytest.raises(ValueError, match="contact_coalitions"):
        contact.contact_coalitions(model, *_args(batch), keep=[256])
    with pytest.raises(ValueError, match="keep is required"):
        contact.contact_coalitions(model, *_args(batch))


def test_dense_signed_frequencies_rows_above_0_and_columns_are_edited():
    """tests/unstructured_inputs: every one of the T x T frequencies is a signed number and the masks are unstructured, so an edit that
    touched row 0 alone, or rows in place of columns, gives other logits.  (unstructured_batch plants its three special genes at the end of
    a batch of at least 4: the first three genes of B = 4 -- a plain one, one with Regulation row 2 fully masked, one with row 0 fully
    masked.)"""
    full = unstructured_batch(4)
    batch = _take(full, slice(0, 3))
    model = _model(B=4)
    donor = torch.from_numpy(np.random.default_rng(9).normal(0.0, 1.5, size=(3, 9, 9)).astype(np.float32))
    w8, w16 = _words(8, 12, 5), _words(16, 12, 6)
    for scale, don in ((0.0, None), (-0.5, None), (1.0, None), (0.0, donor)):
        _rows_are_the_forward(model, batch, "contacts", w8, scale, don)
        _rows_are_the_forward(model, batch, "pcres_and_contacts", w16, scale, don)
    # not vacuous: an edit of row 0 alone, and the transposed edit (rows only / columns only), give other logits than the rule
    drop, con, _ = _players("contacts", 8)
    ruled = contact_batch(batch, 0, drop, con, 0.0)
    f, e = batch["interaction_freq"], ruled["interaction_freq"]
    assert bool((e[:, 1:, 1:] == 0).all()) and bool((e[:, 0, 1:] == 0).all()) and bool((e[:, 1:, 0] == 0).all()) and torch.equal(e[:, 0, 0], f[:, 0, 0])
    row0 = f.clone()
    row0[:, 0, 1:] = 0
    rows_only = f.clone()
    rows_only[:, 1:, :] = 0
    with torch.no_grad():
        want = model(*_args(ruled))
        for other in (row0, rows_only):
            assert not torch.equal(model(*_args(dict(batch, interaction_freq=other))), want)


def test_exact_game_of_the_contacts_phi_delta_and_the_reference():
    from chromoformer_amd import contact
    batch = orc.synthetic_batch(8, seed=31, regime="realistic")
    model = _model(B=8)
    phi, info = contact.contact_shapley(model, *_args(batch), return_coalitions=True)
    assert phi.shape == (8, 8, 2) and info["coalitions"].shape == (8, 256, 2) and not phi.requires_grad
    assert sorted(info) == ["coalitions", "delta", "erased", "logits", "players"] and info["players"] == ["contact%d" % j for j in range(8)]
    _check_phi(phi, info, 8)
    with torch.no_grad():
        assert torch.equal(info["logits"], model(*_args(batch)))
    dummy = _dummies(batch)
    assert bool((phi.cpu()[dummy] == 0).all()) and bool((phi.cpu()[~dummy] != 0).all())
    # the reference's logits on the demo batch: all 256 words at scale 0, and the recorded words of the other games
    z = np.load(os.path.join(GOLDEN, "contact_games.npz"))
    demo = load_npz_batch("demo_subset.npz")[0]
    rolled = torch.roll(demo["interaction_freq"], 1, 0).cuda().contiguous()
    for regression, tag in ((False, "clf"), (True, "reg")):
        m = _model(B=64, regression=regression)
        got = {"joint": contact.contact_coalitions(m, *_args(demo), keep=z["joint.words"], players="pcres_and_contacts"),
               "half": contact.contact_coalitions(m, *_args(demo), keep=z["words8"], scale=0.5),
               "donor": contact.contact_coalitions(m, *_args(demo), keep=z["words8"], donor_freq=rolled)}
        if not regression:
            got["contacts0"] = contact.contact_shapley(m, *_args(demo), return_coalitions=True)[1]["coalitions"]
        for name, t in got.items():
            ref = z["%s.%s" % (name, tag)]
            d = np.abs(t.cpu().numpy() - ref).max()
            print("%s.%s vs the reference: %.3e" % (name, tag, d))
            assert t.shape == ref.shape and d < TOL, (name, tag, d)


def test_null_players_are_exactly_zero():
    from chromoformer_amd import contact
    batch = orc.synthetic_batch(8, seed=31, regime="realistic")
    model = _model(B=8)
    dummy = _dummies(batch)
    assert bool(dummy.any())
    own = batch["interaction_freq"].cuda().contiguous()
    for kw in (dict(scale=1.0), dict(donor_freq=own)):
        phi, info = contact.contact_shapley(model, *_args(batch), return_coalitions=True, **kw)
        assert bool((phi == 0).all()) and bool((info["delta"] == 0).all()), kw
        assert bool((info["coalitions"] == info["logits"][:, None]).all())
        eps, _ = contact.contact_epistasis(model, *_args(batch), **kw)
        assert bool((eps == 0).all())
    assert "donor" in info and "erased" not in info
    for spec in ("contacts", "pcres_and_contacts"):      # flipping the bit of a dummy slot's player changes nothing in that gene
        P = len(_players(spec, 8)[2])
        keep = _words(P, 6, 8)
        rows = contact.contact_coalitions(model, *_args(batch), keep=keep, players=spec).cpu()
        for p in range(P):
            twins = contact.contact_coalitions(model, *_args(batch), keep=[m ^ 1 << p for m in keep], players=spec).cpu()
            gone = dummy[:, p % 8]
            assert torch.equal(twins[gone], rows[gone]), (spec, p)
            assert bool(gone.all()) or not torch.equal(twins[~gone], rows[~gone]), (spec, p)
    phi = contact.contact_shapley(model, *_args(batch), players="pcres_and_contacts")[0].cpu()
    both = torch.cat([dummy, dummy], 1)
    assert bool((phi[both] == 0).all()) and bool((phi[~both] != 0).any())


@pytest.fixture(scope="module")
def joint():
    """i_max = 3, 5 genes with [0, 0, 0, 2, 3] dummy slots, dense signed frequencies; the joint game's table (6 players, 64 rows)."""
    from chromoformer_amd import contact
    cfg = orc._cfg(dict(i_max=3))
    batch = orc.synthetic_batch(5, cfg=cfg, seed=13, regime="realistic")
    batch["interaction_freq"] = torch.from_numpy(np.random.default_rng(5).normal(0.0, 1.5, size=(5, 4, 4)).astype(np.float32))
    P = orc.init_params(cfg, 3, False)
    model = _model(cfg, B=7, seed=3)
    model.load_state_dict(P)
    div, info = contact.contact_dividends(model, *_args(batch), players="pcres_and_contacts")
    return cfg, batch, P, model, div, info


def test_joint_game_contact_is_null_next_to_its_deleted_slot(joint):
    cfg, batch, P, model, div, info = joint
    rows = info["coalitions"].cpu()
    assert rows.shape == (5, 64, 2) and info["players"] == ["pcre0", "pcre1", "pcre2", "contact0", "contact1", "contact2"]
    assert info["names"] == info["players"] and len(info["sets"]) == 64
    dummy = _dummies(batch)
    assert dummy.sum(1).tolist() == [0, 0, 0, 2, 3]
    differs = 0
    for j in range(3):
        for m in range(64):
            if m >> j & 1 or m >> (3 + j) & 1:
                continue
            assert torch.equal(rows[:, m], rows[:, m | 1 << (3 + j)]), (j, m)      # pcre j absent: the contact j bit changes nothing
            live = ~dummy[:, j]
            differs += int(not torch.equal(rows[live, m | 1 << j | 1 << (3 + j)], rows[live, m | 1 << j]))
    assert differs > 0
    div = div.cpu()
    for s in range(64):
        if any(s >> (3 + j) & 1 and not s >> j & 1 for j in range(3)):
            assert bool((div[:, s] == 0).all()), s
    assert bool((div[:3, 0b001001] != 0).all())      # {pcre0, contact0}: the contact acts through the live slot
    # every row is the forward on the edited batch, and the device table agrees with the oracle
    _rows_are_the_forward(model, batch, "pcres_and_contacts", [63, 0, 0b001001, 0b110101, 0b011110, 0b100011, 7, 56])
    from tests.contact_oracle import oracle_contact_coalitions
    drop, con, _ = _players("pcres_and_contacts", 3)
    d = (rows[:, :16] - oracle_contact_coalitions(P, batch, range(16), drop, con, 0.0, None, cfg)).abs().max().item()
    print("joint game, i_max 3: 16 rows vs the oracle %.3e" % d)
    assert d < TOL
    _check_phi(info["phi"], info, 6)


def _sti_gap_bound(v, P):
    """|info["delta"]| under sti, from the call's own table v (float64): the exact sum of the diagonal and the upper triangle IS
    v(N) - v(0), so the gap is rounding alone.  Off the diagonal an entry's terms pass at most three rounded subtractions, the weight's
    rounding, one product and at most 2^(P - 2) additions: gamma_n scale with n = 2^(P - 2) + 5, scale = sum_S w (|a| + |b| + |c| + |d|)
    (pair_index_fp64's second result); a diagonal entry is one subtraction: u scale.  The K = P (P + 1) / 2 entries' fp32 sum in any order
    adds gamma_K (sum |entry| + their errors); 4 u max |v| covers logits - absent and the final subtraction."""
    n = 2 ** (P - 2) + 5
    g = n * U / (1 - n * U)
    I, scale = pair_index_fp64(v, "sti")
    upper = np.triu(np.ones((P, P), dtype=bool))
    own = np.where(np.eye(P, dtype=bool)[None, :, :, None], U * scale, g * scale)[:, upper].sum(1)
    K = P * (P + 1) // 2
    return own + K * U / (1 - K * U) * (np.abs(I[:, upper]).sum(1) + own) + 4 * U * np.abs(v).max(1)


def _greedy_backward(v, target):
    """Plain Python on one gene's table v [2^P, n_out]: from everybody, each round removes the player whose removal leaves the largest
    s * v[target] (s = +1 where everybody >= nobody, else -1); ties go to the lowest player index."""
    P = len(v).bit_length() - 1
    full = (1 << P) - 1
    s = 1.0 if v[full][target] >= v[0][target] else -1.0
    cur, order = full, []
    for _ in range(P):
        best = None
        for p in range(P):
            if cur >> p & 1 and (best is None or s * float(v[cur ^ 1 << p][target]) > s * float(v[cur ^ 1 << best][target])):
                best = p
        order.append(best)
        cur ^= 1 << best
    return order


def test_joint_game_interactions_epistasis_and_backselect(joint):
    from chromoformer_amd import backselect, contact
    cfg, batch, P, model, div, info = joint
    table = info["coalitions"]
    kw = dict(players="pcres_and_contacts")
    sii, isii = contact.contact_shapley_interactions(model, *_args(batch), index="sii", return_coalitions=True, **kw)
    assert torch.equal(isii["coalitions"], table) and torch.equal(isii["phi"], info["phi"]) and isii["players"] == info["players"]
    diag = sii[:, torch.arange(6), torch.arange(6)]
    assert torch.equal(diag, info["phi"]) and torch.equal(sii, sii.transpose(1, 2))
    assert torch.equal(sii, model.shapley_interactions(table, index="sii"))
    sti, isti = contact.contact_shapley_interactions(model, *_args(batch), index="sti", **kw)
    assert torch.equal(sti, sti.transpose(1, 2)) and isti["index"] == "sti" and "erased" in isti
    gap, bound = np.abs(isti["delta"].cpu().numpy()), _sti_gap_bound(table.cpu().numpy().astype(np.float64), 6)
    print("sti delta: max %.3e, max bound %.3e" % (gap.max(), bound.max()))
    assert gap.shape == bound.shape and (gap <= bound).all()
    # epistasis: bit-equal to its definition on contact_coalitions' pair-deletion rows
    eps, ieps = contact.contact_epistasis(model, *_args(batch), **kw)
    rows = contact.contact_coalitions(model, *_args(batch), keep=pair_words(6), **kw).cpu()
    assert eps.shape == (5, 6, 6, 2) and torch.equal(eps.cpu(), torch.from_numpy(epistasis_fp32(rows.numpy())))
    assert torch.equal(eps, eps.transpose(1, 2)) and torch.equal(ieps["logits"].cpu(), rows[:, 0]) and torch.equal(ieps["single"].cpu(), rows[:, 1:7])
    # back-selection on the kept table, as it is
    order, binfo = backselect.backselect(model, table, names=info["players"])
    v = table.cpu().numpy()
    for b in range(5):
        assert order[b].tolist() == _greedy_backward(v[b], 1), b
    assert binfo["names"] == info["players"] and torch.equal(binfo["values"][:, 0], info["logits"]) and torch.equal(binfo["values"][:, 6], info["erased"])


def test_chunking_and_call_after_call(joint):
    from chromoformer_amd import contact
    cfg, batch, P, model7, div, info = joint
    sub = _take(batch, slice(1, 5))      # (max_batch 4 holds at most 4 genes)
    ref = info["coalitions"][1:5].cpu()
    donor = (batch["interaction_freq"][1:5] * -0.5 + 0.25).contiguous()
    runs = {}
    for cap in (4, 7, 64):
        model = _model(cfg, B=cap, seed=3)
        model.load_state_dict(P)
        phi, i1 = contact.contact_shapley(model, *_args(sub), players="pcres_and_contacts", return_coalitions=True)
        assert torch.equal(i1["coalitions"].cpu(), ref), cap
        d1 = contact.contact_shapley(model, *_args(sub), donor_freq=donor.cuda(), return_coalitions=True)
        model.pcre_shapley(*_args(sub))      # another attribution call in between: the one workspace, the word table
        model.mark_shapley(*_args(sub), players="regions")
        phi2, i2 = contact.contact_shapley(model, *_args(sub), players="pcres_and_contacts", return_coalitions=True)
        d2 = contact.contact_shapley(model, *_args(sub), donor_freq=donor.cuda(), return_coalitions=True)
        assert torch.equal(phi, phi2) and torch.equal(i1["coalitions"], i2["coalitions"]), cap
        assert torch.equal(d1[0], d2[0]) and torch.equal(d1[1]["coalitions"], d2[1]["coalitions"]), cap
        runs[cap] = (phi.cpu(), d1[0].cpu(), d1[1]["coalitions"].cpu())
    for cap in (7, 64):
        assert all(torch.equal(a, b) for a, b in zip(runs[4], runs[cap])), cap


def test_i_max_16():
    from chromoformer_amd import contact
    cfg = orc._cfg(dict(i_max=16))
    batch = _take(orc.synthetic_batch(2, cfg=cfg, seed=13, regime="realistic"), slice(0, 1))
    batch["interaction_freq"] = torch.from_numpy(np.random.default_rng(6).normal(0.0, 1.5, size=(1, 17, 17)).astype(np.float32))
    P = orc.init_params(cfg, 3, False)
    model = _model(cfg, B=256, seed=3)
    model.load_state_dict(P)
    words = [0xFFFF, 0, 0x00FF, 0xFF00, 0x8001, 0x5A5A, 0x0100, 0x7FFF, 0xFFFE, 0xA5A5, 0x0001, 0x8000]      # slots 8..15 in use
    got = _rows_are_the_forward(model, batch, "contacts", words, 0.0)
    _rows_are_the_forward(model, batch, "contacts", words[:6], 0.0, torch.roll(batch["interaction_freq"], 1, 2).contiguous())
    _rows_are_the_forward(model, batch, [([j], [15 - j]) for j in range(16)], words[:6], 2.0)      # drop and contact words differ per player
    phi, info = contact.contact_shapley(model, *_args(batch), return_coalitions=True)      # 65,536 rows in 256 chunks
    assert phi.shape == (1, 16, 2) and info["coalitions"].shape == (1, 65536, 2)
    assert bool(torch.isfinite(phi).all()) and bool(torch.isfinite(info["coalitions"]).all())
    assert torch.equal(info["coalitions"][0, words].cpu(), got[0])
    _check_phi(phi, info, 16)
    dummy = _dummies(batch)
    assert bool((~dummy).any()) and bool((phi.cpu()[dummy] == 0).all()) and bool((phi.cpu()[~dummy] != 0).any())
    with pytest.raises(ValueError, match="contact_players: .*i_max = 16 > 8.*'contacts'"):
        contact.contact_shapley(model, *_args(batch), players="pcres_and_contacts")


def test_a_layer_by_layer_regulation_shape():
    cfg = orc._cfg(dict(i_max=3, regulation=REG_4x128))
    batch = orc.synthetic_batch(5, cfg=cfg, seed=13, regime="realistic")
    batch["interaction_freq"] = torch.from_numpy(np.random.default_rng(7).normal(0.0, 1.5, size=(5, 4, 4)).astype(np.float32))
    model = _model(cfg, B=16, seed=3)      # (three chunks: 40 rows)
    model.load_state_dict(orc.init_params(cfg, 3, False))
    _rows_are_the_forward(model, batch, "pcres_and_contacts", [63, 0, 9, 0b110101, 0b011110, 0b100011, 7, 56], 0.0)
    _rows_are_the_forward(model, batch, "contacts", range(8), 0.0, (batch["interaction_freq"] * 0.5 - 1.0).contiguous())


def _opts(drop, con, scale=0.0, donor=None):
    from chromoformer_amd import _lib
    o = _lib.cf_contact_opts()
    d, c = np.ascontiguousarray(drop, dtype=np.uint32), np.ascontiguousarray(con, dtype=np.uint32)
    o.n_players, o.player_drop, o.player_contact, o.scale = len(d), d.ctypes.data, c.ctypes.data, scale
    o.donor_freq = None if donor is None else donor.data_ptr()
    return o, (d, c, donor)


@pytest.mark.parametrize("name,n_reg_head", [("default", 2), ("reg_4x128", 3 * 6 + 1)])
def test_launch_contract_and_refusals_at_the_c_abi(name, n_reg_head):
    """fwd = n_trunk + 1 + chunks x (1 + n_reg_head), with n_trunk + n_reg_head those of cf_forward(save = 0) -- the contract of
    cf_pcre_coalitions with the same n_coal --, plus 1 per reducer."""
    from chromoformer_amd import _lib, contact
    cfg = orc._cfg(None if name == "default" else dict(i_max=3, regulation=REG_4x128))
    S = cfg["i_max"]
    B, n_coal = 6, 10
    rng = np.random.RandomState(1)
    words = [int(w) for w in rng.randint(0, 1 << S, n_coal)]
    batch = orc.synthetic_batch(B, cfg=cfg, seed=23, regime="realistic")
    for chunks in (1, 3):
        cap = B * n_coal if chunks == 1 else (B * n_coal + 2) // 3
        model = _model(cfg, B=cap)
        with torch.no_grad():
            model(*_args(batch))
        n_inf = model.launch_counts()[0]
        model.pcre_coalitions(*_args(batch), keep=words)
        n_pcre = model.launch_counts()[0]
        out = contact.contact_coalitions(model, *_args(batch), keep=words)
        assert model.launch_counts()[0] == n_pcre == n_inf + 2 + (chunks - 1) * (1 + n_reg_head), (chunks, n_inf, n_pcre)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all())
        rows_of = lambda R: n_inf + 2 + (-(-B * R // cap) - 1) * (1 + n_reg_head)      # noqa: E731
        contact.contact_shapley(model, *_args(batch))
        assert model.launch_counts()[0] == rows_of(1 << S) + 1
        contact.contact_epistasis(model, *_args(batch))
        assert model.launch_counts()[0] == rows_of(1 + S + S * (S - 1) // 2) + 1
        contact.contact_shapley_interactions(model, *_args(batch))
        assert model.launch_counts()[0] == rows_of(1 << S) + 2      # k_shapley_pairs and k_shapley (the function asks for phi)
    # refusals by name, before anything is launched
    L = _lib.lib()
    small = _model(cfg, B=4)
    packed = model.pack_batch(batch)      # B = 6 > small's max_batch
    bs = C.byref(packed[0])
    st = torch.cuda.current_stream().cuda_stream
    out = torch.empty(B, max(n_coal, 1 << S), 2, device="cuda")
    keep = np.array(words, dtype=np.uint32)
    kp, op = keep.ctypes.data, out.data_ptr()
    drop, con, _ = _players("contacts", S)
    good, alive = _opts(drop, con)
    n0 = model.launch_counts()[0]

    def refused(rc, *needles):
        err = L.cf_last_error()
        assert rc != 0 and all(n in err for n in needles), err

    who = b"cf_contact_coalitions"
    refused(L.cf_contact_coalitions(small._handle, bs, C.byref(good), kp, n_coal, op, st), who, b"max_batch")
    refused(L.cf_contact_coalitions(None, bs, C.byref(good), kp, n_coal, op, st), who, b"null handle")
    refused(L.cf_contact_coalitions(model._handle, None, C.byref(good), kp, n_coal, op, st), who, b"null batch")
    refused(L.cf_contact_coalitions(model._handle, bs, None, kp, n_coal, op, st), who, b"null opts")
    refused(L.cf_contact_coalitions(model._handle, bs, C.byref(good), kp, n_coal, None, st), who, b"null logits")
    refused(L.cf_contact_coalitions(model._handle, bs, C.byref(good), kp, 0, op, st), who, b"n_coal")
    refused(L.cf_contact_coalitions(model._handle, bs, C.byref(good), None, n_coal, op, st), who, b"null keep")
    bad = keep.copy()
    bad[7] = 1 << S
    refused(L.cf_contact_coalitions(model._handle, bs, C.byref(good), bad.ctypes.data, n_coal, op, st), who, b"keep[7]", b"n_players")
    for o, needles in ((_opts([0] * 17, [1] * 17), (b"n_players = 17",)), (_opts([], []), (b"n_players = 0",)),
                       (_opts([1, 0], [0, 0]), (b"player_drop[1]", b"at least one")), (_opts([1 << S], [0]), (b"player_drop[0]", b"i_max")),
                       (_opts([0, 1], [1, 1 << S]), (b"player_contact[1]", b"i_max")), (_opts(drop, con, float("nan")), (b"scale",)),
                       (_opts(drop, con, float("inf")), (b"scale",))):
        refused(L.cf_contact_coalitions(model._handle, bs, C.byref(o[0]), kp, n_coal, op, st), who, *needles)
    null_arrays = _lib.cf_contact_opts()
    null_arrays.n_players = 2
    refused(L.cf_contact_coalitions(model._handle, bs, C.byref(null_arrays), kp, n_coal, op, st), who, b"null player_drop")
    one, alive1 = _opts([1], [1])
    for fn, nm in ((L.cf_contact_shapley, b"cf_contact_shapley"), (L.cf_contact_epistasis, b"cf_contact_epistasis")):
        refused(fn(small._handle, bs, C.byref(good), op, None, st), nm, b"max_batch")
        refused(fn(None, bs, C.byref(good), op, None, st), nm, b"null handle")
        refused(fn(model._handle, None, C.byref(good), op, None, st), nm, b"null batch")
        refused(fn(model._handle, bs, None, op, None, st), nm, b"null opts")
        refused(fn(model._handle, bs, C.byref(good), None, None, st), nm, b"null")
    refused(L.cf_contact_epistasis(model._handle, bs, C.byref(one), op, None, st), b"cf_contact_epistasis", b"at least 2")
    nm = b"cf_contact_shapley_interactions"
    refused(L.cf_contact_shapley_interactions(model._handle, bs, C.byref(one), 0, op, None, None, st), nm, b"at least 2")
    refused(L.cf_contact_shapley_interactions(model._handle, bs, C.byref(good), 0, None, None, None, st), nm, b"null inter")
    refused(L.cf_contact_shapley_interactions(model._handle, bs, C.byref(good), 7, op, None, None, st), nm, b"index")
    refused(L.cf_contact_shapley_interactions(model._handle, bs, None, 0, op, None, None, st), nm, b"null opts")
    assert model.launch_counts()[0] == n0      # nothing was launched
    # the packed forms (pack_batch, engine.Slot) give the same result as the six tensors
    from chromoformer_amd.engine import Slot
    ref = contact.contact_coalitions(model, *_args(batch), keep=words, scale=0.5).cpu()
    eps_ref = contact.contact_epistasis(model, *_args(batch), scale=0.5)[0].cpu()
    phi_ref = contact.contact_shapley(model, *_args(batch), scale=0.5)[0]
    slot = Slot(model, B).fill(model, batch)
    for p in (packed, slot):
        assert torch.equal(contact.contact_coalitions(model, p, keep=words, scale=0.5).cpu(), ref)
        assert torch.equal(contact.contact_epistasis(model, p, scale=0.5)[0].cpu(), eps_ref)
    # without a caller's row buffer the rows go to the handle-owned one: the same values
    half, alive2 = _opts(drop, con, 0.5)
    eps2 = torch.empty_like(eps_ref, device="cuda")
    assert L.cf_contact_epistasis(model._handle, bs, C.byref(half), eps2.data_ptr(), None, st) == 0, L.cf_last_error()
    phi2 = torch.empty_like(phi_ref)
    assert L.cf_contact_shapley(model._handle, bs, C.byref(half), phi2.data_ptr(), None, st) == 0, L.cf_last_error()
    inter2, phi3 = torch.empty(B, S, S, 2, device="cuda"), torch.empty_like(phi_ref)
    assert L.cf_contact_shapley_interactions(model._handle, bs, C.byref(half), 0, inter2.data_ptr(), phi3.data_ptr(), None, st) == 0, L.cf_last_error()
    torch.cuda.synchronize()
    assert torch.equal(eps2.cpu(), eps_ref) and torch.equal(phi2, phi_ref) and torch.equal(phi3, phi_ref)
    assert torch.equal(inter2, contact.contact_shapley_interactions(model, packed, scale=0.5)[0])


def test_no_side_effects_on_training_and_a_stale_backward_is_refused():
    from chromoformer_amd import contact
    from chromoformer_amd.engine import Trainer
    batches = [orc.synthetic_batch(8, seed=41 + i, regime="realistic") for i in range(4)]

    def run(interpose):
        model = _model(B=8)
        tr = Trainer(model, lr=1e-3)
        slots = [tr.stage(b) for b in batches[:3]]
        tr.step(slots[0])
        if interpose:
            torch.cuda.synchronize()
            contact.contact_shapley(model, *_args(batches[3]), players="pcres_and_contacts")
            contact.contact_epistasis(model, *_args(batches[3]), donor_freq=batches[2]["interaction_freq"].cuda())
            contact.contact_shapley_interactions(model, *_args(batches[3]), scale=2.0)
            torch.cuda.synchronize()
        tr.step(slots[1])
        tr.step(slots[2])      # two training steps afterwards
        torch.cuda.synchronize()
        sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        sd["<exp_avg>"], sd["<exp_avg_sq>"] = model._mflat.cpu().clone(), model._vflat.cpu().clone()
        return sd

    ref, got = run(False), run(True)
    assert all(torch.equal(ref[k], got[k]) for k in ref)

    model = _model(B=8)
    b = batches[0]
    with torch.enable_grad():
        for fn, kw in ((contact.contact_shapley, {}), (contact.contact_epistasis, {}), (contact.contact_coalitions, dict(keep=[255, 0])),
                       (contact.contact_shapley_interactions, {}), (contact.contact_dividends, {})):
            out = model(*_args(b))
            res = fn(model, *_args(batches[1]), **kw)
            assert not (res if torch.is_tensor(res) else res[0]).requires_grad
            with pytest.raises(RuntimeError, match="contact_"):
                out[:, 1].sum().backward()
        model(*_args(b))[:, 1].sum().backward()      # a fresh forward trains as before
    assert float(model._gflat.abs().sum()) > 0


def test_dataset_generator_and_cli(tmp_path):
    import pandas as pd

    from chromoformer_amd import ChromoformerClassifier, contact, predict
    from chromoformer_amd.data import ChromoformerDataset
    from tests import donor_oracle as do
    from tests.synth_data import make_dataset
    npy, dnpy = str(tmp_path / "npy"), str(tmp_path / "donor")
    meta = make_dataset(npy, n_genes=12, seed=11)
    do.donor_dataset(npy, dnpy, do.DONOR_SEED, w_prom=40000)
    dmeta = os.path.join(dnpy, "meta.csv")
    frame = pd.read_csv(dmeta)      # the donor cell type's own contact frequencies: the same regions, other scores
    frame["scores"] = [s if pd.isna(s) else ";".join("%.4f" % (4.5 - float(x) + 0.125 * k) for k, x in enumerate(str(s).split(";")))
                       for s in frame["scores"]]
    frame.to_csv(dmeta, index=False)
    genes = frame.gene_id.tolist()
    ds, dn = ChromoformerDataset(meta, npy, genes), ChromoformerDataset(dmeta, dnpy, genes)
    P = orc.init_params(seed=7)
    ck = str(tmp_path / "w.pt")
    torch.save({"net": P}, ck)
    model = ChromoformerClassifier(seed=123, max_batch=32).cuda(0)
    model.load_state_dict(P)
    n_pcres = np.array([min(len(ds.genes[g]["pcres"]), 8) for g in genes])
    assert (n_pcres > 0).any() and (n_pcres < 8).any()
    # the generator: the scale rule, in chunks of 5 genes
    res = list(contact.contact_shapley_dataset(model, ds, genes=genes, scale=0.5, epistasis=True, interactions="sii", dividends=True, bsz=5))
    assert [r["gene_id"] for r in res] == genes
    for i, r in enumerate(res):
        assert sorted(r) == ["dividends", "eps", "erased", "freq", "gene_id", "interactions", "logits", "mass", "pcres", "phi", "players"]
        assert r["players"] == ["contact%d" % j for j in range(8)] and r["phi"].shape == (8, 2) and r["phi"].dtype == np.float32
        assert r["eps"].shape == r["interactions"].shape == (8, 8, 2) and r["dividends"].shape == r["mass"].shape == (256, 2)
        assert r["freq"].shape == (8,) and len(r["pcres"]) == n_pcres[i] and (r["freq"][:n_pcres[i]] > 0).all() and (r["freq"][n_pcres[i]:] == 0).all()
        assert (r["phi"][n_pcres[i]:] == 0).all() and (r["phi"][:n_pcres[i]] != 0).all()
        assert np.array_equal(r["interactions"][np.arange(8), np.arange(8)], r["phi"])
    # against the donor's frequencies, on the gene's own features and on the donor's
    own = list(contact.contact_shapley_dataset(model, ds, dn, genes=genes, bsz=5))
    swap = list(contact.contact_shapley_dataset(model, ds, dn, genes=genes, marks="donor", bsz=5))
    marks = list(model.mark_donor_shapley_dataset(ds, dn, genes=genes, bsz=5))
    plain = {r["gene_id"]: r for r in res}
    for i, (a, b, m) in enumerate(zip(own, swap, marks)):
        assert sorted(a) == sorted(b) == ["donor", "donor_freq", "freq", "gene_id", "logits", "pcres", "phi", "players"]
        assert np.array_equal(a["logits"], plain[a["gene_id"]]["logits"]) and np.array_equal(a["freq"], plain[a["gene_id"]]["freq"])
        assert a["donor_freq"].shape == (8,) and (a["donor_freq"][:n_pcres[i]] != a["freq"][:n_pcres[i]]).all()
        assert np.array_equal(b["logits"], m["donor"]), i                 # the donor's marks under the gene's masks and frequencies
        assert np.array_equal(b["donor"], m["donor_prediction"]), i       # every contact the donor's too: the donor dataset's own forward
        whole = m["logits"].astype(np.float64) - m["donor_prediction"]      # the two games together account for the whole difference
        parts = m["phi"].astype(np.float64).sum(0) + b["phi"].astype(np.float64).sum(0)
        assert np.abs(parts - whole).max() < 1e-5, (i, parts, whole)
        assert (a["phi"][n_pcres[i]:] == 0).all() and (n_pcres[i] == 0 or (a["phi"][:n_pcres[i]] != 0).any())
    with pytest.raises(ValueError, match="contact_players"):
        next(contact.contact_shapley_dataset(model, ds, genes=genes, players="genes"))
    with pytest.raises(ValueError, match="marks='donor' needs a donor_dataset"):
        next(contact.contact_shapley_dataset(model, ds, genes=genes, marks="donor"))
    # the command line: the writer's one generator run over all 12 genes, bit for bit
    res32 = list(contact.contact_shapley_dataset(model, ds, genes=genes, scale=0.5, interactions="sii", dividends=True))
    swap32 = list(contact.contact_shapley_dataset(model, ds, dn, genes=genes, marks="donor"))
    out, iout, dout, ddout = (str(tmp_path / n) for n in ("c.npz", "ci.npy", "cd.npz", "cdonor.npz"))
    base = ["-m", meta, "-d", npy, "-w", ck, "-o", str(tmp_path / "p.csv")]
    assert predict.main(base + ["--contact-shapley-out", out, "--contact-scale", "0.5", "--contact-interactions-out", iout,
                                "--contact-dividends-out", dout, "--interaction-index", "sii", "--donor-npy-dir", dnpy, "--donor-meta", dmeta,
                                "--contact-donor-shapley-out", ddout, "--contact-donor-marks", "donor"]) == 0
    z = np.load(out)
    assert sorted(z.files) == ["erased", "freq", "gene_ids", "logits", "n_pcres", "phi", "players"]
    assert list(z["gene_ids"]) == genes and list(z["players"]) == ["contact%d" % j for j in range(8)]
    assert z["phi"].shape == (12, 8) and z["phi"].dtype == np.float32 and z["logits"].shape == z["erased"].shape == (12,) and z["freq"].shape == (12, 8)
    assert np.array_equal(z["n_pcres"], n_pcres)
    assert np.array_equal(z["phi"], np.stack([r["phi"][:, 1] for r in res32])) and np.array_equal(z["logits"], np.array([r["logits"][1] for r in res32]))
    assert np.array_equal(z["erased"], np.array([r["erased"][1] for r in res32])) and np.array_equal(z["freq"], np.stack([r["freq"] for r in res32]))
    inter = np.load(iout)
    assert inter.shape == (12, 8, 8) and inter.dtype == np.float32 and np.array_equal(inter, inter.transpose(0, 2, 1))
    assert np.array_equal(inter[:, np.arange(8), np.arange(8)], z["phi"])
    zd = np.load(dout)
    assert sorted(zd.files) == ["dividends", "gene_ids", "mass", "players", "sets"] and zd["dividends"].shape == zd["mass"].shape == (12, 256)
    assert np.array_equal(zd["dividends"][:, 0], z["erased"]) and len(zd["sets"]) == 256 and list(zd["players"]) == list(z["players"])
    assert np.array_equal(zd["dividends"], np.stack([r["dividends"][:, 1] for r in res32]))
    zz = np.load(ddout)
    assert sorted(zz.files) == ["donor", "donor_freq", "freq", "gene_ids", "logits", "marks", "n_pcres", "phi", "players"]
    assert str(zz["marks"]) == "donor" and zz["phi"].shape == (12, 8) and zz["donor_freq"].shape == (12, 8)
    assert np.array_equal(zz["phi"], np.stack([r["phi"][:, 1] for r in swap32])) and np.array_equal(zz["donor"], np.array([r["donor"][1] for r in swap32]))
    sig = torch.sigmoid(torch.from_numpy(z["logits"])).numpy()
    assert np.abs(sig - pd.read_csv(str(tmp_path / "p.csv"))["prediction"].to_numpy()).max() <= 2.0 ** -23
    for extra in (["--contact-scale", "2"], ["--contact-donor-shapley-out", ddout], ["--contact-shapley-out", out, "--contact-donor-marks", "donor"]):
        with pytest.raises(SystemExit) as e:
            predict.main(base + extra)
        assert e.value.code == 2
