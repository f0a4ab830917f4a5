"""Wide histone-mark coalitions and permutation-sampled Shapley values on the GPU (cf_mark_coalitions_wide / cf_mark_shapley_sampled,
the ChromoformerBase methods mark_coalitions_wide / mark_shapley_sampled, attribution.mark_shapley_sampled, predict
--mark-sampled-shapley-out / --mark-donor-sampled-shapley-out).

  * the bits of a wide row: with at most 16 players those of the one-word kernels on the same words; with one player per (mark, region)
    pair (63 players, two words; 119 players, four words) the plain forward on the batch with the gone columns zeroed, or taken from the
    donor;
  * the sampled rows: nobody, everybody, every prefix of every order, bit for bit;
  * phi and stderr against float64 on the call's own rows within a rounding bound derived below, the efficiency gap, null players exactly
    0; with all P! orders the exact Shapley values of mark_shapley / mark_donor_shapley;
  * the same bits whatever max_batch is and call after call; other model shapes; the launch contract and every refusal by name; no side
    effects on training; the dataset generator and the CLI.

No test here depends on sampling luck: the estimator's arithmetic is pinned on the rows the call returns; how close the estimate is to
the exact value is reported by stderr and not asserted.

The rounding bound of phi.  k_perm_shapley forms d_q by one fp32 subtraction, sums the n = n_perm values with n - 1 additions (some
order) and divides once: n + 1 rounded operations, so with u = 2^-24 and gamma(k) = k u / (1 - k u)
    |phi - mean64(d_q)| <= gamma(n + 1) mean_q |d_q|                                                         (B_phi)
(the test rebuilds d_q with numpy's fp32 subtraction, which is the device's, so the subtraction's own error is slack).  stderr: e_q =
fl(d_q - phi) (1 operation, entering squared: 2), the square (1), n - 1 additions, the rounding of n (n - 1), the division and the
square root (3 more, halved by the root but counted whole) are at most n + 6 relative errors on se, and the error of phi moves every
e_q by at most B_phi, the root mean square by at most B_phi / sqrt(n - 1):
    |se - se64| <= gamma(n + 6) se64 + 1.001 B_phi / sqrt(n - 1)                                             (B_se)
info["delta"] = sum_p phi - (v_N - v_0) in fp32: within P max_p B_phi + 4 u max|v|, the form of the exact game's tests."""
import ctypes as C
import itertools
import os

import numpy as np
import pandas as pd
import pytest
import torch

from chromoformer_amd import _lib
from chromoformer_amd.attribution import mark_players_wide, mark_wide_words, shapley_permutations
from oracle import chromoformer_oracle as orc
from tests import donor_oracle as do
from tests import mark_oracle as mo
from tests import perm_oracle as po
from tests import scan_oracle as so
from tests.coalition_oracle import shapley_fp64
from tests.test_input_grads_gpu import _model
from tests.test_mark_coalitions_gpu import GENES, OVERLAP, SHAPES, _zeroed
from tests.test_mark_donor_gpu import _dev, _feats, _selected
from tests.test_pcre_coalitions_gpu import U, _gamma

pytestmark = pytest.mark.gpu
ALL = tuple(range(7))
SEED = 5
THREE = [(ALL, (0,)), (ALL, (1,)), (ALL, (8,))]      # the promoter, pCRE slot 0, pCRE slot 7 (a dummy slot of the third gene)


def _args(batch):
    return tuple(batch[k] for k in so.KEYS)


def _plain(model, batch):
    with torch.no_grad():
        return model(*_args(batch)).cpu()


def _g(k):
    return k * U / (1 - k * U)


def _host(info):
    return {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in info.items()}


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """-> (the three genes' batch, the donor cell type's batch), both on the device: built once, never written."""
    ds = so.scan_dataset(str(tmp_path_factory.mktemp("marks")), w_prom=39000)
    dn = do.donor_dataset(ds.npy_dir, str(tmp_path_factory.mktemp("donor")), do.DONOR_SEED, w_prom=39000)
    return _dev(so.dataset_batch(ds, GENES)), _dev(so.dataset_batch(dn, GENES))


@pytest.fixture(scope="module")
def small():
    """The seed-42 classifier (the golden's weights) at max_batch = 4."""
    return _model(None, False, orc.init_params(None, 42, False), 4)


@pytest.fixture(scope="module")
def wide64():
    """The same classifier at max_batch = 64."""
    return _model(None, False, orc.init_params(None, 42, False), 64)


@pytest.fixture(scope="module")
def cells2(data, small):
    """(phi, info) of small.mark_shapley_sampled, one player per (mark, region) pair, two orders, s = 0: 3 x 126 rows in 95 chunks."""
    phi, info = small.mark_shapley_sampled(*_args(data[0]), players="cells", n_perm=2, seed=SEED, return_rows=True)
    torch.cuda.synchronize()
    return phi.cpu(), _host(info)


@pytest.fixture(scope="module")
def cells2_donor(data, small):
    """The same against the donor cell type."""
    phi, info = small.mark_shapley_sampled(*_args(data[0]), players="cells", n_perm=2, seed=SEED, donor=_feats(data[1]), return_rows=True)
    torch.cuda.synchronize()
    return phi.cpu(), _host(info)


def _reference(model, batch, donor, players, word, T=9):
    """The plain forward on the batch with the gone columns of coalition `word` zeroed (donor None) or taken from the donor."""
    gone = mo.gone_words(players[0], players[1], word, T)
    return _plain(model, _zeroed(batch, gone) if donor is None else _selected(batch, donor, gone))


def _cell_words(P=63, dummy=range(56, 63)):
    """The full word, the empty word, players 31 and 32 alone absent (the two sides of a word boundary), the players of one region alone
    absent (pCRE slot 7: a dummy slot of the third gene), six seeded random words."""
    full = (1 << P) - 1
    rng = np.random.default_rng(17)
    rand = [int("".join("1" if x else "0" for x in rng.random(P) < 0.5), 2) for _ in range(6)]
    return [full, 0, full & ~(1 << 31) & ~(1 << 32), full & ~sum(1 << p for p in dummy)] + rand


def test_at_most_16_players_carry_the_bits_of_the_one_word_kernels(data, small):
    batch, donor = data
    cases = [("marks", [0x7F, 0x00, 0x7F & ~(1 << 3), 0x25]), ("regions", [0x1FF & ~1, 0x001, 0x0AA]), (OVERLAP, [0b00, 0b01, 0b10, 0b11])]
    for spec, words in cases:
        for s in (0.0, 2.5):
            got = small.mark_coalitions_wide(*_args(batch), keep=words, players=spec, scale=s).cpu()
            ref = small.mark_coalitions(*_args(batch), keep=words, players=spec, scale=s).cpu()
            assert got.shape == (3, len(words), 2) and not got.requires_grad and torch.equal(got, ref), (spec, s)
        got = small.mark_coalitions_wide(*_args(batch), keep=words, players=spec, donor=_feats(donor), scale=-1.0).cpu()      # (scale is not read)
        ref = small.mark_donor_coalitions(*_args(batch), keep=words, players=spec, donor=_feats(donor)).cpu()
        assert torch.equal(got, ref), spec
        assert not torch.equal(got, small.mark_coalitions(*_args(batch), keep=words, players=spec).cpu())      # the donor's marks are not zeros


@pytest.mark.parametrize("rule", ["scale", "donor"])
def test_cells_rows_are_the_plain_forward_bit_for_bit(data, small, rule):
    batch = data[0]
    donor = data[1] if rule == "donor" else None
    players = mark_players_wide("cells", 7, 8)
    words = _cell_words()
    kw = dict(donor=_feats(donor)) if donor is not None else {}
    got = small.mark_coalitions_wide(*_args(batch), keep=words, **kw).cpu()      # players="cells", scale=0.0: the defaults
    base = _plain(small, batch)
    assert got.shape == (3, 10, 2) and torch.equal(got[:, 0], base)
    for c, m in enumerate(words):
        assert torch.equal(got[:, c], _reference(small, batch, donor, players, m)), (rule, c, hex(m))
    assert not torch.equal(got[:, 1], base) and len({tuple(got[0, c].tolist()) for c in range(10)}) >= 8
    assert torch.equal(got[2, 3], base[2])      # a dummy slot's players change nothing
    bits = np.array([[bool(m >> p & 1) for p in range(63)] for m in words])
    assert torch.equal(small.mark_coalitions_wide(*_args(batch), keep=bits, **kw).cpu(), got)
    assert torch.equal(small.mark_coalitions_wide(small.pack_batch(batch), keep=words, **kw).cpu(), got)


@pytest.mark.parametrize("rule", ["scale", "donor"])
def test_rows_at_the_ends_of_a_coalition_word(data, small, rule):
    """One kernel pair builds the rows of the one-word and of the wide entry points from kw = ceil(P / 32) words: the player counts at
    which kw or the word index of the last player changes.  The players are the first P of "cells" (31: mark 3 in pCRE slot 3, 32: mark 4
    there); 1 and 16 players through the one-word calls, 32 and 33 through the wide one."""
    batch = data[0]
    donor = data[1] if rule == "donor" else None
    cells = [((f,), (rho,)) for rho in range(9) for f in range(7)]
    base = _plain(small, batch)
    for P, absent in ((1, [(0,)]), (16, [(15,), tuple(range(15)), (0, 5, 9)]), (32, [(31,), tuple(range(31)), (0,)]),
                      (33, [(32,), (31,), tuple(range(32)), (31, 32)])):
        spec = cells[:P]
        players = mark_players_wide(spec, 7, 8)
        full = (1 << P) - 1
        words = [full, 0] + [full & ~sum(1 << p for p in gone) for gone in absent]
        if P > 16:
            got = small.mark_coalitions_wide(*_args(batch), keep=words, players=spec, **(dict(donor=_feats(donor)) if donor is not None else {}))
        elif donor is None:
            got = small.mark_coalitions(*_args(batch), keep=words, players=spec)
        else:
            got = small.mark_donor_coalitions(*_args(batch), keep=words, players=spec, donor=_feats(donor))
        got = got.cpu()
        assert got.shape == (3, len(words), 2) and torch.equal(got[:, 0], base), (rule, P)
        for c, m in enumerate(words):
            assert torch.equal(got[:, c], _reference(small, batch, donor, players, m)), (rule, P, c, hex(m))
        assert not torch.equal(got[:, 2], base), (rule, P)      # the last player alone absent changes a row
        if P == 33:      # ... and is not taken for its neighbour across the word boundary
            assert not torch.equal(got[:, 3], base) and not torch.equal(got[:, 2], got[:, 3]), rule


@pytest.mark.parametrize("rule", ["scale", "donor"])
def test_119_players_in_four_words(rule):
    cfg = orc._cfg(SHAPES["i_max16"][0])
    batch = _dev(orc.synthetic_batch(2, cfg=cfg, seed=13, regime="realistic"))
    donor = _dev(orc.synthetic_batch(2, cfg=cfg, seed=14, regime="realistic")) if rule == "donor" else None
    model = _model(cfg, False, orc.init_params(cfg, 3, False), 5)
    players = mark_players_wide("cells", 7, 16)
    assert len(players[0]) == 119
    full = (1 << 119) - 1
    words = [full, full & ~sum(1 << p for p in (63, 64, 95, 96, 118)), 0, full & ~(1 << 118), 1 << 96]
    kw = dict(donor=_feats(donor)) if donor is not None else {}
    got = model.mark_coalitions_wide(*_args(batch), keep=words, **kw).cpu()
    assert got.shape == (2, 5, 2) and torch.equal(got[:, 0], _plain(model, batch))
    for c, m in enumerate(words):
        assert torch.equal(got[:, c], _reference(model, batch, donor, players, m, 17)), (rule, c)
    assert len({tuple(got[:, c].reshape(-1).tolist()) for c in range(5)}) >= 3      # (a word that differs in a dummy slot alone repeats a row)


@pytest.mark.parametrize("rule", ["scale", "donor"])
def test_sampled_rows_are_the_prefix_coalitions_bit_for_bit(data, small, cells2, cells2_donor, rule):
    batch = data[0]
    donor = data[1] if rule == "donor" else None
    phi, info = cells2 if donor is None else cells2_donor
    players = mark_players_wide("cells", 7, 8)
    perms, rows = info["permutations"], info["rows"]
    assert perms.dtype == np.uint8 and perms.shape == (2, 63) and np.array_equal(perms, shapley_permutations(63, 2, SEED))
    assert rows.shape == (3, 2 + 2 * 62, 2) and phi.shape == info["stderr"].shape == (3, 63, 2) and not phi.requires_grad
    assert info["names"] == players[2] and info["names"][8] == "mark1@pcre0"
    base = _plain(small, batch)
    assert torch.equal(rows[:, 1], base) and torch.equal(info["logits"], base)
    assert torch.equal(rows[:, 0], _reference(small, batch, donor, players, 0)) and torch.equal(info["absent"], rows[:, 0])
    if donor is not None:      # nobody present: the donor's features under the gene's masks and frequencies
        assert torch.equal(rows[:, 0], _plain(small, dict(batch, promoter_feats=donor["promoter_feats"], pcre_feats=donor["pcre_feats"])))
    words = po.prefix_words(perms)      # the test's own prefix words, from the orders the call reports
    assert words[2] == 1 << int(perms[0, 0]) and bin(words[2 + 61]).count("1") == 62 and not words[2 + 61] >> int(perms[0, 62]) & 1
    kw = dict(donor=_feats(donor)) if donor is not None else {}
    got = small.mark_coalitions_wide(*_args(batch), keep=words, **kw).cpu()
    assert got.shape == rows.shape and torch.equal(got, rows)
    assert len({tuple(rows[0, c].tolist()) for c in range(2, 64)}) > 7      # the prefixes differ (a dummy slot's players add nothing)


def _check_estimate(phi, info, null=None):
    """phi, stderr and delta of a call against float64 on its own rows, within B_phi, B_se and the delta bound of the module docstring;
    null: a bool [B, P] of players that must be exactly 0 (the others of the gene's non-null set are free)."""
    perms = info["permutations"]
    n, P = perms.shape
    v = info["rows"].cpu().numpy()
    d = po.marginals(v, perms, np.float32)      # the device's one fp32 subtraction
    phi64, se64 = po.estimate_fp64(d)
    b_phi = _g(n + 1) * np.abs(d.astype(np.float64)).mean(1)
    err = np.abs(phi.cpu().numpy().astype(np.float64) - phi64)
    print("phi: n_perm %d, P %d: max err %.3e, max bound %.3e" % (n, P, err.max(), b_phi.max()))
    assert (err <= b_phi).all(), (err.max(), b_phi.max())
    se = info["stderr"].cpu().numpy().astype(np.float64)
    if n == 1:
        assert (se == 0).all()
    else:
        b_se = _g(n + 6) * se64 + 1.001 * b_phi / np.sqrt(n - 1)
        err = np.abs(se - se64)
        print("stderr: max err %.3e, max bound %.3e, max se %.3e" % (err.max(), b_se.max(), se64.max()))
        assert (err <= b_se).all(), (err.max(), b_se.max())
    dbound = P * b_phi.max(1) + 4 * U * np.abs(v).max(1)
    delta = np.abs(info["delta"].cpu().numpy())
    print("delta: max %.3e, max bound %.3e" % (delta.max(), dbound.max()))
    assert delta.shape == dbound.shape and (delta <= dbound).all(), (delta.max(), dbound.max())
    assert torch.equal(info["logits"].cpu(), info["rows"][:, 1].cpu()) and torch.equal(info["absent"].cpu(), info["rows"][:, 0].cpu())
    if null is not None:
        p, s = phi.cpu().numpy(), info["stderr"].cpu().numpy()
        assert (p[null] == 0).all() and (s[null] == 0).all()
    return phi64


@pytest.mark.parametrize("rule", ["scale", "donor"])
def test_phi_stderr_delta_and_null_players(data, cells2, cells2_donor, rule):
    phi, info = cells2 if rule == "scale" else cells2_donor
    null = np.zeros((3, 63), dtype=bool)
    null[2, 7:] = True      # the third gene has no partners: every pCRE slot is a dummy, in both cell types
    _check_estimate(phi, info, null)
    assert bool((phi[2, :7] != 0).all()) and bool((phi[:2] != 0).any(-1).any(-1).all())
    assert bool((info["stderr"][:2] > 0).any())
    cells = phi.view(3, 9, 7, 2)      # [B, region, mark, n_out]
    assert torch.equal(cells[:, 1, 3], phi[:, 10])


def test_a_donor_aliasing_the_batch_makes_every_player_null(data, wide64):
    batch = data[0]
    base = _plain(wide64, batch)
    phi, info = wide64.mark_shapley_sampled(*_args(batch), players="cells", n_perm=2, seed=1, donor=_feats(batch), return_rows=True)
    assert torch.equal(info["rows"].cpu(), base[:, None].expand(3, 126, 2))
    assert bool((phi == 0).all()) and bool((info["stderr"] == 0).all()) and bool((info["delta"] == 0).all())
    packed = wide64.pack_batch(batch)      # the donor's pointers ARE the batch's
    phi, info = wide64.mark_shapley_sampled(packed, donor=packed, n_perm=1)
    assert bool((phi == 0).all()) and bool((info["stderr"] == 0).all())


def test_all_orders_give_the_exact_shapley_values(data, small):
    """Three explicit players, all 3! = 6 orders: the estimator IS the Shapley value.  Both kernels work on the same row bits (the rows
    are deterministic), so the two results differ by their rounding alone: B_phi of the docstring plus the exact game's
    _gamma(3) sum_m w |difference| (tests/test_pcre_coalitions_gpu.py)."""
    batch, donor = data
    every = np.array(list(itertools.permutations(range(3))), dtype=np.uint8)
    for kw, exact in ((dict(scale=0.0), lambda: small.mark_shapley(*_args(batch), players=THREE, return_coalitions=True)),
                      (dict(scale=2.5), lambda: small.mark_shapley(*_args(batch), players=THREE, scale=2.5, return_coalitions=True)),
                      (dict(donor=_feats(donor)), lambda: small.mark_donor_shapley(*_args(batch), donor=_feats(donor), players=THREE, return_coalitions=True))):
        phi, info = small.mark_shapley_sampled(*_args(batch), players=THREE, permutations=every, return_rows=True, **kw)
        ref, rinfo = exact()
        table = rinfo["coalitions"].cpu()
        assert np.array_equal(info["permutations"], every) and info["rows"].shape == (3, 2 + 6 * 2, 2)
        assert torch.equal(info["rows"].cpu(), table[:, [int(m) for m in po.prefix_words(every)]])      # the same row bits
        _check_estimate(phi, info)
        d = po.marginals(info["rows"].cpu().numpy(), every, np.float32)
        bound = _g(6 + 1) * np.abs(d.astype(np.float64)).mean(1) + _gamma(3) * shapley_fp64(table.numpy())[1]
        err = np.abs(phi.cpu().numpy().astype(np.float64) - ref.cpu().numpy().astype(np.float64))
        print("exactness %s: max err %.3e, max bound %.3e" % (sorted(kw), err.max(), bound.max()))
        assert (err <= bound).all(), (err.max(), bound.max())
        assert bool((phi[2, 1:] == 0).all()) and bool((phi[:, 0] != 0).all())      # the third gene's pCRE players are null


def test_same_bits_for_every_max_batch_and_call_after_call(data, cells2, cells2_donor, wide64):
    batch, donor = data
    for cap in (7, 64):
        model = wide64 if cap == 64 else _model(None, False, orc.init_params(None, 42, False), cap)
        for (phi, info), kw in ((cells2, {}), (cells2_donor, dict(donor=_feats(donor)))):
            p, i = model.mark_shapley_sampled(*_args(batch), players="cells", n_perm=2, seed=SEED, return_rows=True, **kw)
            assert torch.equal(p.cpu(), phi) and torch.equal(i["stderr"].cpu(), info["stderr"]) and torch.equal(i["rows"].cpu(), info["rows"]), cap
            assert torch.equal(i["delta"].cpu(), info["delta"])
    again, info2 = wide64.mark_shapley_sampled(*_args(batch), players="cells", n_perm=2, seed=SEED, return_rows=True)
    assert torch.equal(again.cpu(), cells2[0]) and torch.equal(info2["rows"].cpu(), cells2[1]["rows"])
    other = wide64.mark_shapley_sampled(*_args(batch), players="cells", n_perm=2, seed=SEED + 1)[0]
    assert not torch.equal(other.cpu(), cells2[0])      # other orders, another estimate
    given = wide64.mark_shapley_sampled(wide64.pack_batch(batch), permutations=torch.from_numpy(cells2[1]["permutations"].astype(np.int64)))[0]
    assert torch.equal(given.cpu(), cells2[0])


@pytest.mark.parametrize("name", ["d_emb_64", "embed_2_layers", "reg_layer_by_layer", "regressor"])
def test_other_shapes(name):
    """One order of the 63 cells on two genes (128 rows in chunks of 5): the end rows and a few prefixes against the plain forward on the
    zeroed columns, the estimate against float64."""
    over, regression = SHAPES[name]
    cfg = orc._cfg(over)
    batch = _dev(orc.synthetic_batch(2, cfg=cfg, seed=13, regime="realistic"))
    if name == "embed_2_layers":      # the reference's full [B, 1, L, L] promoter mask: the chunk rows carry all L rows
        assert all(m.numel() == 2 * L * L for m, L in zip(batch["promoter_pad_masks"].values(), (20, 80, 400)))
    model = _model(cfg, regression, orc.init_params(cfg, 3, regression), 5)
    players = mark_players_wide("cells", 7, 8)
    phi, info = model.mark_shapley_sampled(*_args(batch), n_perm=1, seed=2, return_rows=True)
    rows = info["rows"].cpu()
    assert rows.shape == (2, 64, 1 if regression else 2) and phi.shape == (2, 63, rows.shape[-1])
    words = po.prefix_words(info["permutations"])
    for c in (0, 1, 2, 31, 32, 33, 63):
        assert torch.equal(rows[:, c], _reference(model, batch, None, players, words[c])), (name, c)
    _check_estimate(phi, info)
    assert bool((phi != 0).any())


@pytest.mark.parametrize("cap", [64, 7])
def test_launch_contract(data, cap, wide64):
    """fwd = ceil(B n_coal / max_batch) (1 + n_fwd), n_fwd those of cf_forward(save = 0); the sampled call runs R = 2 + n_perm (P - 1)
    rows per gene and adds its reducer."""
    batch, donor = data
    model = wide64 if cap == 64 else _model(None, False, orc.init_params(None, 42, False), cap)
    _plain(model, batch)
    n_fwd = model.launch_counts()[0]
    chunks = lambda rows: -(-rows // cap)      # noqa: E731
    model.mark_coalitions_wide(*_args(batch), keep=_cell_words())
    assert model.launch_counts()[0] == chunks(3 * 10) * (1 + n_fwd)
    model.mark_coalitions_wide(*_args(batch), keep=[0, 5], players="regions", donor=_feats(donor))
    assert model.launch_counts()[0] == chunks(3 * 2) * (1 + n_fwd)
    model.mark_shapley_sampled(*_args(batch), players="regions", n_perm=3)
    assert model.launch_counts()[0] == chunks(3 * (2 + 3 * 8)) * (1 + n_fwd) + 1
    model.mark_shapley_sampled(*_args(batch), players="cells", n_perm=1, donor=_feats(donor))
    assert model.launch_counts()[0] == chunks(3 * 64) * (1 + n_fwd) + 1
    model.mark_shapley_sampled(*_args(batch), players=[(ALL, (0,))], n_perm=4)      # one player: the two end rows alone
    assert model.launch_counts()[0] == chunks(3 * 2) * (1 + n_fwd) + 1


def test_null_stderr_and_the_handle_owned_rows_through_the_c_abi(data, small):
    """se and logits_rows are optional: without them the rows go to the handle-owned buffer and phi carries the same bits."""
    batch = data[0]
    L = _lib.lib()
    bs, keep_alive = small.pack_batch(batch)
    st = torch.cuda.current_stream().cuda_stream
    pm, pr, _ = mark_players_wide("cells", 7, 8)
    perms = shapley_permutations(63, 2, SEED)
    o = _lib.cf_mark_wide_opts()
    o.n_players, o.scale, o.player_marks, o.player_regions = 63, 0.0, pm.ctypes.data, pr.ctypes.data
    ref, info = small.mark_shapley_sampled((bs, keep_alive), n_perm=2, seed=SEED)
    n_launch = small.launch_counts()[0]
    phi = torch.full((3, 63, 2), float("nan"), device="cuda")
    se = torch.full((3, 63, 2), float("nan"), device="cuda")
    assert L.cf_mark_shapley_sampled(small._handle, C.byref(bs), C.byref(o), perms.ctypes.data, 2, phi.data_ptr(), None, None, st) == 0, L.cf_last_error()
    assert torch.equal(phi, ref) and small.launch_counts()[0] == n_launch
    phi.fill_(float("nan"))
    assert L.cf_mark_shapley_sampled(small._handle, C.byref(bs), C.byref(o), perms.ctypes.data, 2, phi.data_ptr(), se.data_ptr(), None, st) == 0, L.cf_last_error()
    assert torch.equal(phi, ref) and torch.equal(se, info["stderr"])
    del keep_alive


def test_refusals_by_name_with_nothing_launched(data):
    batch, donor = data
    L = _lib.lib()
    model = _model(None, False, orc.init_params(None, 42, False), 4)
    bs, keep_alive = model.pack_batch(batch)
    dbs, donor_alive = model.pack_batch(donor)
    _plain(model, batch)
    f0 = model.launch_counts()
    st = torch.cuda.current_stream().cuda_stream
    out = torch.full((3, 128, 2), float("nan"), device="cuda")
    pm, pr, _ = mark_players_wide("cells", 7, 8)
    words = mark_wide_words([0, 1, (1 << 63) - 1, 1 << 62], 63)
    perms = shapley_permutations(63, 2, 0)
    big = _lib.cf_batch.from_buffer_copy(bs)
    big.B = 5

    def opts(n_players=63, marks=pm, regions=pr, scale=0.0, don_p=(None,) * 3, don_c=(None,) * 3):
        o = _lib.cf_mark_wide_opts()
        o.n_players, o.scale = n_players, scale
        o.player_marks = marks.ctypes.data if marks is not None else None
        o.player_regions = regions.ctypes.data if regions is not None else None
        for r in range(3):
            o.donor_promoter_feats[r], o.donor_pcre_feats[r] = don_p[r], don_c[r]
        return o

    def edited(a, p, v):
        a = a.copy()
        a[p] = v
        return a

    dp, dc = tuple(dbs.promoter_feats[r] for r in range(3)), tuple(dbs.pcre_feats[r] for r in range(3))
    many = np.ones(129, dtype=np.uint32)
    bad_opts = [(dict(n_players=0), b"n_players = 0 outside 1..128"), (dict(n_players=129, marks=many, regions=many), b"n_players = 129 outside 1..128"),
                (dict(marks=None), b"null player_marks"), (dict(regions=None), b"null player_marks / player_regions"),
                (dict(marks=edited(pm, 40, 0)), b"player_marks[40] = 0"), (dict(regions=edited(pr, 62, 0)), b"player_regions[62] = 0"),
                (dict(marks=edited(pm, 1, 0x80)), b"n_feats"), (dict(regions=edited(pr, 6, 0x200)), b"i_max"),
                (dict(scale=-0.5), b"scale"), (dict(scale=float("inf")), b"scale"), (dict(scale=float("nan")), b"scale"),
                (dict(don_p=dp), b"donor_promoter_feats / donor_pcre_feats"), (dict(don_p=dp, don_c=(dc[0], None, dc[2])), b"donor_promoter_feats / donor_pcre_feats"),
                (dict(don_c=(None, dc[1], None)), b"are null")]
    entries = [(b"cf_mark_coalitions_wide", lambda h, b, o, dst: L.cf_mark_coalitions_wide(h, b, o, words.ctypes.data, 4, dst, st)),
               (b"cf_mark_shapley_sampled", lambda h, b, o, dst: L.cf_mark_shapley_sampled(h, b, o, perms.ctypes.data, 2, dst, None, None, st))]

    def refused(rc, *needles):
        err = L.cf_last_error()
        assert rc != 0 and all(n in err for n in needles), err

    for name, fn in entries:
        good = opts()
        refused(fn(None, C.byref(bs), C.byref(good), out.data_ptr()), name, b"null handle")
        refused(fn(model._handle, None, C.byref(good), out.data_ptr()), name, b"null batch")
        refused(fn(model._handle, C.byref(bs), None, out.data_ptr()), name, b"null opts")
        refused(fn(model._handle, C.byref(bs), C.byref(good), None), name, b"null logits" if b"wide" in name else b"null phi")
        refused(fn(model._handle, C.byref(big), C.byref(good), out.data_ptr()), name, b"max_batch")
        for kw, msg in bad_opts:
            refused(fn(model._handle, C.byref(bs), C.byref(opts(**kw)), out.data_ptr()), name, msg)
    good = opts()
    name = b"cf_mark_coalitions_wide"
    refused(L.cf_mark_coalitions_wide(model._handle, C.byref(bs), C.byref(good), None, 4, out.data_ptr(), st), name, b"null keep")
    refused(L.cf_mark_coalitions_wide(model._handle, C.byref(bs), C.byref(good), words.ctypes.data, 0, out.data_ptr(), st), name, b"n_coal")
    bad = words.copy()
    bad[3, 1] |= 1 << 31      # player 63 of 63
    refused(L.cf_mark_coalitions_wide(model._handle, C.byref(bs), C.byref(good), bad.ctypes.data, 4, out.data_ptr(), st), name, b"keep[3]", b"n_players = 63")
    name = b"cf_mark_shapley_sampled"
    refused(L.cf_mark_shapley_sampled(model._handle, C.byref(bs), C.byref(good), None, 2, out.data_ptr(), None, None, st), name, b"null perms")
    refused(L.cf_mark_shapley_sampled(model._handle, C.byref(bs), C.byref(good), perms.ctypes.data, 0, out.data_ptr(), None, None, st), name, b"n_perm = 0")
    twice = perms.copy()
    twice[1, 5] = twice[1, 6]      # a repeated player
    refused(L.cf_mark_shapley_sampled(model._handle, C.byref(bs), C.byref(good), twice.ctypes.data, 2, out.data_ptr(), None, None, st), name, b"perms[1]", b"not a permutation")
    high = perms.copy()
    high[0, 0] = 63                # a player >= P
    refused(L.cf_mark_shapley_sampled(model._handle, C.byref(bs), C.byref(good), high.ctypes.data, 2, out.data_ptr(), None, None, st), name, b"perms[0]", b"not a permutation")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and model.launch_counts() == f0      # nothing was launched
    # the donor rule does not read the scale
    assert L.cf_mark_coalitions_wide(model._handle, C.byref(bs), C.byref(opts(scale=-1.0, don_p=dp, don_c=dc)), words.ctypes.data, 1, out.data_ptr(), st) == 0, L.cf_last_error()
    out.fill_(float("nan"))
    # armed riders (a training step in flight): refused; the handle is not used again
    assert L.cf_rider_arm(model._handle, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, 0, 8) == 0, L.cf_last_error()
    for name, fn in entries:
        refused(fn(model._handle, C.byref(bs), C.byref(good), out.data_ptr()), name, b"riders")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    for kw in (dict(players="genes"), dict(players=[((7,), (0,))]), dict(keep=[1 << 63]), dict(keep=[-1])):      # (raised before the library is called)
        with pytest.raises(ValueError, match="mark_players_wide|mark_coalitions_wide"):
            model.mark_coalitions_wide((bs, keep_alive), **dict(dict(keep=[0]), **kw))
    with pytest.raises(ValueError, match="keep is required"):
        model.mark_coalitions_wide((bs, keep_alive))
    for permutations in (np.zeros((2, 62), dtype=np.int64), np.full((1, 63), 63), np.zeros((0, 63), dtype=np.int64), np.zeros((1, 63))):
        with pytest.raises(ValueError, match="mark_shapley_sampled: permutations"):
            model.mark_shapley_sampled((bs, keep_alive), permutations=permutations)
    with pytest.raises(ValueError, match="shapley_permutations"):
        model.mark_shapley_sampled((bs, keep_alive), n_perm=0)
    with pytest.raises(ValueError, match="mark_shapley_sampled: the donor holds"):
        model.mark_shapley_sampled((bs, keep_alive), donor=big)
    del keep_alive, donor_alive


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
            model.mark_shapley_sampled(*_args(dev), players="regions", n_perm=2, scale=2.0)
            model.mark_shapley_sampled(*_args(dev), players="compartments", n_perm=1, donor=_feats(_dev(batches[1])))
            model.mark_coalitions_wide(*_args(dev), keep=[0, 1 << 40])
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
        for method, kw in (("mark_shapley_sampled", dict(players="regions", n_perm=1)), ("mark_coalitions_wide", dict(keep=[0]))):
            out = model(*_args(b))
            res = getattr(model, method)(*_args(b), **kw)
            assert not (res if torch.is_tensor(res) else res[0]).requires_grad
            with pytest.raises(RuntimeError, match=method):
                out[:, 1].sum().backward()
        model(*_args(b))[:, 1].sum().backward()      # a fresh forward trains as before
    assert float(model._gflat.abs().sum()) > 0


def _subset(ds, genes):
    import copy
    sub = copy.copy(ds)
    sub.target_genes = list(genes)
    return sub


def test_dataset_generator_and_cli(tmp_path):
    from chromoformer_amd import ChromoformerClassifier, predict
    from chromoformer_amd.data import ChromoformerDataset, GeneStore
    from tests.synth_data import make_dataset
    npy, dnpy = str(tmp_path / "npy"), str(tmp_path / "donor")
    meta = make_dataset(npy, n_genes=20, seed=11)
    dn = do.donor_dataset(npy, dnpy, do.DONOR_SEED, w_prom=40000)
    genes = pd.read_csv(meta).gene_id.tolist()
    P = orc.init_params(seed=7)
    ck = str(tmp_path / "w.pt")
    torch.save({"net": P}, ck)
    out, dout = str(tmp_path / "sampled.npz"), str(tmp_path / "sampled_donor.npz")
    assert predict.main(["-m", meta, "-d", npy, "-w", ck, "-o", str(tmp_path / "p.csv"), "--mark-sampled-shapley-out", out, "--mark-perms", "2",
                         "--mark-seed", "9", "--mark-scale", "0.5", "--donor-npy-dir", dnpy, "--mark-donor-sampled-shapley-out", dout]) == 0
    ds = ChromoformerDataset(meta, npy, genes)
    model = ChromoformerClassifier(seed=123, max_batch=32).cuda(0)
    model.load_state_dict(P)
    store, dstore = GeneStore(ds, device=model._device, resident=True), GeneStore(dn, device=model._device, resident=True)
    d, dd = store.batch(list(range(20))), dstore.batch(list(range(20)))
    names = mark_players_wide("cells", 7, 8)[2]
    n_pcres = np.array([min(len(ds.genes[g]["pcres"]), 8) for g in genes])
    for path, kw in ((out, dict(scale=0.5)), (dout, dict(donor=_feats(dd)))):
        z = np.load(path)
        assert sorted(z.files) == ["absent", "gene_ids", "logits", "permutations", "phi", "players", "stderr"]
        assert list(z["gene_ids"]) == genes and list(z["players"]) == names
        assert np.array_equal(z["permutations"], shapley_permutations(63, 2, 9))
        assert z["phi"].shape == z["stderr"].shape == (20, 63) and z["phi"].dtype == np.float32 and z["logits"].shape == z["absent"].shape == (20,)
        # the per-batch call on the stores predict() builds: the same bits
        phi, info = model.mark_shapley_sampled(*_args(d), n_perm=2, seed=9, return_rows=True, **kw)
        _check_estimate(phi, info)
        assert np.array_equal(z["phi"], phi.cpu()[..., 1].numpy()) and np.array_equal(z["stderr"], info["stderr"].cpu()[..., 1].numpy())
        assert np.array_equal(z["logits"], info["logits"].cpu()[:, 1].numpy()) and np.array_equal(z["absent"], info["absent"].cpu()[:, 1].numpy())
        cells = z["phi"].reshape(20, 9, 7)
        for i in range(20):      # a dummy slot's players are null players
            assert (cells[i, 1 + n_pcres[i]:] == 0).all() and (cells[i, :1 + n_pcres[i]] != 0).any(), i
    sig = torch.sigmoid(torch.from_numpy(np.load(out)["logits"])).numpy()
    assert np.abs(sig - pd.read_csv(str(tmp_path / "p.csv"))["prediction"].to_numpy()).max() <= 2.0 ** -23
    # the generator, in chunks of 7 genes: the per-batch calls' bits, with and without the donor
    sub = genes[3:13]
    for donor_ds in (None, dn):
        res = list(model.mark_shapley_sampled_dataset(ds, donor_ds, genes=sub, players="regions", n_perm=3, seed=4, scale=0.25, bsz=7))
        assert [r["gene_id"] for r in res] == sub
        src = GeneStore(_subset(ds, sub), device=model._device, resident=True)
        dsrc = GeneStore(_subset(dn, sub), device=model._device, resident=True) if donor_ds is not None else None
        for lo in (0, 7):
            n = min(7, 10 - lo)
            b = src.batch(list(range(lo, lo + n)))
            kw = dict(donor=_feats(dsrc.batch(list(range(lo, lo + n))))) if dsrc is not None else dict(scale=0.25)
            phi, info = model.mark_shapley_sampled(*_args(b), players="regions", n_perm=3, seed=4, **kw)
            for i in range(n):
                r = res[lo + i]
                assert sorted(r) == ["absent", "gene_id", "logits", "permutations", "phi", "players", "stderr"]
                assert r["players"] == ["promoter"] + ["pcre%d" % j for j in range(8)] and np.array_equal(r["permutations"], shapley_permutations(9, 3, 4))
                assert r["phi"].shape == r["stderr"].shape == (9, 2) and r["phi"].dtype == np.float32
                assert np.array_equal(r["phi"], phi[i].cpu().numpy()) and np.array_equal(r["stderr"], info["stderr"][i].cpu().numpy())
                assert np.array_equal(r["logits"], info["logits"][i].cpu().numpy()) and np.array_equal(r["absent"], info["absent"][i].cpu().numpy())
    with pytest.raises(ValueError, match="mark_players_wide"):
        next(model.mark_shapley_sampled_dataset(ds, genes=sub, players="genes"))
    far = ChromoformerDataset(os.path.join(dnpy, "meta.csv"), dnpy, genes, w_prom=38000)
    with pytest.raises(ValueError, match="same_regions: .*w_prom"):
        next(model.mark_shapley_sampled_dataset(ds, far, genes=sub))
