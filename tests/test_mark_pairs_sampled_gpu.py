"""Sampled pairwise Shapley interaction indices of focal players on the GPU (cf_mark_shapley_interactions_sampled and its window / fine
siblings, cf_perm_interactions_from_rows, the ChromoformerBase methods mark_shapley_interactions_sampled /
mark_window_shapley_interactions_sampled / mark_fine_window_shapley_interactions_sampled / perm_interactions_from_rows,
attribution.mark_shapley_interactions_sampled, predict --mark-sampled-interactions-out).

No test here depends on sampling luck: the estimator's arithmetic is pinned on the rows the call returns (bit for bit against
tests/focal_oracle.focal_pairs_fp32, and within a derived rounding bound of float64); how close the estimate is to the exact index is
reported by stderr and asserted only where all P! orders make the estimate the index itself.

The rounding bound of inter.  k_perm_pairs rebuilds the sample s_q from the rows (three fp32 subtractions, for "sti" one product: the
test rebuilds them with numpy's fp32 operations, which are the device's, so these cost nothing), sums the n = n_perm samples with n - 1
additions in some order and divides once: n rounded operations; one more is slack, so that the form is the sibling's.  With u = 2^-24
and gamma(k) = k u / (1 - k u)
    |inter - mean64(s_q)| <= gamma(n + 1) mean_q |s_q|                                                       (B)
stderr: e_q = fl(s_q - inter) (1 operation, entering squared: 2), the square (1), n - 1 additions, the rounding of n (n - 1), the
division and the square root (3 more, halved by the root but counted whole) are at most n + 6 relative errors on se, and the error of
inter moves every e_q by at most B, the root mean square by at most B / sqrt(n - 1):
    |se - se64| <= gamma(n + 6) se64 + 1.001 B / sqrt(n - 1)                                                 (B_se)
-- tests/test_mark_sampled_gpu.py's bounds with s_q in the place of d_q.  info["delta"] ("sii") = sum_{j != i} inter - ((v_N - v_{N-i})
- (v_i - v_0)) in fp32: the marginals M_k = fl(v(T_k + i) - v(T_k)) are the same floats in d(o[k - 1]) and d(o[k]), so per order the
sum of the exact differences M_{a+1} - M_a telescopes to M_{P-1} - M_0, which the reference forms from the same two floats with one more
subtraction: within P max_j B + 8 u max|v|."""
import ctypes as C
import itertools

import numpy as np
import pandas as pd
import pytest
import torch

from chromoformer_amd import _lib
from chromoformer_amd.attribution import focal_row_count, focal_words, mark_players_wide, shapley_permutations
from oracle import chromoformer_oracle as orc
from tests import donor_oracle as do
from tests import focal_oracle as fo
from tests import scan_oracle as so
from tests.interaction_oracle import pair_index_fp64
from tests.test_input_grads_gpu import _model
from tests.test_mark_coalitions_gpu import GENES
from tests.test_mark_donor_gpu import _dev, _feats

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
ALL = tuple(range(7))
SEED = 5
FOCAL = (31, 60)      # mark 3 in pCRE slot 3 (the last player of the first word); mark 4 in pCRE slot 7, a dummy slot of the third gene
FOUR = [(ALL, (0,)), (ALL, (1,)), (ALL, (8,)), (ALL, (2,))]      # the promoter, pCRE 0, pCRE 7, the marks of pCRE 1
EVERY4 = np.array(list(itertools.permutations(range(4))), dtype=np.uint8)


def _args(batch):
    return tuple(batch[k] for k in so.KEYS)


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
def wide64():
    """The seed-42 classifier (the golden's weights) at max_batch = 64."""
    return _model(None, False, orc.init_params(None, 42, False), 64)


@pytest.fixture(scope="module")
def cells(data, wide64):
    """{index: (inter, info)} of wide64.mark_shapley_interactions_sampled, the 63 cells, two orders, focal = FOCAL, s = 0: 370 rows per
    gene."""
    out = {}
    for index in ("sii", "sti"):
        inter, info = wide64.mark_shapley_interactions_sampled(*_args(data[0]), players="cells", focal=FOCAL, index=index, n_perm=2, seed=SEED,
                                                               return_rows=True)
        torch.cuda.synchronize()
        out[index] = (inter.cpu(), _host(info))
    return out


def _check_estimate(inter, se, rows, perms, focal, index, col=None):
    """inter and se against the kernel's arithmetic in numpy (bit for bit) and against float64 on the same fp32 samples within B and
    B_se of the module docstring -> B [B, n_focal, P, n_out]."""
    rows = np.asarray(rows)
    n = len(perms)
    ref, ref_se = fo.focal_pairs_fp32(rows, perms, focal, index, col)
    inter, se = np.asarray(inter), np.asarray(se)
    assert inter.dtype == np.float32 and inter.shape == ref.shape and se.shape == ref.shape
    assert np.array_equal(inter.view(np.uint32), ref.view(np.uint32)), np.abs(inter - ref).max()
    off = np.ones(se.shape, dtype=bool)
    if index == "sii":      # the "sii" diagonal takes k_perm_shapley's approximate square root, for that kernel's bits: pinned to them by the callers
        off[:, np.arange(len(focal)), [int(i) for i in focal]] = False
    assert np.array_equal(se.view(np.uint32)[off], ref_se.view(np.uint32)[off]), np.abs(se - ref_se).max()
    s = fo.focal_samples(rows, perms, focal, index, np.float32, col)
    mean64, se64 = fo.focal_estimate_fp64(s)
    bound = _g(n + 1) * np.abs(s.astype(np.float64)).mean(1)
    err = np.abs(inter.astype(np.float64) - mean64)
    print("inter %s: n_perm %d, P %d: max err %.3e, max bound %.3e" % (index, n, perms.shape[1], err.max(), bound.max()))
    assert (err <= bound).all(), (err.max(), bound.max())
    if n == 1:
        assert (se == 0).all()
    else:
        b_se = _g(n + 6) * se64 + 1.001 * bound / np.sqrt(n - 1)
        err = np.abs(se.astype(np.float64) - se64)
        print("stderr %s: max err %.3e, max bound %.3e, max se %.3e" % (index, err.max(), b_se.max(), se64.max()))
        assert (err <= b_se).all(), (err.max(), b_se.max())
    return bound


@pytest.mark.parametrize("n_perm", [1, 255, 256, 257])
@pytest.mark.parametrize("P", [2, 3, 32, 33, 128])
def test_the_operator_on_synthetic_tables(wide64, P, n_perm):
    """cf_perm_interactions_from_rows on random tables (no forward runs): the players at the ends of a coalition word, the order counts
    around the thread stride (one order; one short of, exactly and one past kShapThreads = 256), both indices, one and two outputs."""
    focal = sorted({p for p in (0, 31, 32, P - 1) if p < P}, reverse=True)
    perms = shapley_permutations(P, n_perm, 100 * P + n_perm)
    col = fo.focal_words(perms, focal, want_words=False)[1]
    R = fo.n_rows(perms, focal)
    rng = np.random.default_rng(P + n_perm)
    for n_out, index in ((1, "sii"), (2, "sti"), (2, "sii"), (1, "sti")):
        rows = rng.standard_normal((2, R, n_out)).astype(np.float32)
        inter, se, phi, phi_se = wide64.perm_interactions_from_rows(torch.from_numpy(rows).cuda(), perms, focal, index)
        assert wide64.launch_counts()[0] == 2      # k_perm_pairs and k_perm_shapley
        inter, se, phi, phi_se = (t.cpu().numpy() for t in (inter, se, phi, phi_se))
        assert inter.shape == se.shape == (2, len(focal), P, n_out) and phi.shape == phi_se.shape == (2, P, n_out)
        _check_estimate(inter, se, rows, perms, focal, index, col)
        for f, i in enumerate(focal):      # the "sii" diagonal carries k_perm_shapley's bits on the leading rows
            if index == "sii":
                assert np.array_equal(inter[:, f, i], phi[:, i]) and np.array_equal(se[:, f, i], phi_se[:, i])
            else:
                assert np.array_equal(inter[:, f, i], rows[:, col[f, 0, 0, 1]] - rows[:, 0]) and (se[:, f, i] == 0).all()
        assert (inter != 0).all()


def test_cells_rows_phi_and_the_leading_block(data, wide64, cells):
    batch = data[0]
    inter, info = cells["sii"]
    perms, rows = info["permutations"], info["rows"]
    names = mark_players_wide("cells", 7, 8)[2]
    assert np.array_equal(perms, shapley_permutations(63, 2, SEED)) and info["names"] == names and info["focal"].tolist() == list(FOCAL)
    assert rows.shape == (3, 370, 2) and inter.shape == info["stderr"].shape == (3, 2, 63, 2) and not inter.requires_grad
    words, col = focal_words(perms, FOCAL)
    assert len(words) == 370 and np.array_equal(info["col"], col) and max(m.bit_length() for m in words) == 63      # two words per coalition
    got = wide64.mark_coalitions_wide(*_args(batch), keep=words).cpu()
    assert torch.equal(got, rows)
    phi, pinfo = wide64.mark_shapley_sampled(*_args(batch), players="cells", permutations=perms, return_rows=True)
    assert torch.equal(pinfo["rows"].cpu(), rows[:, :126]) and torch.equal(phi.cpu(), info["phi"]) and torch.equal(pinfo["stderr"].cpu(), info["phi_stderr"])
    assert torch.equal(info["logits"], rows[:, 1]) and torch.equal(info["absent"], rows[:, 0])
    at = [focal_row_count(perms, FOCAL[:f]) for f in range(2)]
    assert [words[a] for a in at] == [1 << 31, 1 << 60]
    assert torch.equal(info["alone"], rows[:, at]) and torch.equal(info["without"], rows[:, [a + 1 for a in at]])
    for f, i in enumerate(FOCAL):      # the "sii" diagonal is phi
        assert torch.equal(inter[:, f, i], info["phi"][:, i]) and torch.equal(info["stderr"][:, f, i], info["phi_stderr"][:, i])
    sti, sinfo = cells["sti"]
    assert torch.equal(sinfo["rows"], rows) and sinfo["delta"] is None and sinfo["index"] == "sti"
    for f, i in enumerate(FOCAL):
        assert torch.equal(sti[:, f, i], rows[:, at[f]] - rows[:, 0]) and bool((sinfo["stderr"][:, f, i] == 0).all())


@pytest.mark.parametrize("index", ["sii", "sti"])
def test_cells_estimate_bounds_and_exact_zeros(wide64, cells, index):
    inter, info = cells[index]
    rows, perms = info["rows"], info["permutations"]
    op = wide64.perm_interactions_from_rows(rows.cuda(), perms, FOCAL, index)
    assert torch.equal(op[0].cpu(), inter) and torch.equal(op[1].cpu(), info["stderr"])
    assert torch.equal(op[2].cpu(), info["phi"]) and torch.equal(op[3].cpu(), info["phi_stderr"])
    bound = _check_estimate(inter.numpy(), info["stderr"].numpy(), rows.numpy(), perms, FOCAL, index)
    if index == "sii":
        dbound = 63 * bound.max(2) + 8 * U * np.abs(rows.numpy()).max(1)[:, None]
        delta = np.abs(info["delta"].numpy())
        print("delta: max %.3e, max bound %.3e" % (delta.max(), dbound.max()))
        assert delta.shape == dbound.shape == (3, 2, 2) and (delta <= dbound).all(), (delta.max(), dbound.max())
    # the third gene has no partners: every pCRE slot is a dummy -- focal player 60 is null, and so is every partner j in slot 7
    assert bool((inter[2, 1] == 0).all()) and bool((info["stderr"][2, 1] == 0).all())
    assert bool((inter[2, 0, 56:63] == 0).all()) and bool((info["stderr"][2, 0, 56:63] == 0).all())
    assert bool((inter[:2, 0] != 0).any(-1).all()) and bool((inter[0, 1] != 0).any())      # (live players are not zeros)


def test_the_donor_rule(data, wide64, cells):
    batch, donor = data
    perms = cells["sii"][1]["permutations"]
    inter, info = wide64.mark_shapley_interactions_sampled(*_args(batch), players="cells", focal=["mark3@pcre3", "mark4@pcre7"], permutations=perms,
                                                           donor=_feats(donor), scale=-1.0, return_rows=True)      # (scale is not read)
    assert info["focal"].tolist() == list(FOCAL)
    rows = info["rows"].cpu()
    words = focal_words(perms, FOCAL)[0]
    assert torch.equal(wide64.mark_coalitions_wide(*_args(batch), keep=words, donor=_feats(donor)).cpu(), rows)
    assert not torch.equal(rows, cells["sii"][1]["rows"])      # the donor's marks are not zeros
    _check_estimate(inter.cpu().numpy(), info["stderr"].cpu().numpy(), rows.numpy(), perms, FOCAL, "sii")
    assert bool((inter[2, 1] == 0).all()) and bool((inter[2, 0, 56:63] == 0).all())


@pytest.fixture(scope="module")
def four(data, wide64):
    """{index: (inter, info)} of the four-player game with all 24 orders and all four players focal: 226 rows per gene."""
    out = {}
    for index in ("sii", "sti"):
        inter, info = wide64.mark_shapley_interactions_sampled(*_args(data[0]), players=FOUR, focal=range(4), index=index, permutations=EVERY4,
                                                               return_rows=True)
        out[index] = (inter.cpu(), _host(info))
    return out


@pytest.mark.parametrize("index", ["sii", "sti"])
def test_all_orders_give_the_exact_index(data, wide64, four, index):
    """All 4! orders: the estimator IS the index.  The call's rows carry the bits of the 2^4 coalition rows (the rows are
    deterministic), so in float64 the two agree to the rounding of float64 itself: 1e-12 of the index's scale."""
    inter, info = four[index]
    rows = info["rows"].numpy()
    assert rows.shape == (3, 226, 2)
    table = wide64.mark_coalitions_wide(*_args(data[0]), keep=list(range(16)), players=FOUR).cpu().numpy()
    words = focal_words(EVERY4, range(4))[0]
    assert np.array_equal(rows, table[:, words])
    est, _ = fo.focal_estimate_fp64(fo.focal_samples(rows, EVERY4, range(4), index, np.float64))
    ref, scale = pair_index_fp64(table, index)
    err = np.abs(est - ref)
    print("exactness %s: max err %.3e, max scale %.3e" % (index, err.max(), scale.max()))
    assert (err <= 1e-12 * scale).all(), err.max()
    _check_estimate(inter.numpy(), info["stderr"].numpy(), rows, EVERY4, range(4), index)
    assert bool((inter[2, 1:] == 0).all()) and bool((inter[2, 0, 1:] == 0).all())      # the third gene's pCRE players are null


def test_same_bits_for_every_max_batch_and_call_after_call(data, wide64, four):
    batch = data[0]
    keys = ("stderr", "phi", "phi_stderr", "rows", "delta", "alone", "without")
    for cap in (4, 7, 64):
        model = wide64 if cap == 64 else _model(None, False, orc.init_params(None, 42, False), cap)
        inter, info = model.mark_shapley_interactions_sampled(*_args(batch), players=FOUR, focal=range(4), permutations=EVERY4, return_rows=True)
        assert torch.equal(inter.cpu(), four["sii"][0]), cap
        for k in keys:
            assert torch.equal(info[k].cpu(), four["sii"][1][k]), (cap, k)
    packed = wide64.pack_batch(batch)
    inter, info = wide64.mark_shapley_interactions_sampled(packed, players=FOUR, focal=[3, 1], index="sti", permutations=torch.from_numpy(EVERY4.astype(np.int64)))
    assert "rows" not in info and inter.shape == (3, 2, 4, 2)
    sub = four["sti"][0][:, [3, 1]]      # a focal player's rows do not depend on the other focal players
    assert torch.equal(inter.cpu(), sub)


def test_window_and_fine_games(data, wide64):
    batch = data[0]
    perms = shapley_permutations(3, 3, 2)
    inter, info = wide64.mark_window_shapley_interactions_sampled(*_args(batch), players="promoter", width=8, focal=[2, 0], permutations=perms,
                                                                  return_rows=True)
    words, col = focal_words(perms, [2, 0])
    assert len(info["names"]) == 3 and info["rows"].shape == (3, len(words), 2)
    assert torch.equal(wide64.mark_window_coalitions(*_args(batch), keep=words, players="promoter", width=8), info["rows"])
    phi, pinfo = wide64.mark_window_shapley_sampled(*_args(batch), players="promoter", width=8, permutations=perms)
    assert torch.equal(phi, info["phi"]) and torch.equal(pinfo["stderr"], info["phi_stderr"])
    op = wide64.perm_interactions_from_rows(info["rows"], perms, [2, 0])
    assert torch.equal(op[0], inter) and torch.equal(op[1], info["stderr"])
    _check_estimate(inter.cpu().numpy(), info["stderr"].cpu().numpy(), info["rows"].cpu().numpy(), perms, [2, 0], "sii")
    assert bool((inter != 0).any())
    perms = shapley_permutations(4, 3, 3)
    kw = dict(region=0, players="windows", width=100, n_windows=4, start=0)
    inter, info = wide64.mark_fine_window_shapley_interactions_sampled(*_args(batch), focal=[1, 3], index="sti", permutations=perms, return_rows=True, **kw)
    words, col = focal_words(perms, [1, 3])
    assert len(info["names"]) == 4 and info["rows"].shape == (3, len(words), 2)
    assert torch.equal(wide64.mark_fine_window_coalitions(*_args(batch), keep=words, **kw), info["rows"])
    phi, pinfo = wide64.mark_fine_window_shapley_sampled(*_args(batch), permutations=perms, **kw)
    assert torch.equal(phi, info["phi"]) and torch.equal(pinfo["stderr"], info["phi_stderr"])
    op = wide64.perm_interactions_from_rows(info["rows"], perms, [1, 3], "sti")
    assert torch.equal(op[0], inter) and torch.equal(op[1], info["stderr"])
    _check_estimate(inter.cpu().numpy(), info["stderr"].cpu().numpy(), info["rows"].cpu().numpy(), perms, [1, 3], "sti")
    assert bool((inter != 0).any())


@pytest.mark.parametrize("cap", [64, 7])
def test_launch_contract(data, cap, wide64):
    """fwd = ceil(B R / max_batch) (1 + n_fwd), n_fwd those of cf_forward(save = 0), plus k_perm_pairs, plus k_perm_shapley if phi is
    asked for (the Python methods always ask)."""
    batch, donor = data
    model = wide64 if cap == 64 else _model(None, False, orc.init_params(None, 42, False), cap)
    with torch.no_grad():
        model(*_args(batch))
    n_fwd = model.launch_counts()[0]
    chunks = lambda rows: -(-rows // cap)      # noqa: E731
    perms = shapley_permutations(9, 3, 1)
    R = len(focal_words(perms, [0, 4])[0])
    model.mark_shapley_interactions_sampled(*_args(batch), players="regions", focal=[0, 4], permutations=perms)
    assert model.launch_counts()[0] == chunks(3 * R) * (1 + n_fwd) + 2
    model.mark_shapley_interactions_sampled(*_args(batch), players="regions", focal=[0, 4], permutations=perms, donor=_feats(donor), index="sti")
    assert model.launch_counts()[0] == chunks(3 * R) * (1 + n_fwd) + 2
    # through the C ABI without phi, se and logits_rows: one launch less, the same bits
    ref, info = model.mark_shapley_interactions_sampled(*_args(batch), players="regions", focal=[0, 4], permutations=perms)
    L = _lib.lib()
    bs, keep_alive = model.pack_batch(batch)
    pm, pr, _ = mark_players_wide("regions", 7, 8)
    o = _lib.cf_mark_wide_opts()
    o.n_players, o.scale, o.player_marks, o.player_regions = 9, 0.0, pm.ctypes.data, pr.ctypes.data
    focal = np.array([0, 4], dtype=np.int32)
    inter = torch.full((3, 2, 9, 2), float("nan"), device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    assert L.cf_mark_shapley_interactions_sampled(model._handle, C.byref(bs), C.byref(o), perms.ctypes.data, 3, focal.ctypes.data, 2, 0, inter.data_ptr(),
                                                  None, None, None, None, st) == 0, L.cf_last_error()
    assert torch.equal(inter, ref) and model.launch_counts()[0] == chunks(3 * R) * (1 + n_fwd) + 1
    del keep_alive


def test_refusals_by_name_with_nothing_launched(data):
    batch, donor = data
    L = _lib.lib()
    model = _model(None, False, orc.init_params(None, 42, False), 4)
    bs, keep_alive = model.pack_batch(batch)
    with torch.no_grad():
        model(*_args(batch))
    f0 = model.launch_counts()
    st = torch.cuda.current_stream().cuda_stream
    out = torch.full((3, 2, 63, 2), float("nan"), device="cuda")
    pm, pr, _ = mark_players_wide("cells", 7, 8)
    perms = shapley_permutations(63, 2, 0)
    good_focal = np.array([31, 60], dtype=np.int32)
    big = _lib.cf_batch.from_buffer_copy(bs)
    big.B = 5

    def opts(n_players=63, marks=pm, regions=pr, scale=0.0):
        o = _lib.cf_mark_wide_opts()
        o.n_players, o.scale = n_players, scale
        o.player_marks = marks.ctypes.data if marks is not None else None
        o.player_regions = regions.ctypes.data if regions is not None else None
        return o

    name = b"cf_mark_shapley_interactions_sampled"

    def call(h=model._handle, b=bs, o=None, p=perms, n=2, focal=good_focal, nf=2, index=0, dst=out, phi=None, phi_se=None):
        o = opts() if o is None else o
        return L.cf_mark_shapley_interactions_sampled(h, C.byref(b) if b is not None else None, C.byref(o) if o is not False else None,
                                                      p.ctypes.data if p is not None else None, n, focal.ctypes.data if focal is not None else None, nf,
                                                      index, dst.data_ptr() if dst is not None else None, None, phi, phi_se, None, st)

    def refused(rc, *needles):
        err = L.cf_last_error()
        assert rc != 0 and name in err and all(n in err for n in needles), err

    # what the sibling refuses
    refused(call(h=None), b"null handle")
    refused(call(b=None), b"null batch")
    refused(call(o=False), b"null opts")
    refused(call(b=big), b"max_batch")
    many = np.ones(129, dtype=np.uint32)
    refused(call(o=opts(n_players=0)), b"n_players = 0 outside 1..128")
    refused(call(o=opts(n_players=129, marks=many, regions=many)), b"n_players = 129 outside 1..128")
    refused(call(o=opts(marks=None)), b"null player_marks")
    zero = pm.copy()
    zero[40] = 0
    refused(call(o=opts(marks=zero)), b"player_marks[40] = 0")
    refused(call(o=opts(scale=-0.5)), b"scale")
    refused(call(p=None), b"null perms")
    refused(call(n=0), b"n_perm = 0")
    twice = perms.copy()
    twice[1, 5] = twice[1, 6]
    refused(call(p=twice), b"perms[1]", b"not a permutation")
    # ... and its own
    refused(call(dst=None), b"null inter")
    refused(call(focal=None), b"null focal")
    refused(call(nf=0), b"n_focal = 0 outside 1..63")
    refused(call(nf=64), b"n_focal = 64 outside 1..63")
    refused(call(focal=np.array([31, 63], dtype=np.int32)), b"focal[1] = 63 outside 0..62")
    refused(call(focal=np.array([-1, 3], dtype=np.int32)), b"focal[0] = -1 outside 0..62")
    refused(call(focal=np.array([31, 31], dtype=np.int32)), b"focal[1] = 31 repeats focal[0]")
    refused(call(index=2), b"index = 2")
    refused(call(index=-1), b"index = -1")
    refused(call(o=opts(n_players=1), nf=1, focal=np.array([0], dtype=np.int32)), b"a pair needs at least 2")
    refused(call(phi_se=out.data_ptr()), b"phi_se without phi")
    name = b"cf_perm_interactions_from_rows"
    rows = torch.zeros(1, 8, 2, device="cuda")

    def op(h=model._handle, rows=rows, B=1, P=63, n_out=2, focal=good_focal):
        return L.cf_perm_interactions_from_rows(h, rows.data_ptr() if rows is not None else None, B, P, n_out, perms.ctypes.data, 2, focal.ctypes.data, 2, 0,
                                                out.data_ptr(), None, None, None, st)

    refused(op(h=None), b"null handle")
    refused(op(rows=None), b"null rows")
    refused(op(B=0), b"B = 0")
    refused(op(P=129), b"P = 129 outside 2..128")
    refused(op(n_out=0), b"n_out = 0")
    refused(op(focal=np.array([31, 31], dtype=np.int32)), b"repeats")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and model.launch_counts() == f0      # nothing was launched
    # armed riders (a training step in flight): refused; the handle is not used again
    name = b"cf_mark_shapley_interactions_sampled"
    assert L.cf_rider_arm(model._handle, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, 0, 8) == 0, L.cf_last_error()
    refused(call(), b"riders")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    # raised before the library is called
    for kw, msg in ((dict(), "focal is required"), (dict(focal=[63]), "focal_players"), (dict(focal=[1, 1]), "repeats"), (dict(focal=["nobody"]), "not a player name"),
                    (dict(focal=[0], index="banzhaf"), "unknown interaction index"), (dict(focal=[0], players=[(ALL, (0,))]), "a pair needs at least 2"),
                    (dict(focal=[0], permutations=np.zeros((2, 62), dtype=np.int64)), "permutations"), (dict(focal=[0], n_perm=0), "shapley_permutations")):
        with pytest.raises(ValueError, match=msg):
            model.mark_shapley_interactions_sampled((bs, keep_alive), **kw)
    with pytest.raises(ValueError, match="perm_interactions_from_rows: rows"):
        model.perm_interactions_from_rows(rows, perms, [0])
    with pytest.raises(ValueError, match="perm_interactions_from_rows: permutations"):
        model.perm_interactions_from_rows(rows, np.zeros((1, 1), dtype=np.int64), [0])
    del keep_alive


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
            model.mark_shapley_interactions_sampled(*_args(dev), players="regions", focal=[0, 3], n_perm=2, scale=2.0)
            model.mark_shapley_interactions_sampled(*_args(dev), players="compartments", focal=[13], n_perm=1, index="sti", donor=_feats(_dev(batches[1])))
            model.mark_window_shapley_interactions_sampled(*_args(dev), players="promoter", width=8, focal=[1], n_perm=1)
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
    from chromoformer_amd import ChromoformerClassifier, predict
    from chromoformer_amd.data import ChromoformerDataset, GeneStore
    from tests.synth_data import make_dataset
    npy, dnpy = str(tmp_path / "npy"), str(tmp_path / "donor")
    meta = make_dataset(npy, n_genes=20, seed=11)
    dn = do.donor_dataset(npy, dnpy, do.DONOR_SEED, w_prom=40000)
    genes = pd.read_csv(meta).gene_id.tolist()[:2]
    allg = pd.read_csv(meta).gene_id.tolist()
    P = orc.init_params(seed=7)
    ck = str(tmp_path / "w.pt")
    torch.save({"net": P}, ck)
    ds = ChromoformerDataset(meta, npy, allg)
    model = ChromoformerClassifier(seed=123, max_batch=32).cuda(0)
    model.load_state_dict(P)
    names = mark_players_wide("regions", 7, 8)[2]
    perms = shapley_permutations(9, 3, 9)
    store = GeneStore(ds, device=model._device, resident=True)
    dstore = GeneStore(dn, device=model._device, resident=True)
    results = {}
    for tag, donor_ds in (("scale", None), ("donor", dn)):
        res = list(model.mark_shapley_interactions_sampled_dataset(ds, donor_ds, genes=genes, players="regions", top=2, n_perm=3, seed=9, scale=0.5))
        assert [r["gene_id"] for r in res] == genes
        d = store.batch([0, 1])
        kw = dict(donor=_feats(dstore.batch([0, 1]))) if donor_ds is not None else dict(scale=0.5)
        phi = model.mark_shapley_sampled(*_args(d), players="regions", permutations=perms, **kw)[0].cpu().numpy()
        for i, r in enumerate(res):
            assert sorted(r) == ["absent", "focal", "focal_names", "gene_id", "index", "interactions", "logits", "permutations", "phi", "phi_stderr",
                                 "players", "stderr"]
            top = np.argsort(-np.abs(phi[i, :, -1]), kind="stable")[:2]
            assert r["focal"].tolist() == top.tolist() and r["focal_names"] == [names[p] for p in top] and r["players"] == names
            one = store.batch([i])
            kw1 = dict(donor=_feats(dstore.batch([i]))) if donor_ds is not None else dict(scale=0.5)
            inter, info = model.mark_shapley_interactions_sampled(*_args(one), players="regions", focal=top, permutations=perms, return_rows=True, **kw1)
            assert r["interactions"].shape == r["stderr"].shape == (2, 9, 2) and r["interactions"].dtype == np.float32
            assert np.array_equal(r["interactions"], inter[0].cpu().numpy()) and np.array_equal(r["stderr"], info["stderr"][0].cpu().numpy())
            assert np.array_equal(r["phi"], info["phi"][0].cpu().numpy()) and np.array_equal(r["logits"], info["logits"][0].cpu().numpy())
            assert np.array_equal(r["permutations"], perms) and r["index"] == "sii"
            _check_estimate(r["interactions"][None], r["stderr"][None], info["rows"].cpu().numpy(), perms, top, "sii")
        results[tag] = res
    given = list(model.mark_shapley_interactions_sampled_dataset(ds, genes=genes, players="regions", focal=["pcre0", "promoter"], index="sti", n_perm=3, seed=9))
    assert all(r["focal"].tolist() == [1, 0] and r["index"] == "sti" for r in given)
    with pytest.raises(ValueError, match="top = 0"):
        next(model.mark_shapley_interactions_sampled_dataset(ds, genes=genes, players="regions", top=0))
    with pytest.raises(ValueError, match="focal_players"):
        next(model.mark_shapley_interactions_sampled_dataset(ds, genes=genes, players="regions", focal=[9]))
    # the CLI on the same two genes
    sub = str(tmp_path / "two.csv")
    pd.read_csv(meta).iloc[:2].to_csv(sub, index=False)
    out, dout = str(tmp_path / "pairs.npz"), str(tmp_path / "pairs_donor.npz")
    assert predict.main(["-m", sub, "-d", npy, "-w", ck, "-o", str(tmp_path / "p.csv"), "--mark-sampled-interactions-out", out, "--mark-focal", "2",
                         "--mark-sampled-players", "regions", "--mark-perms", "3", "--mark-seed", "9", "--mark-scale", "0.5", "--donor-npy-dir", dnpy,
                         "--mark-donor-sampled-interactions-out", dout]) == 0
    for path, tag in ((out, "scale"), (dout, "donor")):
        z = np.load(path)
        assert sorted(z.files) == ["absent", "focal", "gene_ids", "index", "interactions", "logits", "permutations", "phi", "phi_stderr", "players", "stderr"]
        assert list(z["gene_ids"]) == genes and list(z["players"]) == names and str(z["index"]) == "sii" and np.array_equal(z["permutations"], perms)
        assert z["interactions"].shape == z["stderr"].shape == (2, 2, 9) and z["phi"].shape == (2, 9) and z["focal"].shape == (2, 2)
        for i, r in enumerate(results[tag]):      # the last output column of the generator's result
            assert np.array_equal(z["focal"][i], r["focal"]) and np.array_equal(z["interactions"][i], r["interactions"][..., -1])
            assert np.array_equal(z["stderr"][i], r["stderr"][..., -1]) and np.array_equal(z["phi"][i], r["phi"][..., -1])
            assert np.array_equal(z["logits"][i], r["logits"][-1]) and np.array_equal(z["absent"][i], r["absent"][-1])
    fixed = str(tmp_path / "fixed.npz")
    assert predict.main(["-m", sub, "-d", npy, "-w", ck, "-o", str(tmp_path / "p.csv"), "--mark-sampled-interactions-out", fixed, "--mark-focal",
                         "pcre0,promoter", "--mark-sampled-players", "regions", "--mark-perms", "3", "--mark-seed", "9", "--interaction-index", "sti"]) == 0
    z = np.load(fixed)
    assert z["focal"].tolist() == [[1, 0], [1, 0]] and str(z["index"]) == "sti"
    assert np.array_equal(z["interactions"], np.stack([r["interactions"][..., -1] for r in given]))
    for argv in (["--mark-focal", "2"], ["--mark-sampled-interactions-out", fixed, "--mark-focal", "0"],
                 ["--mark-donor-sampled-interactions-out", fixed], ["--mark-sampled-interactions-out", fixed, "--mark-focal", "pcre0,,x"]):
        with pytest.raises(SystemExit) as e:
            predict.main(["-m", sub, "-d", npy, "-w", ck, "-o", str(tmp_path / "p.csv")] + argv)
        assert e.value.code == 2, argv
