"""Every attribution method that takes the six tensors of forward(), through the one entry for the batch (net_attrib._attrib_call) and,
for the 25 games, the one runner (net_attrib._game), at the smallest arguments that pass every check:

  (a) the six tensors, the pack_batch result and its bare batch struct give the same bits in every returned tensor, and the same
      non-tensor entries;
  (b) the call books itself: a backward() pending from an earlier grad-enabled model(...) raises, naming exactly that method;
  (c) a call refused AFTER the device check (17 fine window players, a donor of B + 1 genes) has booked nothing: the pending
      backward() still runs and leaves the gradients of an undisturbed forward + backward.

What the methods compute is pinned by the oracle tests of each family; here only the plumbing around them is.  The default model with
the seed-7 weights, three genes of the 20-gene synthetic set (tests/synth_data.py, seed 11): a '-' strand gene, a gene with dummy pCRE
slots, a gene with all eight."""
import inspect

import numpy as np
import pandas as pd
import pytest
import torch

from oracle import chromoformer_oracle as orc
from tests import donor_oracle as do
from tests import scan_oracle as so
from tests.synth_data import make_dataset
from tests.test_input_grads_gpu import _model

pytestmark = pytest.mark.gpu
B = 3
P2, P3 = [((0,), (0,)), ((1, 2), (0, 1))], [((0,), (0,)), ((1,), (0, 1, 2)), ((2, 3), (1,))]      # (marks, regions) players
W2, W3 = [((0,), (0,), (3, 5)), ((1, 2), (0, 1), (0, 2))], [((0,), (0,), (g, g + 1)) for g in (2, 9, 19)]      # + (lo, hi), coarse bins
F2, F3 = [((0,), (190, 192)), ((1, 2), (200, 203))], [((0,), (g, g + 2)) for g in (0, 199, 398)]      # (marks, (lo, hi)), finest bins
W17, F17 = [((0,), (0,), (g, g + 1)) for g in range(17)], [((0,), (g, g + 1)) for g in range(17)]
SAMPLED = dict(n_perm=2, seed=3)
FINE = dict(region=0, start=[0, 5, 390], lengths=[40000] * B)

# (method, keyword arguments; "donor" / "flip" stand for the fixture's), 31 methods, some twice
CASES = [
    ("attention_maps", {}), ("attention_maps", dict(which="regulation")), ("pcre_ablation", {}),
    ("pcre_coalitions", dict(keep=[0, 5, 255])), ("pcre_shapley", dict(return_coalitions=True)), ("pcre_epistasis", {}),
    ("pcre_shapley_interactions", dict(index="sti")),
    ("integrated_gradients", dict(n_steps=2)), ("integrated_gradients", dict(n_steps=2, path="signal", donor="donor")),
    ("perturbation_scan", dict(mark_sets=[(0, 1)], flip="flip", return_feats=True)),
    ("perturbation_scan_regions", dict(regions=(0, 2), mark_sets=[(3,)], flip="flip")),
    ("perturbation_scan_fine", dict(mark_sets=[(2,)], width=3, n_windows=2, flip="flip", return_feats=True, **FINE)),
    ("mark_coalitions", dict(keep=[0, 1, 3], players=P2)), ("mark_shapley", dict(players=P3, return_coalitions=True)),
    ("mark_epistasis", dict(players=P2, scale=0.5)), ("mark_shapley_interactions", dict(players=P2)),
    ("mark_donor_coalitions", dict(keep=[0, 2], players=P2, donor="donor")), ("mark_donor_shapley", dict(players=P2, donor="donor")),
    ("mark_donor_epistasis", dict(players=P3, donor="donor")),
    ("mark_donor_shapley_interactions", dict(players=P3, donor="donor", index="sti", return_coalitions=True)),
    ("mark_coalitions_wide", dict(keep=[0, 3], players=P2)), ("mark_coalitions_wide", dict(keep=[1], players=P2, donor="donor")),
    ("mark_shapley_sampled", dict(players=P3, return_rows=True, **SAMPLED)), ("mark_shapley_sampled", dict(players=P2, donor="donor", **SAMPLED)),
    ("mark_shapley_interactions_sampled", dict(players=P3, focal=[1], **SAMPLED)),
    ("mark_window_coalitions", dict(keep=[0, 1], players=W2, flip="flip")), ("mark_window_shapley", dict(players=W3, flip="flip")),
    ("mark_window_shapley", dict(players=W2, donor="donor", return_coalitions=True)),
    ("mark_window_shapley_interactions", dict(players=W2, flip="flip")),
    ("mark_window_shapley_sampled", dict(players=W3, flip="flip", **SAMPLED)),
    ("mark_window_shapley_interactions_sampled", dict(players=W3, focal=[0], index="sti", return_rows=True, **SAMPLED)),
    ("mark_fine_window_coalitions", dict(keep=[0, 2], players=F2, flip="flip", return_feats=True, **FINE)),
    ("mark_fine_window_shapley", dict(players=F3, flip="flip", return_feats=True, **FINE)),
    ("mark_fine_window_shapley", dict(players=F2, donor="donor", **FINE)),
    ("mark_fine_window_shapley_interactions", dict(players=F2, flip="flip", return_coalitions=True, **FINE)),
    ("mark_fine_window_shapley_sampled", dict(players=F3, flip="flip", return_feats=True, **SAMPLED, **FINE)),
    ("mark_fine_window_shapley_interactions_sampled", dict(players="windows", width=200, focal=[1], flip="flip", **SAMPLED, **FINE)),
]
# the exact games refuse a 17th player by message: the window games before the device is asked for, the fine games after it
TOO_MANY = [("mark_window_shapley", dict(players=W17), "takes 1..16"), ("mark_window_shapley_interactions", dict(players=W17), "takes 2..16"),
            ("mark_fine_window_shapley", dict(players=F17, **FINE), "takes 1..16"),
            ("mark_fine_window_shapley_interactions", dict(players=F17, **FINE), "takes 2..16")]
# one method per kind, refused after the device check
DONOR4 = r"donor promoter_feats\[2000\] has shape"
LATE = [("mark_donor_coalitions", dict(keep=[1], players=P2, donor="donor4"), DONOR4), ("mark_fine_window_shapley", TOO_MANY[2][1], "takes 1..16"),
        ("mark_donor_epistasis", dict(players=P2, donor="donor4"), DONOR4),
        ("mark_fine_window_shapley_interactions", TOO_MANY[3][1], "takes 2..16"),
        ("mark_shapley_sampled", dict(players=P2, donor="donor4", **SAMPLED), DONOR4),
        ("mark_shapley_interactions_sampled", dict(players=P2, focal=[0], donor="donor4", **SAMPLED), DONOR4)]


def test_the_cases_cover_the_methods():
    from chromoformer_amd.net_attrib import AttributionMixin
    six = [n for n, f in vars(AttributionMixin).items() if not n.startswith("_") and callable(f) and "pcre_pad_masks" in inspect.signature(f).parameters]
    assert len(six) == 31 and {m for m, _ in CASES} == set(six)


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    """The model, the three genes in the three forms, their donor (three genes, and four), the promoter flips: built once, never written."""
    from chromoformer_amd.data import ChromoformerDataset
    npy = str(tmp_path_factory.mktemp("npy"))
    meta = make_dataset(npy, n_genes=20, seed=11)
    table = pd.read_csv(meta)
    partners = [0 if isinstance(n, float) else len(n.split(";")) for n in table.neighbors]
    minus = next(i for i in range(20) if table.strand[i] == "-")
    short = next(i for i in range(20) if 0 < partners[i] < 8 and i != minus)
    full = next(i for i in range(20) if partners[i] == 8 and i != minus)
    genes = [minus, short, full]
    ds = ChromoformerDataset(meta, npy, table.gene_id.tolist())
    dn = do.donor_dataset(npy, str(tmp_path_factory.mktemp("donor")), w_prom=40000)

    def batch(d, idx):
        b = torch.utils.data.default_collate([d[i] for i in idx])
        return {k: ({r: t.cuda() for r, t in v.items()} if isinstance(v, dict) else v.cuda()) for k, v in b.items() if k in so.KEYS}

    model = _model(None, False, orc.init_params(None, 7, False), 4)
    dev, donor = batch(ds, genes), batch(dn, genes)
    donor4 = batch(dn, genes + [next(i for i in range(20) if i not in genes)])
    packed = model.pack_batch(dev)
    return dict(model=model, six=tuple(dev[k] for k in so.KEYS), packed=packed, struct=packed[0], flip=[True, False, False],
                donor=(donor["promoter_feats"], donor["pcre_feats"]), donor4=(donor4["promoter_feats"], donor4["pcre_feats"]))


def _kw(env, kw):
    return {k: (env[v] if isinstance(v, str) and v in ("donor", "donor4", "flip") else v) for k, v in kw.items()}


def _same(a, b, path, shapes=True):
    """Walks tuples, lists and dicts; tensors carry the same bits (and shapes), everything else is equal."""
    if torch.is_tensor(a):
        assert torch.is_tensor(b) and a.dtype == b.dtype and (not shapes or a.shape == b.shape), path
        assert torch.equal(a.reshape(-1), b.reshape(-1)), path
    elif isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), path
        for k in a:
            _same(a[k], b[k], path + (k,), shapes)
    elif isinstance(a, (tuple, list)):
        assert type(a) is type(b) and len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, path + (i,), shapes)
    elif isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b), path
    else:
        assert type(a) is type(b) and a == b, path


@pytest.mark.parametrize("method,kw", CASES, ids=["%s-%d" % (m, i) for i, (m, _) in enumerate(CASES)])
def test_three_forms_same_bits_and_the_call_is_booked(env, method, kw):
    model, kw = env["model"], _kw(env, kw)
    with torch.enable_grad():
        out = model(*env["six"])
    from_six = getattr(model, method)(*env["six"], **kw)
    with torch.enable_grad(), pytest.raises(RuntimeError, match=r"loss\.backward\(\): %s\(\) has run a forward pass" % method):
        out.sum().backward()
    from_packed = getattr(model, method)(env["packed"], **kw)
    from_struct = getattr(model, method)(env["struct"], **kw)
    torch.cuda.synchronize()
    # (integrated_gradients returns the attributions in the caller's shapes where it was given tensors, in the library's otherwise)
    _same(from_six, from_packed, (method, "packed"), shapes=method != "integrated_gradients")
    _same(from_packed, from_struct, (method, "struct"))


@pytest.mark.parametrize("method,kw,text", TOO_MANY, ids=[m for m, _, _ in TOO_MANY])
def test_a_seventeenth_player_is_refused_by_message(env, method, kw, text):
    with pytest.raises(ValueError, match=r"%s: 17 players; the exact game %s" % (method, text)):
        getattr(env["model"], method)(env["packed"], **kw)


def test_a_call_refused_after_the_device_check_leaves_a_pending_backward_usable(env):
    model = env["model"]
    with torch.enable_grad():
        model(*env["six"])[:, 1].sum().backward()
    ref = model._gflat.clone()
    model._gflat.zero_()
    with torch.enable_grad():
        out = model(*env["six"])
    gen = model._maps_gen
    for method, kw, text in LATE:
        for form in (env["six"], (env["packed"],)):
            with pytest.raises(ValueError, match=text):
                getattr(model, method)(*form, **_kw(env, kw))
    assert model._maps_gen == gen
    with torch.enable_grad():
        out[:, 1].sum().backward()
    assert torch.equal(model._gflat, ref) and float(ref.abs().sum()) > 0
