"""The attribution entry points share one chunk workspace on the handle (attrib_ws, cf_api_attrib.h): one stash, one set of chunk rows
and masks, one growable 32-bit table for coalition words, quadrature nodes and mark sets.  What sharing could break, checked bit for
bit (every comparison is torch.equal):

  * the result of a call does not depend on which calls came before it, and nothing stale is read: the same list of calls in
    opposite orders on two models, and a second pass on the first;
  * the growable buffers grow: a table larger than any initial capacity, then the small call again; against a fresh model;
  * training is untouched: two Trainer steps after the whole list leave the parameters and both moments of a model that never made
    an attribution call.

The default model at max_batch = 4 on three genes: chunks of 4 rows straddle genes.  Allocation failures are not provoked here."""
import pytest
import torch

from oracle import chromoformer_oracle as orc
from tests import scan_oracle as so
from tests.test_input_grads_gpu import _model

pytestmark = pytest.mark.gpu
ALL = tuple(range(7))
WORDS = [0xFF, 0x5A, 0x00]      # everything kept | every other slot | the promoter alone


@pytest.fixture(scope="module")
def args():
    """The six forward arguments of three realistic genes: built once, shared, never written."""
    batch = orc.synthetic_batch(3, regime="realistic")
    return tuple(batch[k] for k in so.KEYS)


@pytest.fixture(scope="module")
def params():
    return orc.init_params(None, 42, False)


def _fresh(params):
    """The seed-42 classifier at max_batch = 4; no attribution call made yet."""
    return _model(None, False, params, 4)


CALLS = [
    ("pcre_ablation", lambda m, a: m.pcre_ablation(*a)),
    ("pcre_coalitions", lambda m, a: m.pcre_coalitions(*a, keep=WORDS)),
    ("pcre_shapley", lambda m, a: m.pcre_shapley(*a, return_coalitions=True)),
    ("pcre_epistasis", lambda m, a: m.pcre_epistasis(*a)),
    ("ig_freq_only", lambda m, a: m.integrated_gradients(*a, n_steps=3, inputs=("interaction_freq",))),
    ("ig_all_inputs", lambda m, a: m.integrated_gradients(*a, n_steps=3)),
    ("ig_signal_path", lambda m, a: m.integrated_gradients(*a, n_steps=3, path="signal")),
    ("scan_regions", lambda m, a: m.perturbation_scan_regions(*a, regions=[0, 1, 2], mark_sets=[ALL])),
    ("attention_maps", lambda m, a: m.attention_maps(*a)),
]


def _tensors(out):
    """Every tensor of a call's result (tensors, tuples, lists and dicts nested in any way), on the host, in a fixed order."""
    if torch.is_tensor(out):
        return [out.detach().cpu().clone()]
    if isinstance(out, dict):
        return [t for k in sorted(out, key=str) for t in _tensors(out[k])]
    if isinstance(out, (tuple, list)):
        return [t for o in out for t in _tensors(o)]
    return []      # (the region list of a scan)


def _run(model, args, calls):
    return {name: _tensors(fn(model, args)) for name, fn in calls}


def _assert_same(got, ref, what):
    assert got.keys() == ref.keys()
    for name in ref:
        assert len(got[name]) == len(ref[name]) > 0, (what, name)
        for i, (g, r) in enumerate(zip(got[name], ref[name])):
            assert g.shape == r.shape and torch.equal(g, r), (what, name, i, (g - r).abs().max().item())


def test_call_order_does_not_matter_and_nothing_is_stale(args, params):
    a, b = _fresh(params), _fresh(params)
    first = _run(a, args, CALLS)
    backwards = _run(b, args, CALLS[::-1])
    _assert_same(backwards, first, "reverse order on a fresh model")
    _assert_same(_run(a, args, CALLS), first, "second pass")


def test_word_table_grows_for_coalitions(args, params):
    m = _fresh(params)
    small = m.pcre_coalitions(*args, keep=WORDS).cpu()
    n = 100 * len(WORDS)      # 300 words: above the table's 256-word floor
    big = m.pcre_coalitions(*args, keep=WORDS * 100).cpu()
    assert big.shape == (3, n, 2)
    for c in range(n):
        assert torch.equal(big[:, c], small[:, c % len(WORDS)]), c
    assert torch.equal(m.pcre_coalitions(*args, keep=WORDS).cpu(), small)
    assert not torch.equal(small[:, 0], small[:, 2])      # (the words do move the logits)


def test_word_table_grows_for_quadrature_nodes(args, params):
    m = _fresh(params)
    few = _tensors(m.integrated_gradients(*args, n_steps=2))
    many = _tensors(m.integrated_gradients(*args, n_steps=150))      # 300 words of nodes and weights: above every floor (64 nodes, 256 words)
    ref = _tensors(_fresh(params).integrated_gradients(*args, n_steps=150))
    assert len(many) == len(ref) > 0
    for i, (g, r) in enumerate(zip(many, ref)):
        assert torch.equal(g, r), (i, (g - r).abs().max().item())
    again = _tensors(m.integrated_gradients(*args, n_steps=2))
    for i, (g, r) in enumerate(zip(again, few)):
        assert torch.equal(g, r), (i, (g - r).abs().max().item())


def test_slot_rows_grow_for_the_scan(args, params):
    m = _fresh(params)
    one, _ = m.perturbation_scan_regions(*args, regions=[1], mark_sets=[ALL])
    two, _ = m.perturbation_scan_regions(*args, regions=[1], mark_sets=[(1, 4), ALL])      # twice the variants: the slot rows grow
    ref, _ = _fresh(params).perturbation_scan_regions(*args, regions=[1], mark_sets=[(1, 4), ALL])
    assert two.shape == ref.shape == (1, 3, 1 + 2 * 20, 2) and torch.equal(two, ref)
    again, _ = m.perturbation_scan_regions(*args, regions=[1], mark_sets=[ALL])
    assert torch.equal(again, one)
    assert torch.equal(two[:, :, 1 + 20:], one[:, :, 1:])      # the all-marks set is the second set of the larger call


def test_training_is_untouched(args, params):
    from chromoformer_amd.engine import Trainer
    batches = [orc.synthetic_batch(4, seed=s, regime="realistic") for s in (21, 22)]

    def run(attribute):
        model = _fresh(params)
        if attribute:
            _run(model, args, CALLS)
        tr = Trainer(model, lr=1e-3)
        for b in batches:
            tr.step(tr.stage(b))
        torch.cuda.synchronize()
        return [t.cpu().clone() for t in (model._flat, model._mflat, model._vflat)]

    for got, ref in zip(run(True), run(False)):
        assert torch.equal(got, ref)
