"""The public surface of the model classes, and what a model that was never moved to a GPU refuses, against tests/golden/model_api.json
(tests/golden/make_goldens.py model_api, written on the commit before the attribution methods moved into net_attrib.py): the names,
the signatures, and type and message of every device-free refusal.  Docstring TEXT is not in the fixture, so that a wording fix does
not need a new one; that every moved method still has one is asserted here."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

from chromoformer_amd import _lib, net

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_api.json")
CLASSES = ("ChromoformerBase", "ChromoformerClassifier", "ChromoformerRegressor", "Chromoformer")


def public_names(cls):
    """The public attributes a model class adds to, or overrides of, torch.nn.Module (the walk of make_goldens.model_api)."""
    return sorted(n for n in dir(cls) if not n.startswith("_")
                  and inspect.getattr_static(cls, n) is not inspect.getattr_static(torch.nn.Module, n, None))


def _table(P, dtype=torch.float32):
    return torch.zeros(1, 1 << P, 2, dtype=dtype)


_SIX = [{2000: torch.zeros(1)}] * 5 + [torch.zeros(1)]      # six tensors' worth of arguments: a model without a device never reads them
_DONOR = ({2000: torch.zeros(1)}, {2000: torch.zeros(1)})

# id -> the call.  `m`: a ChromoformerClassifier that was never moved to a device; `b`: an (empty) batch struct, the packed form of the
# first argument that reaches the device check without a tensor being touched.
REFUSALS = {
    # keep is required
    "pcre_coalitions:keep": lambda m, b: m.pcre_coalitions(b),
    "mark_coalitions:keep": lambda m, b: m.mark_coalitions(b),
    "mark_donor_coalitions:keep": lambda m, b: m.mark_donor_coalitions(b, donor=b),
    "mark_coalitions_wide:keep": lambda m, b: m.mark_coalitions_wide(b),
    "mark_window_coalitions:keep": lambda m, b: m.mark_window_coalitions(b),
    "mark_fine_window_coalitions:keep": lambda m, b: m.mark_fine_window_coalitions(b),
    # a bad players spec, a bad word of keep
    "mark_coalitions:players": lambda m, b: m.mark_coalitions(b, keep=[1], players="nucleosomes"),
    "mark_shapley:players": lambda m, b: m.mark_shapley(b, players="nucleosomes"),
    "mark_epistasis:players": lambda m, b: m.mark_epistasis(b, players=[((99,), (0,))]),
    "mark_shapley_interactions:players": lambda m, b: m.mark_shapley_interactions(b, players="nucleosomes"),
    "mark_coalitions:word": lambda m, b: m.mark_coalitions(b, keep=[1 << 7]),
    "pcre_coalitions:word": lambda m, b: m.pcre_coalitions(b, keep=[1 << 8]),
    # a bad index
    "pcre_shapley_interactions:index": lambda m, b: m.pcre_shapley_interactions(b, index="shap"),
    "shapley_interactions:index": lambda m, b: m.shapley_interactions(_table(3), index="shap"),
    "set_interactions:index": lambda m, b: m.set_interactions(_table(2), index="shap"),
    # tables
    "shapley_interactions:P=1": lambda m, b: m.shapley_interactions(_table(1)),
    "shapley_interactions:dtype": lambda m, b: m.shapley_interactions(_table(3, torch.float64)),
    "shapley_interactions:device": lambda m, b: m.shapley_interactions(_table(3)),
    "shapley_dividends:shape": lambda m, b: m.shapley_dividends(torch.zeros(3, 100, 2)),
    "shapley_dividends:n_out": lambda m, b: m.shapley_dividends(torch.zeros(3, 256, 1)),
    "shapley_dividends:numpy": lambda m, b: m.shapley_dividends(np.zeros((3, 4, 2), np.float32)),
    "shapley_dividends:device": lambda m, b: m.shapley_dividends(_table(2)),
    "set_interactions:shape": lambda m, b: m.set_interactions(torch.zeros(256, 2)),
    "set_interactions:device": lambda m, b: m.set_interactions(_table(2)),
    # integrated gradients
    "integrated_gradients:path": lambda m, b: m.integrated_gradients(*_SIX, n_steps=2, path="curved"),
    "integrated_gradients:donor+linear": lambda m, b: m.integrated_gradients(*_SIX, n_steps=2, donor=_DONOR),
    "integrated_gradients:donor+baseline": lambda m, b: m.integrated_gradients(*_SIX, n_steps=2, path="signal", donor=_DONOR,
                                                                               baselines={"pcre_feats": {2000: torch.zeros(1)}}),
    "integrated_gradients:donor+inputs": lambda m, b: m.integrated_gradients(*_SIX, n_steps=2, path="signal", donor=_DONOR,
                                                                             inputs=("interaction_freq",)),
    "integrated_gradients:signal+baseline": lambda m, b: m.integrated_gradients(*_SIX, n_steps=2, path="signal",
                                                                                baselines={"pcre_feats": {2000: torch.zeros(1)}}),
    "integrated_gradients:signal+inputs": lambda m, b: m.integrated_gradients(*_SIX, n_steps=2, path="signal", inputs="interaction_freq"),
    # not on a GPU: one method per family, packed form and six tensors
    "attention_maps:device": lambda m, b: m.attention_maps(b),
    "pcre_ablation:device": lambda m, b: m.pcre_ablation(*_SIX),
    "pcre_shapley:device": lambda m, b: m.pcre_shapley(b),
    "pcre_epistasis:device": lambda m, b: m.pcre_epistasis(*_SIX),
    "mark_shapley:device": lambda m, b: m.mark_shapley(b),
    "mark_donor_shapley:device": lambda m, b: m.mark_donor_shapley(b, donor=b),
    "mark_shapley_sampled:device": lambda m, b: m.mark_shapley_sampled(b, n_perm=2),
    "mark_shapley_interactions_sampled:device": lambda m, b: m.mark_shapley_interactions_sampled(b, focal=[0], n_perm=2),
    "mark_window_shapley:device": lambda m, b: m.mark_window_shapley(b, width=5),
    "mark_fine_window_shapley:device": lambda m, b: m.mark_fine_window_shapley(b, width=100),
    "integrated_gradients:device": lambda m, b: m.integrated_gradients(b, n_steps=2),
    "perturbation_scan:device": lambda m, b: m.perturbation_scan(b),
    "perturbation_scan_regions:device": lambda m, b: m.perturbation_scan_regions(*_SIX),
    "perturbation_scan_fine:device": lambda m, b: m.perturbation_scan_fine(b),
    "perm_interactions_from_rows:device": lambda m, b: m.perm_interactions_from_rows(torch.zeros(1, 4, 2), [[0, 1]], [0]),
    "trunk_outputs:device": lambda m, b: m.trunk_outputs(b),
}


def refusal(case):
    """-> [exception type name, message] of a call that must raise on a model without a device."""
    model = net.ChromoformerClassifier(seed=1, max_batch=2)      # (never .cuda())
    gen = model._maps_gen
    try:
        case(model, _lib.cf_batch())
    except Exception as e:      # noqa: BLE001 (the type is what is compared)
        assert model._maps_gen == gen
        return [type(e).__name__, str(e)]
    raise AssertionError("the call was accepted")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("cls", CLASSES)
def test_public_names_and_signatures(golden, cls):
    c = getattr(net, cls)
    names = public_names(c)
    assert names == golden[cls]["attributes"]
    assert {n: str(inspect.signature(getattr(c, n))) for n in names if callable(getattr(c, n))} == golden[cls]["signatures"]
    assert c.MAP_KEYS == ("embed", "pairwise_interaction", "regulation", "regulatory_embedding") and "MAP_KEYS" in names


def test_every_attribution_method_has_a_docstring_and_is_found_on_the_model():
    from chromoformer_amd.net_attrib import AttributionMixin
    moved = [n for n, f in vars(AttributionMixin).items() if not n.startswith("_") and callable(f)]
    assert len(moved) >= 50 and issubclass(net.ChromoformerBase, AttributionMixin)
    for n in moved:
        doc = inspect.getdoc(getattr(net.ChromoformerBase, n))
        assert doc and "%(" not in doc, n
        assert getattr(net.Chromoformer, n) is getattr(AttributionMixin, n), n


def test_the_refusal_table_covers_what_it_must(golden):
    assert set(REFUSALS) == set(golden["refusals"])
    kept = [k for k in REFUSALS if k.endswith(":keep")]
    assert len(kept) == 6 and all(golden["refusals"][k][0] == "ValueError" and "keep is required" in golden["refusals"][k][1] for k in kept)
    assert sum(golden["refusals"][k][0] == "RuntimeError" for k in REFUSALS if k.endswith(":device")) >= 10


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_device_free_refusal(golden, case):
    assert refusal(REFUSALS[case]) == golden["refusals"][case]
