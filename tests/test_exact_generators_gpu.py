"""The exact dataset generators (attribution.mark_shapley, mark_donor_shapley, mark_window_shapley, mark_fine_window_shapley) under the
combinations of `interactions`, `dividends`, a donor dataset and `epistasis` that no other test runs: every dict against the direct
model.* calls on the same batches, bit for bit, and its sorted key set.

The other tests run, per generator (i = an interaction index, d = dividends, e = epistasis, donor = a donor dataset):
  mark_shapley              plain, e, i, d                  (test_mark_coalitions_gpu, test_shapley_interactions_gpu, test_dividends_gpu)
  mark_donor_shapley        plain, e, i, i + d              (test_mark_donor_gpu, test_shapley_interactions_gpu, test_dividends_gpu)
  mark_window_shapley       plain, donor, i, d              (test_mark_windows_gpu, test_shapley_interactions_gpu, test_dividends_gpu)
  mark_fine_window_shapley  plain, donor, i, d              (test_mark_fine_windows_gpu, test_shapley_interactions_gpu, test_dividends_gpu)
and this file the rest: four combinations each.  The 20-gene synthetic data set, 10 genes in chunks of 7 (two chunks of different size)."""
import copy

import numpy as np
import pandas as pd
import pytest
import torch

from oracle import chromoformer_oracle as orc
from tests import donor_oracle as do
from tests import scan_oracle as so

pytestmark = pytest.mark.gpu
BASE = ["gene_id", "logits", "phi", "players"]
OPTIONAL = {"i": ["interactions"], "d": ["dividends", "mass"], "e": ["eps"]}


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    """The two cell types, the model and resident stores of the ten genes: built once, never written."""
    from chromoformer_amd import ChromoformerClassifier
    from chromoformer_amd.data import ChromoformerDataset, GeneStore
    from tests.synth_data import make_dataset
    root = tmp_path_factory.mktemp("exact_generators")
    npy, dnpy = str(root / "npy"), str(root / "donor")
    meta = make_dataset(npy, n_genes=20, seed=11)
    genes = pd.read_csv(meta).gene_id.tolist()
    ds = ChromoformerDataset(meta, npy, genes)
    dn = do.donor_dataset(npy, dnpy, do.DONOR_SEED, w_prom=40000)
    model = ChromoformerClassifier(seed=123, max_batch=32).cuda(0)
    model.load_state_dict(orc.init_params(seed=7))
    sub = genes[3:13]

    def resident(dataset):
        part = copy.copy(dataset)
        part.target_genes = list(sub)
        return GeneStore(part, device=model._device, resident=True)

    return dict(ds=ds, dn=dn, model=model, sub=sub, store=resident(ds), dstore=resident(dn), plain={})


def _chunks(env, donor):
    """Per chunk of 7 genes -> (first gene, n, forward()'s arguments, the donor pair or None, the donor's batch dict or None)."""
    for lo in (0, 7):
        n = min(7, 10 - lo)
        b = env["store"].batch(list(range(lo, lo + n)))
        db = env["dstore"].batch(list(range(lo, lo + n))) if donor else None
        yield lo, n, tuple(b[k] for k in so.KEYS), (db["promoter_feats"], db["pcre_feats"]) if donor else None, db


def _direct(model, prefix, args, kw, interactions, dividends):
    """The direct calls of one exact game -> host arrays (phi, interactions or None, dividends or None, mass or None) and info."""
    if interactions is None:
        inter, (phi, info) = None, getattr(model, prefix + "_shapley")(*args, return_coalitions=dividends, **kw)
    else:
        inter, info = getattr(model, prefix + "_shapley_interactions")(*args, index=interactions, return_coalitions=dividends, **kw)
        phi, inter = info["phi"], inter.cpu().numpy()
    div, mass = None, None
    if dividends:
        div, mass = (t.cpu().numpy() for t in model.shapley_dividends(info["coalitions"], return_mass=True))
    return phi.cpu().numpy(), inter, div, mass, info


def _same(a, b):
    return a.dtype == b.dtype and np.array_equal(a, b)


def _keys(flags, base):
    return sorted(base + [k for f in flags for k in OPTIONAL[f]])


def _check_optional(r, i, inter, div, mass):
    if inter is not None:
        assert _same(r["interactions"], inter[i])
    if div is not None:
        assert _same(r["dividends"], div[i]) and _same(r["mass"], mass[i])


@pytest.mark.parametrize("flags", ["id", "ide", "ie", "de"])
def test_mark_shapley(env, flags):
    model, sub = env["model"], env["sub"]
    index, div_on, eps_on = "sii" if "i" in flags else None, "d" in flags, "e" in flags
    res = list(model.mark_shapley_dataset(env["ds"], genes=sub, players="regions", scale=0.5, epistasis=eps_on, bsz=7, interactions=index,
                                          dividends=div_on))
    assert [r["gene_id"] for r in res] == sub
    kw = dict(players="regions", scale=0.5)
    for lo, n, args, _, _ in _chunks(env, False):
        phi, inter, div, mass, info = _direct(model, "mark", args, kw, index, div_on)
        eps = model.mark_epistasis(*args, **kw)[0].cpu().numpy() if eps_on else None
        for i in range(n):
            r = res[lo + i]
            assert sorted(r) == _keys(flags, BASE + ["erased"]) and len(r["players"]) == 9
            assert _same(r["phi"], phi[i]) and _same(r["logits"], info["logits"][i].cpu().numpy()) and _same(r["erased"], info["erased"][i].cpu().numpy())
            assert eps is None or _same(r["eps"], eps[i])
            _check_optional(r, i, inter, div, mass)


@pytest.mark.parametrize("flags", ["d", "de", "ie", "ide"])
def test_mark_donor_shapley(env, flags):
    model, sub = env["model"], env["sub"]
    index, div_on, eps_on = "sii" if "i" in flags else None, "d" in flags, "e" in flags
    res = list(model.mark_donor_shapley_dataset(env["ds"], env["dn"], genes=sub, players="regions", epistasis=eps_on, bsz=7, interactions=index,
                                                dividends=div_on))
    assert [r["gene_id"] for r in res] == sub
    for lo, n, args, donor, db in _chunks(env, True):
        kw = dict(donor=donor, players="regions")
        phi, inter, div, mass, info = _direct(model, "mark_donor", args, kw, index, div_on)
        eps = model.mark_donor_epistasis(*args, **kw)[0].cpu().numpy() if eps_on else None
        with torch.no_grad():
            pred = model(*(db[k] for k in so.KEYS)).cpu().numpy()
        for i in range(n):
            r = res[lo + i]
            assert sorted(r) == _keys(flags, BASE + ["donor", "donor_prediction"]) and len(r["players"]) == 9
            assert _same(r["phi"], phi[i]) and _same(r["logits"], info["logits"][i].cpu().numpy()) and _same(r["donor"], info["donor"][i].cpu().numpy())
            assert _same(r["donor_prediction"], pred[i]) and (eps is None or _same(r["eps"], eps[i]))
            _check_optional(r, i, inter, div, mass)


WINDOW_CASES = [("id", False), ("i", True), ("d", True), ("id", True)]


@pytest.mark.parametrize("flags, donor", WINDOW_CASES, ids=["%s-%s" % (f, "donor" if d else "scale") for f, d in WINDOW_CASES])
def test_mark_window_shapley(env, flags, donor):
    model, sub, ds = env["model"], env["sub"], env["ds"]
    index, div_on = "sii" if "i" in flags else None, "d" in flags
    gen = lambda **kw: list(model.mark_window_shapley_dataset(ds, env["dn"] if donor else None, genes=sub, width=4, scale=0.25, bsz=7, **kw))      # noqa: E731
    if ("window", donor) not in env["plain"]:      # (the host-side keys -- names, coordinates, null players -- from the plain run other tests pin)
        env["plain"]["window", donor] = gen()
    res, plain = gen(interactions=index, dividends=div_on), env["plain"]["window", donor]
    assert [r["gene_id"] for r in res] == sub
    for lo, n, args, pair, _ in _chunks(env, donor):
        flip = [ds.genes[g]["tss"][2] != "+" for g in sub[lo:lo + n]]
        phi, inter, div, mass, info = _direct(model, "mark_window", args, dict(players="promoter", width=4, scale=0.25, donor=pair, flip=flip), index, div_on)
        absent = info["donor" if donor else "erased"].cpu().numpy()
        for i in range(n):
            r, p = res[lo + i], plain[lo + i]
            assert sorted(r) == _keys(flags, BASE + ["absent", "estimator", "null", "stderr", "windows"]) and r["estimator"] == "exact"
            assert _same(r["phi"], phi[i]) and _same(r["logits"], info["logits"][i].cpu().numpy()) and _same(r["absent"], absent[i])
            assert _same(r["stderr"], np.zeros((5, 2), np.float32)) and len(r["players"]) == 5
            assert r["players"] == p["players"] and r["windows"] == p["windows"] and _same(r["null"], p["null"])
            _check_optional(r, i, inter, div, mass)


@pytest.mark.parametrize("flags, donor", WINDOW_CASES, ids=["%s-%s" % (f, "donor" if d else "scale") for f, d in WINDOW_CASES])
def test_mark_fine_window_shapley(env, flags, donor):
    """zoom = 2: two ranks per gene.  The promoter in 4 coarse players of 5 coarsest bins, each zoomed window in 4 fine players of 25
    finest bins; a rank's start comes from the direct coarse game, as the generator takes it."""
    model, sub, ds = env["model"], env["sub"], env["ds"]
    index, div_on = "sii" if "i" in flags else None, "d" in flags
    gen = lambda **kw: list(model.mark_fine_window_shapley_dataset(ds, env["dn"] if donor else None, genes=sub, region="promoter", zoom=2,      # noqa: E731
                                                                   coarse_width=5, width=25, scale=0.25, bsz=7, **kw))
    if ("fine", donor) not in env["plain"]:
        env["plain"]["fine", donor] = gen()
    res, plain = gen(interactions=index, dividends=div_on), env["plain"]["fine", donor]
    assert [r["gene_id"] for r in res] == sub
    coarse = [(list(range(7)), [0], (g, g + 5)) for g in range(0, 20, 5)]
    for lo, n, args, pair, _ in _chunks(env, donor):
        flip = [ds.genes[g]["tss"][2] != "+" for g in sub[lo:lo + n]]
        cphi, cinfo = model.mark_window_shapley(*args, players=coarse, scale=0.25, donor=pair, flip=flip)
        cphi = cphi.cpu().numpy()
        zoom = [np.argsort(-np.abs(cphi[i, :, 1]), kind="stable")[:2] for i in range(n)]
        for rank in (0, 1):
            kw = dict(region=0, players="windows", width=25, n_windows=4, start=[int(z[rank]) * 100 for z in zoom], lengths=[40000] * n, scale=0.25,
                      donor=pair, flip=flip)
            phi, inter, div, mass, info = _direct(model, "mark_fine_window", args, kw, index, div_on)
            absent = info["donor" if donor else "erased"].cpu().numpy()
            for i in range(n):
                r, p = res[lo + i], plain[lo + i]
                mine = r["rank"] == rank
                assert sorted(r) == _keys(flags, ["absent", "coarse_phi", "coarse_windows", "exact", "gene_id", "index", "logits", "phi", "players", "rank",
                                                  "region", "stderr", "windows", "zoom"])
                assert r["exact"] is True and r["stderr"] is None and _same(r["zoom"], zoom[i].astype(np.int64)) and _same(r["coarse_phi"], cphi[i])
                assert r["index"][mine].tolist() == [0, 1, 2, 3] and _same(r["phi"][mine], phi[i]) and _same(r["absent"][rank], absent[i])
                assert _same(r["logits"], cinfo["logits"][i].cpu().numpy())
                assert r["players"] == p["players"] and r["windows"] == p["windows"] and r["coarse_windows"] == p["coarse_windows"] and r["region"] == p["region"]
                if inter is not None:
                    assert len(r["interactions"]) == 2 and _same(r["interactions"][rank], inter[i])
                if div is not None:
                    assert len(r["dividends"]) == len(r["mass"]) == 2 and _same(r["dividends"][rank], div[i]) and _same(r["mass"][rank], mass[i])
