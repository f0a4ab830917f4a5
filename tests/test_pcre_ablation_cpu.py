"""In-silico pCRE deletion without a GPU: the reference's logits with the interaction-mask row and column of a pCRE set equal those
with the pCRE made a dataset dummy (bit for bit) and with it physically removed (tests/golden/pcre_ablation.npz) -- "mask row and
column" means "delete the pCRE" --, the oracle of tests/ablation_oracle.py reproduces them, and cf_pcre_ablation is declared, bound
and offered by the predict CLI."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import chromoformer_oracle as orc
from tests.ablation_oracle import oracle_ablation
from tests.helpers import GOLDEN, load_npz_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _batch(tag):
    return load_npz_batch("demo_subset.npz")[0] if tag == "demo" else orc.synthetic_batch(8, seed=31, regime="realistic")


@pytest.mark.parametrize("head", ["clf", "reg"])
@pytest.mark.parametrize("tag", ["demo", "real"])
def test_masking_a_pcre_is_deleting_it_in_the_reference(tag, head):
    z = np.load(os.path.join(GOLDEN, "pcre_ablation.npz"))
    masked, dummy, gone = (z["%s.%s.%s" % (tag, head, k)] for k in ("masked", "dummy", "removed"))
    assert masked.shape == (8 if tag == "real" else 6, 10, 1 if head == "reg" else 2)
    assert np.array_equal(masked, dummy)
    assert np.abs(masked - gone).max() <= 1e-5
    # the variants differ from the baseline where there is a pCRE to delete, and not where the slot is already a dummy
    im = _batch(tag)["interaction_masks"][2000][:, 0, 0, 1:].numpy()      # [B, S]: key j + 1 masked for the promoter row
    delta = np.abs(masked[:, 1:9] - masked[:, :1]).max(-1)
    assert (delta[im] == 0).all() and (delta[~im] > 0).all()


@pytest.mark.parametrize("regression", [False, True], ids=["classifier", "regressor"])
@pytest.mark.parametrize("tag", ["demo", "real"])
def test_the_oracle_reproduces_the_reference(tag, regression):
    z = np.load(os.path.join(GOLDEN, "pcre_ablation.npz"))
    got = oracle_ablation(orc.init_params(None, 42, regression), _batch(tag))
    ref = torch.from_numpy(z["%s.%s.masked" % (tag, "reg" if regression else "clf")])
    assert got.shape == ref.shape
    assert (got - ref).abs().max().item() <= 1e-6


def test_the_entry_point_is_declared_bound_and_offered():
    hdr = open(os.path.join(ROOT, "include", "chromoformer_hip.h")).read()
    assert re.search(r"int\s+cf_pcre_ablation\s*\(\s*cf_handle\s*\*\s*h\s*,\s*const\s+cf_batch\s*\*\s*batch\s*,\s*float\s*\*\s*logits\s*,"
                     r"\s*void\s*\*\s*stream\s*\)", hdr)
    from chromoformer_amd import _lib
    assert "cf_pcre_ablation" in _lib.SYMBOLS
    from chromoformer_amd import ChromoformerRegressor
    from chromoformer_amd.net import Chromoformer
    assert Chromoformer.pcre_ablation is ChromoformerRegressor.pcre_ablation
    out = subprocess.run([sys.executable, "-m", "chromoformer_amd.predict", "--help"], cwd=ROOT, capture_output=True, text=True,
                         check=True).stdout
    assert "--pcre-ablation-out" in out
