"""Input gradients without a GPU: the oracle's autograd reproduces the reference's (tests/golden/input_grads.npz), which pins the
fp32 / fp64 oracle that test_input_grads_gpu.py judges the HIP path by; and cf_backward_from_inputs is declared, exported and bound."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from oracle import chromoformer_oracle as orc
from tests.helpers import GOLDEN, load_npz_batch

BINS = (2000, 500, 100)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("regression", [False, True], ids=["classifier", "regressor"])
@pytest.mark.parametrize("tag", ["kat", "real"])
def test_oracle_input_grads_reproduce_the_reference(tag, regression):
    z = np.load(os.path.join(GOLDEN, "input_grads.npz"))
    batch = load_npz_batch("kat.npz")[0] if tag == "kat" else orc.synthetic_batch(8, seed=31, regime="realistic")
    head, col = ("reg", 0) if regression else ("clf", 1)
    gene = int(z["%s.gene" % tag])
    pf = {b: batch["promoter_feats"][b].clone().requires_grad_(True) for b in BINS}
    cf = {b: batch["pcre_feats"][b].clone().requires_grad_(True) for b in BINS}
    fr = batch["interaction_freq"].clone().requires_grad_(True)
    orc.forward(orc.init_params(None, 42, regression), dict(batch, promoter_feats=pf, pcre_feats=cf, interaction_freq=fr))[:, col].sum().backward()
    got = {"interaction_freq": fr.grad}
    for b in BINS:
        got["promoter_feats.%d" % b], got["pcre_feats.%d" % b] = pf[b].grad, cf[b].grad
    for k, g in got.items():
        ref = torch.from_numpy(z["%s.%s.grad.%s" % (tag, head, k)])
        assert (g[gene] - ref).norm().item() <= 1e-5 * ref.norm().item() + 1e-9, k
    if tag == "real":      # gene 7 holds one pCRE and seven dummy slots: their gradients are exact zeros
        for b in BINS:
            assert bool((torch.from_numpy(z["real.%s.grad.pcre_feats.%d" % (head, b)])[1:] == 0).all())


def test_the_entry_point_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "chromoformer_hip.h")).read()
    assert re.search(r"int\s+cf_backward_from_inputs\s*\(", hdr) and "typedef struct cf_input_grads" in hdr
    from chromoformer_amd import _lib
    assert "cf_backward_from_inputs" in _lib.SYMBOLS
    assert [n for n, _ in _lib.cf_input_grads._fields_] == ["promoter_feats", "pcre_feats", "interaction_freq"]
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT cf_backward_from_inputs$", out, re.M)
