"""Attention maps without a GPU: the recording oracle (tests/attn_oracle.py, a patch of orc._attend) reproduces the reference's att_prob
rows, fc_head input and logits (tests/golden/attention_maps.npz) -- which pins the referee test_attention_maps_gpu.py judges the HIP path
by -- and cf_attention_maps / cf_attn_maps are declared, exported and bound."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from oracle import chromoformer_oracle as orc
from tests.attn_oracle import oracle_maps
from tests.helpers import GOLDEN, load_npz_batch

BINS = (2000, 500, 100)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("regression", [False, True], ids=["classifier", "regressor"])
@pytest.mark.parametrize("tag", ["kat", "real"])
def test_oracle_attention_maps_reproduce_the_reference(tag, regression):
    z = np.load(os.path.join(GOLDEN, "attention_maps.npz"))
    batch = load_npz_batch("kat.npz")[0] if tag == "kat" else orc.synthetic_batch(8, seed=31, regime="realistic")
    head = "reg" if regression else "clf"
    genes = list(z["%s.genes" % tag])
    logits, maps = oracle_maps(orc.init_params(None, 42, regression), batch)
    for k, v in maps.items():
        ref = torch.from_numpy(z["%s.%s.%s" % (tag, head, k)])
        got = v[genes] if k.startswith(("embed.", "pairwise_interaction.")) else v
        assert got.shape == ref.shape, k
        assert (got - ref).abs().max().item() < 2e-6, k
    assert (logits - torch.from_numpy(z["%s.%s.logits" % (tag, head)])).abs().max().item() < 1e-5
    if tag == "real":      # gene 7 holds one pCRE and seven dummy slots, gene 1 none: masked keys are exact zeros, dummy rows uniform
        for b in BINS:
            pw = z["real.%s.pairwise_interaction.%d" % (head, b)]
            L = pw.shape[-1]
            assert np.allclose(pw[0], 1.0 / L, atol=1e-7) and np.allclose(pw[1][:, 1:], 1.0 / L, atol=1e-7)      # genes [1, 7]
            rg = z["real.%s.regulation.%d" % (head, b)]
            assert (rg[7, :, :, 2:] == 0).all() and (rg[1, :, :, 1:] == 0).all() and np.allclose(rg[1, :, :, 0], 1.0)


def test_the_entry_point_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "chromoformer_hip.h")).read()
    assert re.search(r"int\s+cf_attention_maps\s*\(", hdr) and "typedef struct cf_attn_maps" in hdr
    from chromoformer_amd import _lib
    assert "cf_attention_maps" in _lib.SYMBOLS
    assert [n for n, _ in _lib.cf_attn_maps._fields_] == ["embed", "pairwise", "regulation", "embedding"]
    from chromoformer_amd import ChromoformerClassifier
    from chromoformer_amd.net import Chromoformer
    assert Chromoformer.attention_maps is ChromoformerClassifier.attention_maps
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT cf_attention_maps$", out, re.M)
