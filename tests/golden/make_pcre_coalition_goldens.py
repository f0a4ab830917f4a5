"""Generate tests/golden/pcre_coalitions.npz by IMPORTING the reference (same setup as make_pcre_ablation_goldens.py).

The logits of every pCRE coalition as the reference computes them, seed-42 weights, classifier and regressor, on the demo batch of
demo_subset.npz (6 genes with 0, 1, 5, 8, 8 and 3 pCREs): "demo.clf" [6, 256, 2] and "demo.reg" [6, 256, 1], indexed by the
coalition word m (bit j set: pCRE slot j kept; clear: interaction_masks row and column j + 1 set at every resolution).  Several
coalitions travel in one reference call, stacked along the batch dimension (the model is per-gene in eval mode).  The oracle of
tests/coalition_oracle.py must reproduce them to 1e-5 before anything is written.  Runs only where the reference is present:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_pcre_coalition_goldens.py
"""
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.Tensor.cuda = lambda self, *a, **k: self
torch.nn.Module.cuda = lambda self, *a, **k: self
sys.modules.setdefault("wandb", types.ModuleType("wandb"))

from chromoformer.net import ChromoformerClassifier, ChromoformerRegressor  # noqa: E402

from oracle import chromoformer_oracle as orc  # noqa: E402
from tests.coalition_oracle import coalition_masks, oracle_coalitions  # noqa: E402
from tests.helpers import load_npz_batch  # noqa: E402

S = 8
PER_CALL = 16      # coalitions per reference call
torch.set_num_threads(8)


def stacked(batch, words):
    """The batches of coalition_masks(batch, m, S) for m in words, concatenated along the batch dimension (coalition-major)."""
    parts = [coalition_masks(batch, m, S) for m in words]
    return {k: ({b: torch.cat([p[k][b] for p in parts]) for b in v} if isinstance(v, dict) else torch.cat([p[k] for p in parts]))
            for k, v in parts[0].items()}


def main():
    arrs = {}
    batch = {k: v for k, v in load_npz_batch("demo_subset.npz")[0].items() if k != "label"}
    B = batch["interaction_freq"].shape[0]
    words = list(range(1 << S))
    for head, Model in (("clf", ChromoformerClassifier), ("reg", ChromoformerRegressor)):
        torch.manual_seed(0)
        model = Model().eval()
        rows = []
        with torch.no_grad():
            for lo in range(0, len(words), PER_CALL):
                b = stacked(batch, words[lo:lo + PER_CALL])
                out = model(b["promoter_feats"], b["promoter_pad_masks"], b["pcre_feats"], b["pcre_pad_masks"], b["interaction_masks"],
                            b["interaction_freq"])
                rows.append(out.view(-1, B, out.shape[-1]).transpose(0, 1))      # [B, PER_CALL, n_out]
                print(head, lo, flush=True)
        ref = torch.cat(rows, 1)
        ora = oracle_coalitions(orc.init_params(None, 42, head == "reg"), batch, words)      # the oracle must agree before anything is written
        d = (ora - ref).abs().max().item()
        print(head, "oracle vs reference %.2e" % d, flush=True)
        assert d < 1e-5, (head, d)
        arrs["demo.%s" % head] = ref.numpy().astype(np.float32)
    path = os.path.join(HERE, "pcre_coalitions.npz")
    np.savez_compressed(path, **arrs)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
