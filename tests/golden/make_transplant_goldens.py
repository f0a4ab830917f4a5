"""Generate tests/golden/transplant.npz by IMPORTING the reference (same setup as make_perturbation_scan_goldens.py).

The pCRE transplant as its definition reads: the partner list of a gene's metadata row is edited -- a partner replaced by another
region, or one appended, with a contact score f -- and the reference's own ChromoformerDataset (w_prom = 39000) and seed-42 models
run on the gene.  Six cases on tests.scan_oracle.scan_dataset, chosen from its metadata: a partner replaced by another gene's enhancer;
a partner appended to a two-partner gene; one appended to a gene without partners; a '-' strand gene; an 1,800-sample candidate; the
regressor.  Per case the gene, the slot, the candidate's coordinates, f and the logits of the unedited and of the edited gene,
[2, n_out].  The oracle of tests/transplant_oracle.py must reproduce the edited item bit for bit and the logits before anything is
written.  Runs only where the reference is present:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_transplant_goldens.py
"""
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402
import torch  # noqa: E402

torch.Tensor.cuda = lambda self, *a, **k: self
torch.nn.Module.cuda = lambda self, *a, **k: self
sys.modules.setdefault("wandb", types.ModuleType("wandb"))

from chromoformer.data import ChromoformerDataset  # noqa: E402
from chromoformer.net import ChromoformerClassifier, ChromoformerRegressor  # noqa: E402

from oracle import chromoformer_oracle as orc  # noqa: E402
from tests import scan_oracle as so  # noqa: E402
from tests import transplant_oracle as to  # noqa: E402
from tests.transplant_cases import choose_cases, edited_meta, oracle_candidate  # noqa: E402

W_PROM = 39000
torch.set_num_threads(8)


def ref_logits(model, b):
    with torch.no_grad():
        return model(b["promoter_feats"], b["promoter_pad_masks"], b["pcre_feats"], b["pcre_pad_masks"], b["interaction_masks"],
                     b["interaction_freq"])


def main():
    with tempfile.TemporaryDirectory() as tmp:
        mine = so.scan_dataset(tmp, w_prom=W_PROM)
        table = pd.read_csv(os.path.join(tmp, "meta.csv"))
        cases = choose_cases(mine)
        models = {False: ChromoformerClassifier().eval(), True: ChromoformerRegressor().eval()}
        out = {False: [], True: []}
        for name, gid, slot, cand, f, regression in cases:
            def ref_item(meta):
                path = os.path.join(tmp, "meta_case.csv")
                meta.to_csv(path, index=False)
                ds = ChromoformerDataset(path, tmp, [gid], w_prom=W_PROM)
                return torch.utils.data.default_collate([ds[0]])

            base, edit = ref_item(table), ref_item(edited_meta(table, gid, slot, cand, f))
            feats, cols = oracle_candidate(mine, cand)
            mine_edit = to.transplant(base, 0, feats, cols, f, slot)
            for k in to.KEYS:      # the oracle's edit of the reference's item is the reference's item of the edited metadata
                pairs = [(mine_edit[k][b], edit[k][b]) for b in edit[k]] if isinstance(edit[k], dict) else [(mine_edit[k], edit[k])]
                assert all(torch.equal(a, b) for a, b in pairs), (name, k)
            ref = torch.cat([ref_logits(models[regression], base), ref_logits(models[regression], edit)])
            P = orc.init_params(None, 42, regression)
            with torch.no_grad():
                ora = torch.cat([orc.forward(P, base), orc.forward(P, mine_edit)])
            d = (ora - ref).abs().max().item()
            assert d < 1e-5, (name, d)
            print("%-10s %s slot %d <- %s:%d-%d f = %g: oracle vs reference %.2e; effect %.2e" % (
                (name, gid, slot) + tuple(cand) + (f, d, (ref[1] - ref[0]).abs().max().item())))
            out[regression].append(ref.numpy().astype(np.float32))
    arrs = {"w_prom": np.int64(W_PROM), "names": np.array([c[0] for c in cases]), "genes": np.array([c[1] for c in cases]),
            "slots": np.array([c[2] for c in cases], dtype=np.int64), "cand_chrom": np.array([c[3][0] for c in cases]),
            "cand_start": np.array([c[3][1] for c in cases], dtype=np.int64), "cand_end": np.array([c[3][2] for c in cases], dtype=np.int64),
            "freq": np.array([c[4] for c in cases], dtype=np.float64), "regression": np.array([c[5] for c in cases]),
            "clf": np.stack(out[False]), "reg": np.stack(out[True])}
    path = os.path.join(HERE, "transplant.npz")
    np.savez_compressed(path, **arrs)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
