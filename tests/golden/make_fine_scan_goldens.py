"""Generate tests/golden/fine_scan.npz by IMPORTING the reference (same setup as make_perturbation_scan_goldens.py).

The fine-resolution perturbation scan as its definition reads: the raw .npy region of a gene is rewritten with the samples of a window
of FINEST bins (100 bp) multiplied by s for the marks of a set, and the reference's own ChromoformerDataset (w_prom = 39000) and
seed-42 models, classifier and regressor, run on it.  The three genes of make_perturbation_scan_goldens.py (a '-' strand gene with a
12,201-sample pCRE, a '+' strand gene with an 1,800-sample pCRE, a gene without partners), six (region, lo, hi, scale, marks) cases;
per case the logits of the unperturbed and of the perturbed genes, [B, 2, n_out].  The oracle of tests/fine_scan_oracle.py (the rule on
the stored features, partly covered bins recomputed from their finest children) must reproduce them within the project's 1e-4 before
anything is written; observed: 2.68e-07 at most over the six cases and both heads (the windows move the logits by 1.7e-05 to
1.95e-02).  Runs only where the reference is present:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_fine_scan_goldens.py
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
import torch  # noqa: E402

torch.Tensor.cuda = lambda self, *a, **k: self
torch.nn.Module.cuda = lambda self, *a, **k: self
sys.modules.setdefault("wandb", types.ModuleType("wandb"))

from chromoformer.data import ChromoformerDataset  # noqa: E402
from chromoformer.net import ChromoformerClassifier, ChromoformerRegressor  # noqa: E402

from oracle import chromoformer_oracle as orc  # noqa: E402
from tests import fine_scan_oracle as fo  # noqa: E402
from tests import scan_oracle as so  # noqa: E402

W_PROM = 39000
GENES = ["ENSGSYN00001", "ENSGSYN00000", "ENSGSYN00002"]
ALL = tuple(range(7))
CASES = [  # (region, lo, hi, scale) in finest bins, marks
    ((0, 0, 1, 0.0), ALL),           # the first 100 bp: the LAST real row of the mirrored '-' strand promoter
    ((0, 383, 390, 0.0), (1, 4)),    # inside the short last coarse bin (ten children)
    ((0, 197, 204, 2.5), (0,)),      # across bin 200: a boundary at 500 bp and at 2 kb
    ((1, 0, 3, 0.0), ALL),
    ((1, 118, 123, 2.5), (2, 5)),    # the tail of the 12,201-sample pCRE: its last finest bin holds one sample
    ((1, 15, 18, 0.0), ALL),         # the tail of the 1,800-sample pCRE; an inner stretch of the other
]
TOL = 1e-4
torch.set_num_threads(8)


def ref_logits(model, b):
    with torch.no_grad():
        return model(b["promoter_feats"], b["promoter_pad_masks"], b["pcre_feats"], b["pcre_pad_masks"], b["interaction_masks"],
                     b["interaction_freq"])


def main():
    arrs = {"w_prom": np.int64(W_PROM), "genes": np.array(GENES), "cases": np.array([c for c, _ in CASES], dtype=np.float64),
            "marks": np.array([[f in m for f in range(7)] for _, m in CASES])}
    worst = 0.0
    with tempfile.TemporaryDirectory() as tmp:
        mine = so.scan_dataset(tmp, w_prom=W_PROM)
        meta = os.path.join(tmp, "meta.csv")
        base_mine = so.dataset_batch(mine, GENES)
        flips = [mine.genes[g]["tss"][2] != "+" for g in GENES]

        def ref_batch():
            ds = ChromoformerDataset(meta, tmp, GENES, w_prom=W_PROM)
            return torch.utils.data.default_collate([ds[i] for i in range(len(GENES))])

        models = {"clf": ChromoformerClassifier().eval(), "reg": ChromoformerRegressor().eval()}
        base = {h: ref_logits(m, ref_batch()) for h, m in models.items()}
        out = {h: [] for h in models}
        lengths = []
        for (region, lo, hi, scale), marks in CASES:
            kept, lens = {}, []
            for gid in GENES:                                                  # rewrite the region's file of every gene that has it
                chrom, tss, _ = mine.genes[gid]["tss"]
                reg = (chrom, tss - 20000, tss + 20000) if region == 0 else (mine.genes[gid]["pcres"][region - 1:region] or [None])[0]
                if reg is None:
                    lens.append(0)
                    continue
                path = os.path.join(tmp, "%s:%d-%d.npy" % reg)
                a = np.load(path)
                kept[path] = a
                col0, ncols = (20000 - W_PROM // 2, W_PROM) if region == 0 else (0, a.shape[1])
                lens.append(ncols)
                c0, c1 = col0 + min(lo * 100, ncols), col0 + min(hi * 100, ncols)
                b = a.astype(np.float32)
                if c0 < c1:
                    b[list(marks), c0:c1] *= np.float32(scale)
                np.save(path, b)
            lengths.append(lens)
            try:
                pert = ref_batch()
            finally:
                for path, a in kept.items():
                    np.save(path, a)
            for h, m in models.items():
                ref = torch.stack([base[h], ref_logits(m, pert)], 1)
                ora, _, kinds = fo.oracle_fine(orc.init_params(None, 42, h == "reg"), base_mine, region=region, scale=scale, width=hi - lo, start=lo,
                                               n_windows=1, mark_sets=[marks], lengths=lens, flip=flips if region == 0 else None)
                d = (ora - ref).abs().max().item()
                worst = max(worst, d)
                assert d < TOL, (h, region, lo, hi, d)
                assert any((kinds[b] == fo.PART).any() for b in kinds)
                print(h, (region, lo, hi, scale), marks, "oracle vs reference %.2e; effect %.2e" % (d, (ref[:, 1] - ref[:, 0]).abs().max().item()))
                out[h].append(ref.numpy().astype(np.float32))
        for h in models:
            arrs[h] = np.stack(out[h])
        arrs["lengths"] = np.array(lengths, dtype=np.int64)
    path = os.path.join(HERE, "fine_scan.npz")
    np.savez_compressed(path, **arrs)
    print("worst oracle vs reference %.2e" % worst)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
