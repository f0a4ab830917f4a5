"""Generate tests/golden/mark_donor.npz by IMPORTING the reference (same setup as make_mark_coalition_goldens.py).

Histone-mark coalitions against a donor cell type as their definition reads: the raw .npy regions of a gene are rewritten with the
rows of every absent player's marks taken from the donor's file of the same name (tests.donor_oracle.donor_dataset, seed
DONOR_SEED), and the reference's own ChromoformerDataset (w_prom = 39000) and seed-42 models, classifier and regressor, run on
them.  Three genes of tests.scan_oracle.scan_dataset (a '-' strand gene with a 12,201-sample pCRE, a '+' strand gene with an
1,800-sample pCRE, a gene without partners), six (players, word) cases; per case the logits of the rewritten genes, [B, n_out], and
once the unperturbed ones.  The oracle of tests/donor_oracle.py must reproduce them before anything is written.  Runs only where the
reference is present, its checkout named by CHROMOFORMER_REFERENCE:

    PYTHONDONTWRITEBYTECODE=1 CHROMOFORMER_REFERENCE=<checkout> python tests/golden/make_mark_donor_goldens.py
"""
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ["CHROMOFORMER_REFERENCE"]
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.Tensor.cuda = lambda self, *a, **k: self
torch.nn.Module.cuda = lambda self, *a, **k: self
sys.modules.setdefault("wandb", types.ModuleType("wandb"))

from chromoformer.data import ChromoformerDataset  # noqa: E402
from chromoformer.net import ChromoformerClassifier, ChromoformerRegressor  # noqa: E402

from chromoformer_amd.attribution import mark_players  # noqa: E402
from oracle import chromoformer_oracle as orc  # noqa: E402
from tests import donor_oracle as do  # noqa: E402
from tests import mark_oracle as mo  # noqa: E402
from tests import scan_oracle as so  # noqa: E402

W_PROM = 39000
GENES = ["ENSGSYN00001", "ENSGSYN00000", "ENSGSYN00002"]
OVERLAP = [((0, 1), (0, 1)), ((1, 2), (0, 2))]      # mark 1 of the promoter belongs to both players
CASES = [  # players, word (bit p set: player p present)
    ("marks", 0x7F & ~(1 << 3)),
    ("marks", 0x00),
    ("marks", 0x25),
    ("compartments", 0x3FFF & ~(1 << 1) & ~(1 << 11) & ~(1 << 12)),
    ("regions", 0x1FF & ~1 & ~(1 << 2)),
    (OVERLAP, 0x0),
]
torch.set_num_threads(8)


def ref_logits(model, b):
    with torch.no_grad():
        return model(b["promoter_feats"], b["promoter_pad_masks"], b["pcre_feats"], b["pcre_pad_masks"], b["interaction_masks"],
                     b["interaction_freq"])


def main():
    arrs = {"w_prom": np.int64(W_PROM), "genes": np.array(GENES), "donor_seed": np.int64(do.DONOR_SEED), "n_players": [], "player_marks": [],
            "player_regions": [], "words": np.array([w for _, w in CASES], dtype=np.uint32)}
    with tempfile.TemporaryDirectory() as tmp, tempfile.TemporaryDirectory() as dtmp:
        mine = so.scan_dataset(tmp, w_prom=W_PROM)
        donor = do.donor_dataset(tmp, dtmp, do.DONOR_SEED, w_prom=W_PROM)
        meta = os.path.join(tmp, "meta.csv")
        base_mine, base_donor = so.dataset_batch(mine, GENES), so.dataset_batch(donor, GENES)

        def ref_batch():
            ds = ChromoformerDataset(meta, tmp, GENES, w_prom=W_PROM)
            return torch.utils.data.default_collate([ds[i] for i in range(len(GENES))])

        models = {"clf": ChromoformerClassifier().eval(), "reg": ChromoformerRegressor().eval()}
        for h, m in models.items():
            arrs["base." + h] = ref_logits(m, ref_batch()).numpy().astype(np.float32)
        out = {h: [] for h in models}
        for spec, word in CASES:
            marks, regions, _ = mark_players(spec, 7, 8)
            P = len(marks)
            arrs["n_players"].append(P)
            arrs["player_marks"].append(np.pad(marks, (0, 16 - P)))
            arrs["player_regions"].append(np.pad(regions, (0, 16 - P)))
            gone = mo.gone_words(marks, regions, word, 9)
            kept = {}
            for gid in GENES:                                                  # rewrite every region file of the gene
                chrom, tss, _ = mine.genes[gid]["tss"]
                for rho, reg in enumerate([(chrom, tss - 20000, tss + 20000)] + [tuple(p) for p in mine.genes[gid]["pcres"]]):
                    rows = [f for f in range(7) if gone[rho] >> f & 1]
                    if not rows:
                        continue
                    name = "%s:%d-%d.npy" % reg
                    path = os.path.join(tmp, name)
                    a = np.load(path)
                    kept[path] = a
                    b = a.copy()
                    b[rows] = np.load(os.path.join(dtmp, name))[rows]
                    np.save(path, b)
            try:
                pert = ref_batch()
            finally:
                for path, a in kept.items():
                    np.save(path, a)
            for h, m in models.items():
                ref = ref_logits(m, pert)
                ora = do.oracle_donor_coalitions(orc.init_params(None, 42, h == "reg"), base_mine, base_donor, (marks, regions), [word])[:, 0]
                d = (ora - ref).abs().max().item()
                assert d < 1e-5, (h, spec, word, d)
                print(h, spec if isinstance(spec, str) else "overlap", hex(word),
                      "oracle vs reference %.2e; effect %.2e" % (d, (ref - torch.from_numpy(arrs["base." + h])).abs().max().item()))
                out[h].append(ref.numpy().astype(np.float32))
        for h in models:
            arrs[h] = np.stack(out[h])
    for k in ("n_players", "player_marks", "player_regions"):
        arrs[k] = np.array(arrs[k], dtype=np.uint32)
    path = os.path.join(HERE, "mark_donor.npz")
    np.savez_compressed(path, **arrs)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
