"""Generate tests/golden/fine_window.npz by IMPORTING the reference (same setup as make_mark_window_goldens.py).

The fine window game as its definition reads: the raw .npy region of a gene is rewritten with the samples of every absent player's marks
INSIDE the player's window of FINEST bins (100 bp, relative to a per-gene start) multiplied by s -- once, however many absent players
cover a sample -- or replaced by the donor cell type's samples (tests/donor_oracle.donor_dataset), and the reference's own
ChromoformerDataset (w_prom = 39000) and seed-42 models, classifier and regressor, run on it.  The three genes of
make_fine_scan_goldens.py, six cases, among them two overlapping absent players at once, mark x window cells, the tails of both pCREs
and one donor case; per case the logits of the edited genes, [B, n_out], and once the unedited ones.  The players travel as one table,
a row (case, marks word, lo, hi, present) per player.  The oracle of tests/fine_window_oracle.py (the rule on the stored features)
must reproduce the logits within the project's 1e-4 before anything is written.  Runs only where the reference is present, its
checkout named by CHROMOFORMER_REFERENCE:

    PYTHONDONTWRITEBYTECODE=1 CHROMOFORMER_REFERENCE=<checkout> python tests/golden/make_fine_window_goldens.py
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

from oracle import chromoformer_oracle as orc  # noqa: E402
from tests import donor_oracle as do  # noqa: E402
from tests import fine_window_oracle as fw  # noqa: E402
from tests import scan_oracle as so  # noqa: E402

W_PROM = 39000
GENES = ["ENSGSYN00001", "ENSGSYN00000", "ENSGSYN00002"]
F = 7
ALL = tuple(range(F))
TOL = 1e-4


def present(P, *gone):
    return [p not in gone for p in range(P)]


CASES = [  # region, start per gene, players, present, scale, donor rule
    (0, [0, 0, 0], fw.windows_players(F, 2, 5), present(5, 0), 0.0, False),            # the first 200 bp: the LAST real rows of the mirrored promoter
    (0, [380, 190, 100], [((1, 4), (0, 7)), ((0, 1, 2), (5, 12)), (ALL, (18, 23))], present(3, 0, 1), 0.0, False),      # two overlapping absent
    (0, [195, 195, 195], fw.cells_players(F, 2, 5), present(35, 3, 8, 9, 17, 31, 32, 34), 2.5, False),                   # cells across bin 200
    (1, [115, 13, 0], fw.windows_players(F, 3, 3), present(3, 0, 2), 0.0, False),      # the tails of the 12,201- and the 1,800-sample pCRE
    (0, [200, 60, 381], [((1, 4), (0, 7)), (ALL, (9, 11))], present(2, 0, 1), 0.0, True),      # the donor rule, two absent players
    (1, [0, 0, 0], [(ALL, (0, 5)), ((2, 5), (3, 30))], present(2, 0, 1), 0.5, False),
]
torch.set_num_threads(8)


def ref_logits(model, b):
    with torch.no_grad():
        return model(b["promoter_feats"], b["promoter_pad_masks"], b["pcre_feats"], b["pcre_pad_masks"], b["interaction_masks"],
                     b["interaction_freq"])


def main():
    table = [(k, sum(1 << f for f in ms), lo, hi, int(here)) for k, (_, _, players, pres, _, _) in enumerate(CASES)
             for (ms, (lo, hi)), here in zip(players, pres)]
    arrs = {"w_prom": np.int64(W_PROM), "genes": np.array(GENES), "players": np.array(table, dtype=np.int32),
            "regions": np.array([c[0] for c in CASES], dtype=np.int64), "starts": np.array([c[1] for c in CASES], dtype=np.int64),
            "scales": np.array([c[4] for c in CASES], dtype=np.float64), "donor": np.array([c[5] for c in CASES]),
            "donor_seed": np.int64(do.DONOR_SEED)}
    worst = 0.0
    with tempfile.TemporaryDirectory() as tmp, tempfile.TemporaryDirectory() as dtmp:
        mine = so.scan_dataset(tmp, w_prom=W_PROM)
        donor_ds = do.donor_dataset(tmp, dtmp, do.DONOR_SEED, w_prom=W_PROM)
        meta = os.path.join(tmp, "meta.csv")
        base_mine, donor_mine = so.dataset_batch(mine, GENES), so.dataset_batch(donor_ds, GENES)
        flips = [mine.genes[g]["tss"][2] != "+" for g in GENES]

        def ref_batch():
            ds = ChromoformerDataset(meta, tmp, GENES, w_prom=W_PROM)
            return torch.utils.data.default_collate([ds[i] for i in range(len(GENES))])

        models = {"clf": ChromoformerClassifier().eval(), "reg": ChromoformerRegressor().eval()}
        for h, m in models.items():
            arrs["base." + h] = ref_logits(m, ref_batch()).numpy().astype(np.float32)
        out = {h: [] for h in models}
        lengths = []
        for k, (region, starts, players, pres, scale, donor) in enumerate(CASES):
            kept, lens = {}, []
            for i, gid in enumerate(GENES):                                    # rewrite the region's file of every gene that has it
                chrom, tss, _ = mine.genes[gid]["tss"]
                reg = (chrom, tss - 20000, tss + 20000) if region == 0 else (mine.genes[gid]["pcres"][region - 1:region] or [None])[0]
                if reg is None:
                    lens.append(0)
                    continue
                name = "%s:%d-%d.npy" % tuple(reg)
                path = os.path.join(tmp, name)
                a = np.load(path)
                kept[path] = a
                lens.append(W_PROM if region == 0 else a.shape[1])
                d = np.load(os.path.join(dtmp, name)) if donor else None
                np.save(path, fw.edit_raw(a, players, pres, starts[i], 100, scale, d, W_PROM if region == 0 else None))
            lengths.append(lens)
            try:
                pert = ref_batch()
            finally:
                for path, a in kept.items():
                    np.save(path, a)
            for h, m in models.items():
                ref = ref_logits(m, pert)
                ora, _, kinds, _ = fw.oracle_fine_window(orc.init_params(None, 42, h == "reg"), base_mine, players, [pres], region=region, start=starts,
                                                         lengths=lens, flip=flips if region == 0 else None, scale=scale,
                                                         donor=donor_mine if donor else None)
                d = (ora[:, 0] - ref).abs().max().item()
                worst = max(worst, d)
                assert d < TOL, (h, k, d)
                assert any((kinds[b] == fw.PART).any() for b in kinds)
                print(h, "case", k, "oracle vs reference %.2e; effect %.2e" % (d, (ref - torch.from_numpy(arrs["base." + h])).abs().max().item()))
                out[h].append(ref.numpy().astype(np.float32))
        for h in models:
            arrs[h] = np.stack(out[h])
        arrs["lengths"] = np.array(lengths, dtype=np.int64)
    path = os.path.join(HERE, "fine_window.npz")
    np.savez_compressed(path, **arrs)
    print("worst oracle vs reference %.2e" % worst)
    print("wrote", path, "%d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
