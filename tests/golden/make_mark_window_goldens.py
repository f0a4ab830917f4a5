"""Generate tests/golden/mark_windows.npz by IMPORTING the reference (same setup as make_mark_coalition_goldens.py).

The window game as its definition reads: the raw .npy regions of a gene are rewritten with the samples of every absent player's marks
multiplied by s INSIDE the player's window of coarse bins (once, however many absent players cover a sample), and the reference's own
ChromoformerDataset (w_prom = 39000) and seed-42 models, classifier and regressor, run on them.  The three genes of
make_mark_coalition_goldens.py, six (players, word, scale) cases; per case the logits of the edited genes, [B, n_out], and once the
unedited ones.  The players travel as one table, a row (case, marks word, regions word, lo, hi, present) per player.  The oracle of
tests/window_oracle.py must reproduce the logits before anything is written.  Runs only where the reference is present, its checkout
named by CHROMOFORMER_REFERENCE:

    PYTHONDONTWRITEBYTECODE=1 CHROMOFORMER_REFERENCE=<checkout> python tests/golden/make_mark_window_goldens.py
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
from tests import scan_oracle as so  # noqa: E402
from tests import window_oracle as wo  # noqa: E402

W_PROM = 39000
GENES = ["ENSGSYN00001", "ENSGSYN00000", "ENSGSYN00002"]
F, S, W, BC = 7, 8, 20, 2000
ALL = tuple(range(F))


def absent(P, *gone):
    return wo.full_word(P) & ~sum(1 << p for p in gone)


CASES = [  # players, word (bit p set: player p present), scale
    (wo.players_promoter(F, W, 4), absent(5, 1, 2), 0.0),                                      # two adjacent stretches of the promoter
    (wo.players_promoter_cells(F, W, 4), absent(35, 3, 8, 17, 31, 32, 34), 0.0),               # marks in stretches; the short last bin
    (wo.players_regions(F, S, W, 5), absent(36, 0, 4, 5, 9, 35), 0.5),                         # pCRE windows, some past the pCRE's end
    ([((0, 1), (0, 1), (2, 7)), ((1, 2), (0,), (5, 12))], 0, 2.5),                             # overlap: covered samples scaled once
    (wo.players_promoter(F, W, 1), absent(20, 19), 0.0),                                       # the narrowed promoter's half bin alone
    (wo.players_regions(F, S, W, 20), 0, 0.0),                                                 # whole regions: everything erased
]
torch.set_num_threads(8)


def ref_logits(model, b):
    with torch.no_grad():
        return model(b["promoter_feats"], b["promoter_pad_masks"], b["pcre_feats"], b["pcre_pad_masks"], b["interaction_masks"],
                     b["interaction_freq"])


def main():
    table = [(k, sum(1 << f for f in ms), sum(1 << r for r in rs), lo, hi, word >> p & 1)
             for k, (players, word, _) in enumerate(CASES) for p, (ms, rs, (lo, hi)) in enumerate(players)]
    arrs = {"w_prom": np.int64(W_PROM), "genes": np.array(GENES), "players": np.array(table, dtype=np.int16),
            "scales": np.array([s for _, _, s in CASES], dtype=np.float64)}
    with tempfile.TemporaryDirectory() as tmp:
        mine = so.scan_dataset(tmp, w_prom=W_PROM)
        meta = os.path.join(tmp, "meta.csv")
        base_mine = so.dataset_batch(mine, GENES)
        flips = [mine.genes[g]["tss"][2] != "+" for g in GENES]

        def ref_batch():
            ds = ChromoformerDataset(meta, tmp, GENES, w_prom=W_PROM)
            return torch.utils.data.default_collate([ds[i] for i in range(len(GENES))])

        models = {"clf": ChromoformerClassifier().eval(), "reg": ChromoformerRegressor().eval()}
        for h, m in models.items():
            arrs["base." + h] = ref_logits(m, ref_batch()).numpy().astype(np.float32)
        out = {h: [] for h in models}
        for k, (players, word, scale) in enumerate(CASES):
            gone = wo.gone_table(players, word, S + 1, W)
            kept = {}
            for gid in GENES:                                                  # rewrite the region files of the gene
                chrom, tss, _ = mine.genes[gid]["tss"]
                for rho, reg in enumerate([(chrom, tss - 20000, tss + 20000)] + [tuple(p) for p in mine.genes[gid]["pcres"]][:S]):
                    if not any(gone[rho]):
                        continue
                    path = os.path.join(tmp, "%s:%d-%d.npy" % reg)
                    a = np.load(path)
                    kept[path] = a
                    b = a.astype(np.float32)
                    col0, ncols = (20000 - W_PROM // 2, W_PROM) if rho == 0 else (0, a.shape[1])
                    for g in range(W):
                        lo, hi = col0 + g * BC, col0 + min((g + 1) * BC, ncols)
                        if gone[rho][g] and lo < hi:
                            b[sorted(gone[rho][g]), lo:hi] *= np.float32(scale)
                    np.save(path, b)
            try:
                pert = ref_batch()
            finally:
                for path, a in kept.items():
                    np.save(path, a)
            for h, m in models.items():
                ref = ref_logits(m, pert)
                with torch.no_grad():
                    ora = orc.forward(orc.init_params(None, 42, h == "reg"), wo.edited_batch(base_mine, players, word, scale, flip=flips))
                d = (ora - ref).abs().max().item()
                assert d < 1e-5, (h, k, d)
                print(h, "case", k, "oracle vs reference %.2e; effect %.2e" % (d, (ref - torch.from_numpy(arrs["base." + h])).abs().max().item()))
                out[h].append(ref.numpy().astype(np.float32))
        for h in models:
            arrs[h] = np.stack(out[h])
    path = os.path.join(HERE, "mark_windows.npz")
    np.savez_compressed(path, **arrs)
    print("wrote", path, "%d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
