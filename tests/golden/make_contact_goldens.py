"""Generate tests/golden/contact_games.npz by IMPORTING the reference (same setup as make_pcre_coalition_goldens.py).

The logits of contact-game coalitions as the reference computes them on the edited tensors of tests/contact_oracle.contact_batch,
seed-42 weights, on the demo batch of demo_subset.npz (6 genes with 0, 1, 5, 8, 8 and 3 pCREs):

    contacts0.clf            [6, 256, 2]   every word of players "contacts" at scale = 0, word m at column m (classifier)
    joint.words              [32]          32 fixed words of "pcres_and_contacts" (16 players; the first two: everybody, nobody)
    joint.clf / joint.reg    [6, 32, n_out]    ... at scale = 0
    words8                   [32]          32 fixed words of the 8 "contacts" players (the first two: everybody, nobody)
    half.clf / half.reg      [6, 32, n_out]    "contacts" at scale = 0.5 on words8
    donor.clf / donor.reg    [6, 32, n_out]    "contacts" under the donor rule on words8; the donor is the batch's interaction_freq
                                               rolled by one gene (torch.roll(freq, 1, 0))

Several coalitions travel in one reference call, stacked along the batch dimension (the model is per-gene in eval mode).  The oracle
(tests/contact_oracle.oracle_contact_coalitions) must reproduce every array to 1e-5 before anything is written.  Runs only where the
reference is present, in about 2 minutes on 8 CPU threads (116 s when the file was written):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_contact_goldens.py
"""
import os
import sys
import time
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

from chromoformer_amd.attribution import contact_players  # noqa: E402
from oracle import chromoformer_oracle as orc  # noqa: E402
from tests.contact_oracle import contact_batch, oracle_contact_coalitions  # noqa: E402
from tests.helpers import load_npz_batch  # noqa: E402

S = 8
PER_CALL = 16      # coalitions per reference call
torch.set_num_threads(8)


def fixed_words(P, seed):
    """32 words of P players: everybody, nobody, then 30 drawn once from a seeded stream."""
    rng = np.random.RandomState(seed)
    return np.array([(1 << P) - 1, 0] + [int(w) for w in rng.randint(0, 1 << P, 30)], dtype=np.uint32)


def reference_rows(model, batch, words, drop, contact, scale, donor):
    B = batch["interaction_freq"].shape[0]
    rows = []
    with torch.no_grad():
        for lo in range(0, len(words), PER_CALL):
            parts = [contact_batch(batch, m, drop, contact, scale, donor) for m in words[lo:lo + PER_CALL]]
            b = {k: ({r: torch.cat([p[k][r] for p in parts]) for r in v} if isinstance(v, dict) else torch.cat([p[k] for p in parts]))
                 for k, v in parts[0].items()}
            out = model(b["promoter_feats"], b["promoter_pad_masks"], b["pcre_feats"], b["pcre_pad_masks"], b["interaction_masks"],
                        b["interaction_freq"])
            rows.append(out.view(-1, B, out.shape[-1]).transpose(0, 1))
    return torch.cat(rows, 1)


def main():
    t0 = time.time()
    batch = {k: v for k, v in load_npz_batch("demo_subset.npz")[0].items() if k != "label"}
    donor = torch.roll(batch["interaction_freq"], 1, 0)
    contacts, joint = contact_players("contacts", S), contact_players("pcres_and_contacts", S)
    words8, words16 = fixed_words(8, 7), fixed_words(16, 8)
    arrs = {"joint.words": words16, "words8": words8}
    games = [("contacts0", contacts, np.arange(256, dtype=np.uint32), 0.0, None, ("clf",)),
             ("joint", joint, words16, 0.0, None, ("clf", "reg")),
             ("half", contacts, words8, 0.5, None, ("clf", "reg")),
             ("donor", contacts, words8, 0.0, donor, ("clf", "reg"))]
    for head, Model in (("clf", ChromoformerClassifier), ("reg", ChromoformerRegressor)):
        torch.manual_seed(0)
        model = Model().eval()
        P = orc.init_params(None, 42, head == "reg")
        for name, (drop, contact, _), words, scale, don, heads in games:
            if head not in heads:
                continue
            ref = reference_rows(model, batch, words, drop, contact, scale, don)
            ora = oracle_contact_coalitions(P, batch, words, drop, contact, scale, don)      # must agree before anything is written
            d = (ora - ref).abs().max().item()
            print("%s.%s oracle vs reference %.2e  (%.0f s)" % (name, head, d, time.time() - t0), flush=True)
            assert d < 1e-5, (name, head, d)
            arrs["%s.%s" % (name, head)] = ref.numpy().astype(np.float32)
    path = os.path.join(HERE, "contact_games.npz")
    np.savez_compressed(path, **arrs)
    print("wrote", path, "%.1f KB, %.0f s" % (os.path.getsize(path) / 1024, time.time() - t0))


if __name__ == "__main__":
    main()
