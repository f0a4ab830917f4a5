"""Generate tests/golden/unstructured.npz by IMPORTING the reference (same setup as make_goldens.py).

The reference's forward, loss and backward, seed-42 weights, classifier and regressor, on tests.unstructured_inputs.unstructured_batch(
4, seed=SEED): dense signed interaction frequencies, unsymmetric per-resolution interaction masks with fully masked rows, pad masks
with holes / single valid bins / fully masked slots and random non-centre rows, features non-zero under the masks.  Results only --
the tests regenerate the inputs from the seed:
  <head>.logits, <head>.loss                 forward and CrossEntropy / MSE loss
  <head>.grad_norms, names                   Frobenius norm of every parameter gradient of the loss (NaN: never receives one)
  <head>.grad.<name>                         in full: every Regulation gamma_f, the lin_proj* weights, fc_head
  <head>.freq_grad                           interaction_freq.grad of logits[:, 1].sum() (classifier) / logits[:, 0].sum() (regressor)
The oracle has to agree before anything is written.  Runs only where the reference is present:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_unstructured_goldens.py
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
from tests.helpers import referee_oracle  # noqa: E402
from tests.unstructured_inputs import SEED, unstructured_batch  # noqa: E402

B = 4
torch.set_num_threads(8)


def in_full(name):
    return name.endswith("gamma_f") or "lin_proj" in name or name.startswith("fc_head")


def ref_call(model, batch, freq):
    return model(batch["promoter_feats"], batch["promoter_pad_masks"], batch["pcre_feats"], batch["pcre_pad_masks"],
                 batch["interaction_masks"], freq)


def main():
    arrs = {}
    for head, Model, col in (("clf", ChromoformerClassifier, 1), ("reg", ChromoformerRegressor, 0)):
        reg = head == "reg"
        batch = unstructured_batch(B, seed=SEED, regression=reg)
        model = Model(seed=42)
        logits = ref_call(model, batch, batch["interaction_freq"])
        crit = torch.nn.MSELoss() if reg else torch.nn.CrossEntropyLoss()
        loss = crit(logits, batch["label"].view(-1, 1) if reg else batch["label"])
        loss.backward()
        names = [k for k, _ in model.named_parameters()]
        grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.named_parameters()}
        freq = batch["interaction_freq"].clone().requires_grad_(True)
        ref_call(model, batch, freq)[:, col].sum().backward()
        # the oracle on the same inputs
        P = orc.init_params(None, 42, reg)
        assert list(P) == names
        ol, oloss, og = referee_oracle(P, batch, reg, torch.float32)
        assert (ol - logits.detach()).abs().max().item() < 1e-6 and abs(oloss - float(loss)) < 1e-6
        assert sorted(og) == sorted(k for k, g in grads.items() if g is not None)
        worst = max(((og[k] - g).norm() / g.norm()).item() for k, g in grads.items() if g is not None)
        assert worst < 5e-4, worst
        ofreq = batch["interaction_freq"].clone().requires_grad_(True)
        orc.forward(P, dict(batch, interaction_freq=ofreq))[:, col].sum().backward()
        dfreq = ((ofreq.grad - freq.grad).norm() / freq.grad.norm()).item()
        assert dfreq < 1e-4, dfreq
        print("%s: loss %.6f, oracle against the reference: worst gradient %.2e (relative Frobenius), freq grad %.2e" % (head, float(loss), worst, dfreq))
        arrs["%s.logits" % head] = logits.detach().numpy()
        arrs["%s.loss" % head] = np.float64(loss.item())
        arrs["%s.grad_norms" % head] = np.array([np.nan if grads[k] is None else grads[k].double().norm().item() for k in names])
        arrs["%s.freq_grad" % head] = freq.grad.numpy()
        for k in names:
            if grads[k] is not None and in_full(k):
                arrs["%s.grad.%s" % (head, k)] = grads[k].numpy()
    arrs["names"] = np.array(names)
    arrs["seed"], arrs["B"] = np.array(SEED), np.array(B)
    path = os.path.join(HERE, "unstructured.npz")
    np.savez_compressed(path, **arrs)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
