"""The oracle of the contact games (ChromoformerBase.contact_coalitions / contact_shapley / ...): the rule of
include/chromoformer_hip.h in plain torch on a batch dict.

  * contact_batch: the batch of one coalition word -- for the absent players the interaction-mask row and column j + 1 of every slot j
    they drop set at every resolution (tests/coalition_oracle.coalition_masks' rule), and every entry of interaction_freq in row or
    column j + 1 of every slot j whose contact they hold edited ONCE: scale * f in float32 (one multiplication), or the donor's entry;
  * oracle_contact_coalitions: orc.forward on those batches, one pass per word.

Used by the contact tests and by tests/golden/make_contact_goldens.py."""
import torch

from oracle import chromoformer_oracle as orc


def gone_words(word, drop, contact):
    """-> (D, C): the OR of drop_p / contact_p over the players whose bit of `word` is clear."""
    D = C = 0
    for p, (d, c) in enumerate(zip(drop, contact)):
        if not int(word) >> p & 1:
            D |= int(d)
            C |= int(c)
    return D, C


def contact_batch(batch, word, drop, contact, scale=0.0, donor_freq=None):
    """The batch edited for coalition `word` (bit p set: player p present) of the players (drop[p], contact[p]) -> a new batch dict."""
    P = len(drop)
    assert len(contact) == P and 0 <= int(word) < 1 << P
    out = {k: ({b: t.clone() for b, t in v.items()} if isinstance(v, dict) else v.clone()) for k, v in batch.items()}
    T = out["interaction_freq"].shape[-1]
    D, C = gone_words(word, drop, contact)
    assert not D >> (T - 1) and not C >> (T - 1)
    gone = [j + 1 for j in range(T - 1) if D >> j & 1]
    for im in out["interaction_masks"].values():
        im[:, 0, gone, :] = True
        im[:, 0, :, gone] = True
    hit = torch.zeros(T, T, dtype=torch.bool)
    for j in range(T - 1):
        if C >> j & 1:
            hit[j + 1, :] = True
            hit[:, j + 1] = True
    f = batch["interaction_freq"]
    assert f.dtype == torch.float32
    if donor_freq is None:
        edited = torch.tensor(scale, dtype=torch.float32) * f      # one fp32 multiplication per entry
    else:
        edited = donor_freq.to(torch.float32).reshape(f.shape)
    out["interaction_freq"] = torch.where(hit.to(f.device), edited.to(f.device), f)
    return out


def oracle_contact_coalitions(P, batch, keep, drop, contact, scale=0.0, donor_freq=None, cfg=None):
    """-> logits [B, n_coal, n_out]: orc.forward on contact_batch, one pass per word of `keep`."""
    with torch.no_grad():
        return torch.stack([orc.forward(P, contact_batch(batch, m, drop, contact, scale, donor_freq), cfg) for m in keep], 1)
