"""The oracle of in-silico pCRE deletion (ChromoformerBase.pcre_ablation): the contract's edited interaction masks, one orc.forward
per variant.  Also the two dataset-level edits the contract claims it equals (data.py:122, 200-209): slot j made a dummy, and pCRE j
removed with the later slots shifted left.  Used by the ablation tests and by tests/golden/make_pcre_ablation_goldens.py."""
import torch

from oracle import chromoformer_oracle as orc


def _copy(batch):
    return {k: ({b: t.clone() for b, t in v.items()} if isinstance(v, dict) else v.clone()) for k, v in batch.items()}


def variant_masks(batch, v, S):
    """The batch with every gene's interaction masks edited for variant v (0: as given; 1 + j: row and column j + 1 set; S + 1: rows
    and columns 1..S set)."""
    out = _copy(batch)
    if v == 0:
        return out
    sl = slice(v, v + 1) if v <= S else slice(1, S + 1)
    for m in out["interaction_masks"].values():
        m[:, 0, sl, :] = True
        m[:, 0, :, sl] = True
    return out


def as_dummy(batch, slots):
    """Slots made dataset dummies in every gene: features zeroed, pad mask set, frequency 0, interaction-mask row and column set."""
    out = _copy(batch)
    for s in slots:
        for b in out["pcre_feats"]:
            out["pcre_feats"][b][:, s] = 0.0
            out["pcre_pad_masks"][b][:, s] = True
            out["interaction_masks"][b][:, 0, s + 1, :] = True
            out["interaction_masks"][b][:, 0, :, s + 1] = True
        out["interaction_freq"][:, s + 1, :] = 0.0
        out["interaction_freq"][:, :, s + 1] = 0.0
    return out


def removed(batch, j, S):
    """pCRE j removed in every gene: slots j + 1.. shift left, a dummy is appended."""
    out = as_dummy(batch, [j])
    order = [s for s in range(S) if s != j] + [j]
    tok = torch.tensor([0] + [s + 1 for s in order])
    for b in out["pcre_feats"]:
        out["pcre_feats"][b] = out["pcre_feats"][b][:, order].contiguous()
        out["pcre_pad_masks"][b] = out["pcre_pad_masks"][b][:, order].contiguous()
        out["interaction_masks"][b] = out["interaction_masks"][b][:, :, tok][:, :, :, tok].contiguous()
    out["interaction_freq"] = out["interaction_freq"][:, tok][:, :, tok].contiguous()
    return out


def oracle_ablation(P, batch, cfg=None):
    """-> logits [B, i_max + 2, n_out]: orc.forward on the contract's edited masks, one pass per variant."""
    S = orc._cfg(cfg)["i_max"]
    with torch.no_grad():
        return torch.stack([orc.forward(P, variant_masks(batch, v, S), cfg) for v in range(S + 2)], 1)
