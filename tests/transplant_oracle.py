"""Oracle of the pCRE transplant screen (cf_pcre_transplant, chromoformer_amd.transplant), on the CPU with plain torch on batch dicts
in the reference's layout ([B, 1, 1, L, L] / [B, S, 1, L, L] pad masks, [B, 1, T, T] interaction masks, [B, T, T] frequencies; compact
[B, S, L] pCRE mask rows are understood too).  Independent of the product code: nothing of chromoformer_amd is imported.

The rule, candidate (feats {binsize: [L, F]}, cols {binsize: [L] bool, True = masked}) in slot j of gene g at frequency f:
  * pcre_feats[b][g, j] = feats[b];  pcre_pad_masks[b][g, j, 0] = rows_promoter[:, None] | cols[None, :], rows_promoter the diagonal of
    the gene's promoter pad mask (a compact mask: the row itself becomes cols);
  * interaction_masks[b][g, 0]: with dead(t) its diagonal, row and column j + 1 become dead, entry (j + 1, j + 1) becomes False;
  * interaction_freq[g]: row and column j + 1 become 0, entry (0, j + 1) becomes f.
slot = -1: nothing is edited."""
import torch

from oracle import chromoformer_oracle as orc

KEYS = ("promoter_feats", "promoter_pad_masks", "pcre_feats", "pcre_pad_masks", "interaction_masks", "interaction_freq")


def clone(batch):
    return {k: ({b: t.clone() for b, t in batch[k].items()} if isinstance(batch[k], dict) else batch[k].clone()) for k in KEYS}


def take(batch, genes):
    """The genes `genes` (indices) of a batch dict -> batch dict (copies)."""
    idx = torch.as_tensor(list(genes), dtype=torch.long)
    return {k: ({b: t[idx].clone() for b, t in batch[k].items()} if isinstance(batch[k], dict) else batch[k][idx].clone()) for k in KEYS}


def append_slot(batch, g):
    """The slot "append" takes for gene g: its first dead token t >= 1 at the coarsest resolution (fewest bins), as slot t - 1; -1: none."""
    bc = min(batch["promoter_feats"], key=lambda b: batch["promoter_feats"][b].shape[-2])
    im = batch["interaction_masks"][bc][g]
    T = im.shape[-1]
    dead = im.reshape(T, T).bool().diagonal()
    for t in range(1, T):
        if bool(dead[t]):
            return t - 1
    return -1


def transplant(batch, g, feats, cols, f, slot):
    """-> the batch dict with the candidate in slot `slot` of gene g at frequency f (a copy; slot = -1: the batch's own values)."""
    out = clone(batch)
    if slot < 0:
        return out
    J = slot + 1
    for b in out["pcre_feats"]:
        L = out["pcre_feats"][b].shape[-2]
        out["pcre_feats"][b][g, slot] = torch.as_tensor(feats[b], dtype=out["pcre_feats"][b].dtype)
        c = torch.as_tensor(cols[b]).bool().reshape(L)
        m = out["pcre_pad_masks"][b]
        if m[g, slot].numel() == L * L:
            rows = batch["promoter_pad_masks"][b][g].reshape(L, L).bool().diagonal()
            m[g, slot] = (rows[:, None] | c[None, :]).reshape(m[g, slot].shape).to(m.dtype)
        else:
            m[g, slot] = c.reshape(m[g, slot].shape).to(m.dtype)
        im = out["interaction_masks"][b][g]
        T = im.shape[-1]
        v = im.reshape(T, T)      # (a view of the copy)
        dead = v.bool().diagonal().clone()
        v[J, :] = dead.to(v.dtype)
        v[:, J] = dead.to(v.dtype)
        v[J, J] = 0
    fr = out["interaction_freq"][g]
    fr[J, :] = 0
    fr[:, J] = 0
    fr[0, J] = f
    return out


def candidate(lib_feats, lib_cols, c):
    """Candidate c of a library given as {binsize: [C, L, F]} and {binsize: [C, L]} -> (feats, cols) of transplant()."""
    return {b: t[c] for b, t in lib_feats.items()}, {b: t[c] for b, t in lib_cols.items()}


def edited_batch(batch, lib_feats, lib_cols, c, freq, q, slots):
    """The whole batch with candidate c at freq[g, c, q] in slot slots[g] of every gene g -> batch dict of the same B genes."""
    out = batch
    feats, cols = candidate(lib_feats, lib_cols, c)
    for g in range(batch["interaction_freq"].shape[0]):
        out = transplant(out, g, feats, cols, float(freq[g, c, q]), int(slots[g]))
    return out


def oracle_logits(P, batch, lib_feats, lib_cols, freq, slots, cfg=None, variants=None):
    """orc.forward on the edited batches -> logits [B, nv, n_out] for the (c, q) pairs `variants` (default: all, c-major)."""
    C, Q = freq.shape[1], freq.shape[2]
    variants = [(c, q) for c in range(C) for q in range(Q)] if variants is None else list(variants)
    out = []
    with torch.no_grad():
        for c, q in variants:
            out.append(orc.forward(P, edited_batch(batch, lib_feats, lib_cols, c, freq, q, slots), cfg))
    return torch.stack(out, 1)
