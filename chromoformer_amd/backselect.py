"""Greedy player selection of the mark games and of kept coalition tables: which few players are enough on their own to make a call, and
in what order does the prediction fall apart when players are taken away?  (cf_mark_backselect, cf_mark_window_backselect,
cf_mark_fine_backselect, cf_backselect_from_rows; csrc/cf_backselect.h.)

Functions on a model (a chromoformer_amd.net class on a GPU), not methods of it: the public names of the model classes are a kept
surface (tests/golden/model_api.json).  Each is the kind "backselect" of the one game runner (net_attrib.AttributionMixin._game): the
six arguments of forward() or a packed batch, the players of the sibling *_coalitions method, and the selection's own options.  There
is no PyTorch fallback and no torch arithmetic here: the order, the curve, the threshold, the size and the subset come from the
library's kernels."""
from __future__ import annotations

import torch

from . import attribution as A


@torch.no_grad()
def mark_backselect(model, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                    interaction_freq=None, players="cells", mode="backward", frac=0.9, threshold=None, target=None, direction="auto",
                    scale=0.0, donor=None, return_rows=False):
    """Greedy selection among up to 128 histone-mark players (cf_mark_backselect) -> (order, info), tensors on the model's device, no
    autograd graph: which few (mark, region) cells are enough on their own to make this call, and in what order does the prediction
    fall apart when cells are taken away?  Deterministic -- no sampling error -- at P (P + 1) / 2 + 1 forwards per gene.

      order               int32 [B, P]: the player of each move.  mode "backward": from everybody, each round removes the player
                          whose removal leaves the LARGEST direction * logit[target] (the least needed first); "forward": from
                          nobody, each round adds the player that raises it most.  Ties go to the lowest player index
      info["values"]      [B, P + 1, n_out]: the logits after t moves -- the deletion (insertion) curve; values[:, 0] is
                          info["logits"] (backward) or info["absent"] (forward), values[:, P] the other one, bit for bit
      info["size"]        int32 [B]: the players of the smallest set on the path with direction * (value - threshold) >= 0
                          (everybody counts as sufficient); info["subset"] bool [B, P]: that set -- in backward mode the
                          sufficient input subset, the last `size` players of order
      info["threshold"]   [B]: absent + frac * (logits - absent) on column target, rounded per operation, or `threshold`
      info["direction"]   int32 [B]: +1 where logits[target] >= absent[target], else -1; or `direction` (1 / -1) for every gene
      info["logits"], info["absent"]   [B, n_out]: everybody present (the prediction), nobody present
      info["names"], info["mode"], info["target"]   the players' names, the mode, the logit column
      info["rows"]        with return_rows: every evaluated row, a list of views: [B, 2, n_out] (nobody, everybody), then per
                          round t = 0 .. P - 2 [B, P - t, n_out], the candidates in ascending player order

    target: default 1 for the classifier, 0 for the regressor; threshold: [B] floats in place of frac.  players, scale and donor
    as in mark_coalitions_wide (with at most 16 players the game is mark_coalitions').  The subset, the size and the threshold
    come from the library's kernels; the host sees no logit during the call.  The packed forms of the first argument and the
    effect on a pending backward() are those of mark_coalitions."""
    batch = (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq)
    return model._game("mark_backselect", "mark_wide", "backselect", batch, players=players, scale=scale, donor=donor, table=return_rows,
                      select=(mode, frac, threshold, target, direction))

@torch.no_grad()
def mark_window_backselect(model, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                           interaction_freq=None, players="promoter", width=1, mode="backward", frac=0.9, threshold=None, target=None,
                           direction="auto", scale=0.0, donor=None, flip=None, return_rows=False):
    """Greedy selection among up to 128 window players (cf_mark_window_backselect) -> (order, info) with the keys of
    mark_backselect: which stretches are enough on their own?  players, width, scale, donor and flip as in mark_window_coalitions;
    mode, frac, threshold, target and direction as in mark_backselect.  A null player (a window past the region's real bins, a
    dummy slot) ties with the current set: it goes first wherever nothing scores higher."""
    batch = (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq)
    return model._game("mark_window_backselect", "mark_window", "backselect", batch, players=players, width=width, scale=scale, donor=donor,
                      flip=flip, table=return_rows, select=(mode, frac, threshold, target, direction))

@torch.no_grad()
def mark_fine_window_backselect(model, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                                interaction_freq=None, region=0, players="windows", width=1, n_windows=None, start=0, lengths=None,
                                mode="backward", frac=0.9, threshold=None, target=None, direction="auto", scale=0.0, donor=None, flip=None,
                                return_rows=False):
    """Greedy selection among up to 128 fine window players (cf_mark_fine_backselect) -> (order, info) with the keys of
    mark_backselect: which 200 bp stretches of the peak are enough on their own?  region, players, width, n_windows, start, lengths,
    scale, donor and flip as in mark_fine_window_coalitions (there is no return_feats: the rounds have different row counts); mode,
    frac, threshold, target and direction as in mark_backselect."""
    batch = (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq)
    return model._game("mark_fine_window_backselect", "mark_fine_window", "backselect", batch, players=players, width=width, scale=scale,
                      donor=donor, flip=flip, fine=(region, n_windows, start, lengths), table=return_rows,
                      select=(mode, frac, threshold, target, direction))


@torch.no_grad()
def backselect(model, coalitions, mode="backward", frac=0.9, threshold=None, target=None, direction="auto", names=None):
    """Greedy player selection on a kept coalition table (cf_backselect_from_rows) -> (order, info) with the keys of mark_backselect
    (no "rows").  `coalitions` is info["coalitions"] of any exact *_shapley call (the pCRE game, the mark games, the window games),
    [B, 2^P, n_out] with word m at column m, 1 <= P <= 16.  On the table of a mark game the result is that of mark_backselect on
    the same players: equal orders, bit-equal values.  names: the players' names for info["names"].  No forward runs and a
    pending backward() is left alone."""
    return model._backselect_table(coalitions, mode, frac, threshold, target, direction, names)


def mark_backselect_dataset(model, dataset, donor_dataset=None, genes=None, players="cells", mode="backward", frac=0.9, target=None, scale=0.0, bsz=None,
                            store=None, donor_store=None):
    """Greedy player selection of up to 128 histone-mark players for the genes of a ChromoformerDataset (one mark_backselect per
    batch): which few (mark, region) cells are enough on their own to make the call, and in what order does the prediction fall apart?
    Without `donor_dataset` an absent player's raw signal is scaled by `scale` (0 erases it); with one -- the same genes over the same
    regions in another cell type (same_regions runs first) -- it takes the donor's signal.  A generator over `genes` (ids; default:
    the dataset's) in chunks of at most min(bsz, model.max_batch) genes; per gene it yields a dict of host arrays:

        gene_id        the id
        order          int32 [P]: the player of each move (backward: removed; forward: added)
        ordered        the players' names in that order
        curve          float32 [P + 1, n_out]: the logits after t moves (the deletion curve; the insertion curve in forward mode)
        size           the number of players of the smallest sufficient set on the path
        subset         bool [P]: that set;  subset_names  its players' names
        threshold      the value logit `target` of a sufficient set reaches;  direction  +1 / -1, the sign of logits - absent
        logits, absent float32 [n_out]: every player present (the prediction), every player absent
        players        the players' names (attribution.mark_players_wide)

    The binned features come from `store` / `donor_store` as in mark_donor_shapley.  Parameters, gradients and optimiser state are left
    as they are; the pass overwrites the activations a grad-enabled model(...) keeps for its backward."""
    ds, dn = dataset, donor_dataset
    who = "mark_backselect"
    binsizes, _, genes, chunk = A._open(who, model, ds, genes, bsz, dn)
    spec = players if isinstance(players, str) else list(players)
    names = A.mark_players_wide(spec, ds.n_feats, ds.i_max)[2]      # (refusals before anything is loaded)
    for ids, _, _, args, donor, _ in A._batches(who, model, ds, genes, chunk, binsizes, store, dn, donor_store):
        order, info = mark_backselect(model, *args, players=spec, mode=mode, frac=frac, target=target, scale=scale, donor=donor)
        order = order.cpu().numpy()
        host = {k: info[k].cpu().numpy() for k in ("values", "size", "subset", "threshold", "direction", "logits", "absent")}
        for i, g in enumerate(ids):
            yield dict(gene_id=g, order=order[i].copy(), ordered=[names[p] for p in order[i]], curve=host["values"][i].copy(),
                       size=int(host["size"][i]), subset=host["subset"][i].copy(), subset_names=A.subset_names(host["subset"][i], names),
                       threshold=float(host["threshold"][i]), direction=int(host["direction"][i]), logits=host["logits"][i].copy(),
                       absent=host["absent"][i].copy(), players=list(names))
