"""Contact games: does an enhancer matter through its chromatin state or through its contact with the promoter?  Coalition forwards,
exact Shapley values, pair epistasis, interaction indices and dividends of players that delete pCRE slots and / or edit the
promoter-pCRE contact frequencies (interaction_freq), which enter every Regulation layer as a bias on the attention scores.
(cf_contact_coalitions, cf_contact_shapley, cf_contact_epistasis, cf_contact_shapley_interactions; csrc/cf_contact.h.)

Functions on a model (a chromoformer_amd.net class on a GPU), not methods of it: the public names of the model classes are a kept
surface (tests/golden/model_api.json), as for chromoformer_amd.backselect.  Each is a kind of the one game runner
(net_attrib.AttributionMixin._game) on the family "contact": the six arguments of forward() or a packed batch, then the players and the
rule.  There is no PyTorch fallback: the rows, the values and the indices come from the library's kernels.

The rule.  A player has two sets of pCRE slots (attribution.contact_players): the slots it DROPS and the slots whose CONTACT it holds.
In a coalition's row, for the absent players: interaction_masks row and column j + 1 are set at every resolution for every dropped slot
j (the rule of pcre_coalitions), and every entry of interaction_freq in row or column j + 1 is edited, once, for every slot j whose
contact is held -- scaled by `scale` (0 erases, the default; 2 doubles; 1 changes nothing; any finite value: the bias is signed) or,
with `donor_freq`, replaced by the donor's entry.  Three facts hold bit for bit: players that only drop play the pCRE game; a masked
score is replaced, not biased, so next to a deleted slot its contact is a null player; a dummy slot, scale = 1 and a donor_freq equal
to the gene's own are null players."""
from __future__ import annotations

from types import SimpleNamespace

import torch

from . import attribution as A
from .net_attrib import _INTER_DOC


@torch.no_grad()
def contact_coalitions(model, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                       interaction_freq=None, keep=None, players="contacts", scale=0.0, donor_freq=None):
    """The prediction under coalitions of contact players (cf_contact_coalitions) -> logits [B, n_coal, n_out] on the model's device,
    no autograd graph.  players: attribution.contact_players ("contacts", "pcres", "pcres_and_contacts", "all" or a list of
    (drop_slots, contact_slots) pairs).  `keep`: a sequence / array of ints, bit p set = player p present, or a bool array
    [n_coal, P].  Column c is the inference forward on the tensors the module's rule gives for the absent players of keep[c]
    (model(...) under no_grad on those tensors, bit-equal); the full word 2^P - 1 is the prediction.  donor_freq: a contiguous float32
    tensor [B, T, T] on the model's device, T = i_max + 1 -- the same genes' frequencies in another cell type, or a hypothetical
    contact map.  The Embedding + Pairwise stage runs once, the Regulation stack and the head on the B * n_coal rows.  The first
    argument after the model may also be a packed batch (an engine.Slot or a pack_batch result), with nothing after it.  The pass
    overwrites the activations a grad-enabled model(...) keeps for its backward: such a pending backward() raises."""
    batch = (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq)
    return model._game("contact_coalitions", "contact", "coalitions", batch, keep=keep, players=players, scale=scale, donor=donor_freq)


@torch.no_grad()
def contact_shapley(model, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                    interaction_freq=None, players="contacts", scale=0.0, donor_freq=None, return_coalitions=False):
    """Exact Shapley values of contact players (cf_contact_shapley) -> (phi, info), tensors on the model's device, no autograd graph:

      phi                 [B, P, n_out]: player p's average marginal contribution to each logit over all orders of adding the
                          players to the gene with every player absent; exactly 0 for a null player (a dummy slot, scale = 1, a
                          donor_freq equal to the gene's own)
      info["logits"]      [B, n_out]: the prediction (every player present; model(...) under no_grad, bit-equal)
      info["erased"]      [B, n_out]: every player absent (info["donor"] with donor_freq)
      info["delta"]       [B, n_out]: phi.sum(1) - (logits - erased), the efficiency gap (rounding only)
      info["players"]     the players' names
      info["coalitions"]  [B, 2^P, n_out], with return_coalitions: the logits of every coalition, word m at column m

    players, scale and donor_freq as in contact_coalitions; all 2^P coalitions (256 for the eight contacts) run from one trunk pass,
    in logit space, where efficiency holds.  With players="pcres" phi carries the bits of model.pcre_shapley.  The kept table feeds
    model.shapley_dividends, model.shapley_interactions and backselect.backselect as any other.  The packed forms of the first
    argument and the effect on a pending backward() are those of contact_coalitions."""
    batch = (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq)
    return model._game("contact_shapley", "contact", "shapley", batch, players=players, scale=scale, donor=donor_freq, table=return_coalitions)


@torch.no_grad()
def contact_epistasis(model, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                      interaction_freq=None, players="contacts", scale=0.0, donor_freq=None):
    """Pair epistasis of contact players (cf_contact_epistasis) -> (eps, info), tensors on the model's device, no autograd graph.
    With v(...) the logits with the named players absent:

      eps[:, i, j]    [B, P, P, n_out]: ((v() - v(i)) - v(j)) + v(i, j) for i != j, exactly symmetric: 0 when the two players add
                      up, non-zero when they are redundant or cooperate; eps[:, i, i] = v() - v(i), the leave-one-out effect
      info["logits"]  [B, n_out]: v(), the prediction;  info["single"]  [B, P, n_out]: v(i);  info["players"]  the names

    The 1 + P + P (P - 1) / 2 rows (attribution.coalition_table("pairs", P)) run from one trunk pass; at least 2 players.  players,
    scale, donor_freq, the packed forms of the first argument and the effect on a pending backward() are those of
    contact_coalitions."""
    batch = (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq)
    return model._game("contact_epistasis", "contact", "epistasis", batch, players=players, scale=scale, donor=donor_freq)


@torch.no_grad()
def contact_shapley_interactions(model, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                                 interaction_freq=None, players="contacts", scale=0.0, donor_freq=None, index="sii", return_coalitions=False):
    """Pairwise Shapley interaction indices of contact players (cf_contact_shapley_interactions) -> (inter, info), tensors on the
    model's device, no autograd graph.  At least 2 players; the 2^P coalitions run once, as in contact_shapley:

      %(inter)s
    players, scale and donor_freq as in contact_coalitions (the absent key is "donor" with donor_freq).  The packed forms of the first
    argument and the effect on a pending backward() are those of contact_coalitions."""
    batch = (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq)
    return model._game("contact_shapley_interactions", "contact", "shapley_interactions", batch, players=players, scale=scale, donor=donor_freq,
                       index=index, table=return_coalitions)


contact_shapley_interactions.__doc__ %= {"inter": _INTER_DOC.replace("\n    ", "\n") % {
    "absent": "erased", "sibling": "contact_shapley", "players": "\n      info[\"players\"]     the players' names"}}


@torch.no_grad()
def contact_dividends(model, *args, **kwargs):
    """contact_shapley(model, ..., return_coalitions=True) with the same arguments, then model.shapley_dividends on its table ->
    (div, info) as model.mark_dividends: div [B, 2^P, n_out], word m at column m; info is contact_shapley's plus phi, mass, names and
    sets.  In the joint game ("pcres_and_contacts") every set that holds `contact j` without `pcre j` has dividend exactly 0."""
    phi, info = contact_shapley(model, *args, **dict(kwargs, return_coalitions=True))
    return model._dividends_info(phi, info, info["players"])


def bound(model):
    """The two exact-game functions with `model` bound, under the names attribution._exact_game asks a model for."""
    return SimpleNamespace(contact_shapley=lambda *a, **k: contact_shapley(model, *a, **k),
                           contact_shapley_interactions=lambda *a, **k: contact_shapley_interactions(model, *a, **k))


def contact_shapley_dataset(model, dataset, donor_dataset=None, genes=None, players="contacts", scale=0.0, marks="own", epistasis=False,
                            interactions=None, dividends=False, bsz=None, store=None, donor_store=None):
    """contact_shapley (and optionally contact_epistasis, contact_shapley_interactions in its place, the dividends) over the genes of
    a ChromoformerDataset, against a donor cell type's contact frequencies if a donor dataset is given
    (chromoformer_amd.attribution.contact_shapley, a generator of per-gene dicts)."""
    return A.contact_shapley(model, dataset, donor_dataset, genes=genes, players=players, scale=scale, marks=marks, epistasis=epistasis,
                             interactions=interactions, dividends=dividends, bsz=bsz, store=store, donor_store=donor_store)
