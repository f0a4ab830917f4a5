"""`python -m chromoformer_amd.predict` -- the inference entrypoint (reference: demo/run_demo.py and
demo/run_demo_regression.py, same -m / -d / -o / -w options plus --regression instead of a second script).

    prediction column = sigmoid(logits)[:, 1]   (classifier, demo/run_demo.py:116)
                      = logits[:, 0]            (regressor,  demo/run_demo_regression.py:117)

Forward only (`cf_forward(..., save_for_backward=0)`) on batches staged from a GeneStore.  Checkpoints in the
reference's `.pt` layout load directly; checkpoints written before the reference renamed its modules
(`embed2000_a`, `transformer500`, `lin_proj_c`, ... -- the mapping of misc/convert_weight.py:19-88) are renamed
on the fly."""
from __future__ import annotations

import argparse
import re

import numpy as np
import pandas as pd
import torch

from .data import ChromoformerDataset, GeneStore
from .engine import Slot, Trainer
from .net import ChromoformerClassifier, ChromoformerRegressor
from .util import seed_everything

_LEGACY = [  # (pattern, replacement), applied in order; first match of the second group wins (convert_weight.py)
    (r"transformer(2000|500|100)", r"regulation.\1.transformer"),
    (r"embed(2000|500|100)_a", r"embed.\1"),
    (r"embed(2000|500|100)_b", r"pairwise_interaction.\1"),
    (r"^embed(?=\d)", "embed."),
    (r"^pw_int", "pairwise_interaction."),
    (r"^reg(?=\d)", "regulation."),
]


def modernise_keys(state):
    """Legacy checkpoint keys -> current `state_dict` keys (no-op for current checkpoints)."""
    out = {}
    for k, v in state.items():
        k = k.replace("lin_proj_c.", "lin_proj_pcre.") if "lin_proj_c." in k else k
        for pat, rep in _LEGACY:
            k2 = re.sub(pat, rep, k, count=1)
            if k2 != k:
                k = k2
                break
        out[k] = v
    return out


def _savez(path, **arrays):
    """np.savez to exactly `path` (through a file object: given a name without .npz, np.savez would append it)."""
    with open(path, "wb") as f:
        np.savez(f, **arrays)


def _slot_batches(who, model, store, bsz):
    """The genes of a device-resident store, in store order, in batches of at most bsz -> (lo, B, slot) per batch: genes lo .. lo + B - 1
    gathered on the device (cf_gather_batch) into a Slot of B genes, one Slot per size.  The gather's error word is read when the
    caller comes back for the next batch, after its own work on this one: an error raises RuntimeError naming `who`, the writer."""
    import ctypes as C

    from . import _lib
    n, dev, L = len(store), model._device, _lib.lib()
    struct = store.struct()
    order = torch.arange(n, dtype=torch.int32, device=dev)
    slots = {}
    st = torch.cuda.current_stream(dev).cuda_stream
    for lo in range(0, n, bsz):
        B = min(bsz, n - lo)
        slot = slots.get(B) or slots.setdefault(B, Slot(model, B))
        cursor = torch.tensor([0, 1, 0, 0], dtype=torch.int32).to(dev)
        _lib.check(L.cf_gather_batch(model._handle, C.byref(struct), order[lo:].data_ptr(), cursor.data_ptr(), C.byref(slot.struct), None, st),
                   "cf_gather_batch")
        yield lo, B, slot
        if int(cursor[2].item()):
            raise RuntimeError("%s: the device-side gather reported errors at gene %d (store / order mismatch)" % (who, lo))


def _dict_batches(store, donor_store, bsz):
    """The genes of a device-resident store, in store order, in batches of at most bsz -> (lo, B, forward()'s six arguments from
    store.batch, the donor pair from donor_store.batch or None without a donor store, the donor's batch dict or None) per batch."""
    from .attribution import _BATCH_KEYS, _donor_pair
    for lo in range(0, len(store), bsz):
        idx = list(range(lo, min(lo + bsz, len(store))))
        d = store.batch(idx)
        dd = donor_store.batch(idx) if donor_store is not None else None
        yield lo, len(idx), tuple(d[k] for k in _BATCH_KEYS), None if dd is None else _donor_pair(dd), dd


def write_attention_maps(model, store, bsz, attention_dir=None, embeddings_out=None):
    """Attention maps (`attention_dir`/{embed,pairwise_interaction,regulation}_{binsize}.npy) and / or the regulatory embedding
    (`embeddings_out`, [n_genes, 3 * d_emb]) of every gene of a device-resident store, in store order.  Per batch: one device gather
    into a Slot and one model.attention_maps; the rows go straight into .npy memory maps (nothing is gathered in host memory)."""
    import os
    which = (("embed", "pairwise_interaction", "regulation") if attention_dir else ()) + (("regulatory_embedding",) if embeddings_out else ())
    if not which:
        return
    n = len(store)
    embed, pair, reg = model._kws
    S, T = model.i_max, model.i_max + 1
    outs = {}
    if attention_dir:
        os.makedirs(attention_dir, exist_ok=True)
        for b, nb in zip(model.binsizes, model.n_bins):
            for key, shape in (("embed", (embed["n_heads"], nb)), ("pairwise_interaction", (pair["n_layers"], S, pair["n_heads"], nb)),
                               ("regulation", (reg["n_layers"], reg["n_heads"], T))):
                outs[key, b] = np.lib.format.open_memmap(os.path.join(attention_dir, "%s_%d.npy" % (key, b)), mode="w+", dtype=np.float32,
                                                         shape=(n,) + shape)
    if embeddings_out:
        outs["regulatory_embedding", None] = np.lib.format.open_memmap(embeddings_out, mode="w+", dtype=np.float32,
                                                                       shape=(n, len(model.binsizes) * model.d_emb))
    for lo, B, slot in _slot_batches("write_attention_maps", model, store, bsz):
        _, maps = model.attention_maps(slot, which=which)
        for (key, b), mm in outs.items():
            mm[lo:lo + B] = (maps[key] if b is None else maps[key][b]).cpu().numpy()
    for mm in outs.values():
        mm.flush()


def write_pcre_ablation(model, store, bsz, path, regression=False):
    """In-silico pCRE deletion of every gene of a device-resident store, in store order: `path`, a float32 .npy [n_genes, i_max + 2]
    holding the prediction column's quantity (sigmoid(logits)[:, 1], or logits[:, 0] for the regressor) with nothing deleted
    (column 0), pCRE slot j deleted (column 1 + j) and the promoter alone (last column).  Per batch: one device gather into a Slot
    and one model.pcre_ablation.  The logits (8 bytes per gene and column) are kept on the host; each column goes through the
    very sigmoid call predict() makes on the [n_genes, 2] logits, so column 0 is the prediction bit for bit."""
    n, V = len(store), model.i_max + 2
    logits = torch.empty(n, V, model.n_out)
    for lo, B, slot in _slot_batches("write_pcre_ablation", model, store, bsz):
        logits[lo:lo + B] = model.pcre_ablation(slot).cpu()
    mm = np.lib.format.open_memmap(path, mode="w+", dtype=np.float32, shape=(n, V))
    for v in range(V):
        col = logits[:, v].contiguous()          # [n_genes, n_out], laid out as the logits predict() turns into its column
        mm[:, v] = col.numpy().reshape(-1) if regression else torch.sigmoid(col).numpy()[:, 1]
    mm.flush()


_EXACT_GAMES = {      # the exact games of the writers, by the prefix of their model methods (<game>_shapley, _epistasis, _dividends, ...):
    # kw: the keyword arguments those methods take; absent: info's key (and the .npz column) of the prediction with every player absent;
    # extra: the game's own column of the Shapley .npz
    "pcre": dict(kw=(), absent="promoter_only", extra="n_pcres"),
    "mark": dict(kw=("players", "scale"), absent="erased", extra=None),
    "mark_donor": dict(kw=("donor", "players"), absent="donor", extra="donor_prediction"),
}


def _game_kw(game, players, scale, donor):
    """The keyword arguments of an exact game's model methods."""
    given = dict(players=players, scale=scale, donor=donor)
    return {k: given[k] for k in _EXACT_GAMES[game]["kw"]}


def write_exact_values(model, game, store, donor_store, bsz, gene_ids, shapley_out=None, epistasis_out=None, interactions_out=None,
                       regression=False, players="marks", scale=0.0, index="sii"):
    """Exact Shapley values, pair epistasis and / or pairwise Shapley interaction indices of one game of every gene of a device-resident
    store, in store order, in LOGIT space of the prediction's column (1 for the classifier, 0 for the regressor: the efficiency identity
    phi.sum(1) = logits - absent holds there, not after the sigmoid).  game (_EXACT_GAMES):

        "pcre"         the pCREs (P = i_max).  shapley_out: an .npz with phi [n, P], logits [n], promoter_only [n] and n_pcres [n] (the
                       slots that are no dummies)
        "mark"         the histone marks; players (attribution.mark_players) and scale apply.  shapley_out: an .npz with gene_ids [n],
                       players [P] (names), phi [n, P], logits [n] and erased [n]
        "mark_donor"   the marks against donor_store, the same genes in the same order in a donor cell type; players applies.
                       shapley_out: gene_ids, players, phi, logits, donor [n] (every player's marks from the donor, under the gene's
                       masks and frequencies) and donor_prediction [n] (the plain forward of the donor's own batch)

    epistasis_out: a float32 .npy [n, P, P]; interactions_out: a float32 .npy [n, P, P], the index `index` ("sii" / "sti").  Per batch:
    one device gather into a Slot (the donor game: one store.batch per store), one model.<game>_shapley and / or one
    model.<game>_epistasis; with interactions_out one model.<game>_shapley_interactions, which serves shapley_out too (the 2^P forwards
    run once); the donor game's shapley_out adds one plain forward of the donor's batch."""
    from .attribution import _BATCH_KEYS, mark_players
    who, desc = "write_exact_values", _EXACT_GAMES[game]
    n, t, with_donor = len(store), 0 if regression else 1, "donor" in desc["kw"]
    if with_donor and len(donor_store) != n:
        raise ValueError("%s: the donor store holds %d genes, the store %d" % (who, len(donor_store), n))
    names = mark_players(players, model.n_feats, model.i_max)[2] if "players" in desc["kw"] else None
    P = model.i_max if names is None else len(names)
    phi, logits, absent = torch.empty(n, P), torch.empty(n), torch.empty(n)
    extra = torch.empty(n, dtype=torch.int32 if game == "pcre" else torch.float32)
    eps = np.lib.format.open_memmap(epistasis_out, mode="w+", dtype=np.float32, shape=(n, P, P)) if epistasis_out else None
    inter = np.lib.format.open_memmap(interactions_out, mode="w+", dtype=np.float32, shape=(n, P, P)) if interactions_out else None
    if with_donor:
        batches = _dict_batches(store, donor_store, bsz)
    else:      # (the Slot alone: the packed form of the methods' first argument)
        batches = ((lo, B, (slot,), None, None) for lo, B, slot in _slot_batches(who, model, store, bsz))
    for lo, B, args, feats, dd in batches:
        kw = _game_kw(game, players, scale, feats)
        if inter is not None:
            x, info = getattr(model, game + "_shapley_interactions")(*args, index=index, **kw)
            inter[lo:lo + B] = x[..., t].cpu().numpy()
            p = info["phi"]
        elif shapley_out:
            p, info = getattr(model, game + "_shapley")(*args, **kw)
        if shapley_out:
            phi[lo:lo + B] = p[..., t].cpu()
            logits[lo:lo + B] = info["logits"][:, t].cpu()
            absent[lo:lo + B] = info[desc["absent"]][:, t].cpu()
            if game == "pcre":
                dummy = torch.stack([m[:, 0, 1:] != 0 for m in args[0].im]).all(0)      # a dummy slot: its key masked for the promoter row, every resolution
                extra[lo:lo + B] = (~dummy).sum(1).to(torch.int32).cpu()
            elif with_donor:
                with torch.no_grad():
                    extra[lo:lo + B] = model(*(dd[k] for k in _BATCH_KEYS))[:, t].cpu()
        if eps is not None:
            eps[lo:lo + B] = getattr(model, game + "_epistasis")(*args, **kw)[0][..., t].cpu().numpy()
    if shapley_out:
        cols = {"phi": phi.numpy(), "logits": logits.numpy(), desc["absent"]: absent.numpy()}
        if desc["extra"]:
            cols[desc["extra"]] = extra.numpy()
        if names is not None:
            cols = dict(gene_ids=np.array(list(gene_ids)), players=np.array(names), **cols)
        _savez(shapley_out, **cols)
    for mm in (eps, inter):
        if mm is not None:
            mm.flush()


def write_dividends(model, store, donor_store, bsz, gene_ids, path, game="mark", regression=False, players="marks", scale=0.0):
    """Harsanyi dividends of an exact game of every gene of a device-resident store, in store order, in LOGIT space of the
    prediction's column, into `path`, an .npz with gene_ids [n], players [P] (names), sets [2^P] (the set names by word, "" for the empty
    set), dividends [n, 2^P] float32 (word m at column m; they add up to the logit of every coalition) and mass [n, 2^P] (the scale of
    a dividend's rounding error, attribution.dividend_bound).  game: "pcre" (model.pcre_dividends), "mark" (model.mark_dividends; players
    and scale apply) or "mark_donor" (model.mark_donor_dividends against donor_store, the same genes in the same order; players
    applies).  Per batch: one gather per store and one such call (its own 2^P forwards)."""
    n = len(store)
    if game not in _EXACT_GAMES:
        raise ValueError("write_dividends: unknown game %r; choose from %s" % (game, list(_EXACT_GAMES)))
    with_donor = "donor" in _EXACT_GAMES[game]["kw"]
    if with_donor and (donor_store is None or len(donor_store) != n):
        raise ValueError("write_dividends: the donor store must hold the store's %d genes" % n)
    t = 0 if regression else 1
    div, mass, names, sets = None, None, None, None
    for lo, B, args, feats, _ in _dict_batches(store, donor_store if with_donor else None, bsz):
        x, info = getattr(model, game + "_dividends")(*args, **_game_kw(game, players, scale, feats))
        if div is None:
            div, mass = np.empty((n, x.shape[1]), np.float32), np.empty((n, x.shape[1]), np.float32)
            names, sets = info["names"], info["sets"]
        div[lo:lo + B] = x[..., t].cpu().numpy()
        mass[lo:lo + B] = info["mass"][..., t].cpu().numpy()
    _savez(path, gene_ids=np.array(list(gene_ids)), players=np.array(names), sets=np.array(sets), dividends=div, mass=mass)


def write_mark_sampled_values(model, store, donor_store, bsz, gene_ids, path, regression=False, players="cells", n_perm=64, seed=0, scale=0.0):
    """Permutation-sampled Shapley values of up to 128 histone-mark players (model.mark_shapley_sampled) of every gene of a
    device-resident store, in store order, in LOGIT space of the prediction's column, into `path`, an .npz with gene_ids [n], players
    [P] (names), permutations uint8 [n_perm, P] (the orders, the same for every gene), phi [n, P], stderr [n, P] (the standard error of
    phi over the orders: the sampling error is reported, not bounded), logits [n] and absent [n] (every player absent; phi sums to
    their difference).  donor_store None: an absent player's raw signal is scaled by `scale`; else a store of the same genes in the
    same order in the donor cell type, whose signal it takes.  Per batch: one gather per store and one model.mark_shapley_sampled."""
    from .attribution import mark_players_wide, shapley_permutations
    n = len(store)
    if donor_store is not None and len(donor_store) != n:
        raise ValueError("write_mark_sampled_values: the donor store holds %d genes, the store %d" % (len(donor_store), n))
    names = mark_players_wide(players, model.n_feats, model.i_max)[2]
    P, t = len(names), 0 if regression else 1
    perms = shapley_permutations(P, n_perm, seed)
    phi, se, logits, absent = torch.empty(n, P), torch.empty(n, P), torch.empty(n), torch.empty(n)
    for lo, B, args, feats, _ in _dict_batches(store, donor_store, bsz):
        p, info = model.mark_shapley_sampled(*args, players=players, permutations=perms, scale=scale, donor=feats)
        phi[lo:lo + B] = p[..., t].cpu()
        se[lo:lo + B] = info["stderr"][..., t].cpu()
        logits[lo:lo + B] = info["logits"][:, t].cpu()
        absent[lo:lo + B] = info["absent"][:, t].cpu()
    _savez(path, gene_ids=np.array(list(gene_ids)), players=np.array(names), permutations=perms, phi=phi.numpy(), stderr=se.numpy(),
           logits=logits.numpy(), absent=absent.numpy())


def write_mark_backselect(model, store, donor_store, bsz, gene_ids, path, regression=False, players="cells", mode="backward", frac=0.9, scale=0.0):
    """Greedy player selection among up to 128 histone-mark players (backselect.mark_backselect) of every gene of a device-resident store,
    in store order, on the prediction's logit column, into `path`, an .npz with gene_ids [n], players [P] (names), mode, frac, order
    int32 [n, P] (the player of each move), curve [n, P + 1] (the logit after t moves), size [n] and subset bool [n, P] (the smallest
    sufficient set on the path), threshold [n], direction [n], logits [n] and absent [n].  donor_store None: an absent player's raw
    signal is scaled by `scale`; else a store of the same genes in the same order in the donor cell type, whose signal it takes.
    Per batch: one gather per store and one backselect.mark_backselect."""
    from .attribution import mark_players_wide
    from .backselect import mark_backselect
    n = len(store)
    if donor_store is not None and len(donor_store) != n:
        raise ValueError("write_mark_backselect: the donor store holds %d genes, the store %d" % (len(donor_store), n))
    names = mark_players_wide(players, model.n_feats, model.i_max)[2]
    P, t = len(names), 0 if regression else 1
    order, curve, size, subset = torch.empty(n, P, dtype=torch.int32), torch.empty(n, P + 1), torch.empty(n, dtype=torch.int32), torch.empty(n, P, dtype=torch.bool)
    thr, sign, logits, absent = torch.empty(n), torch.empty(n, dtype=torch.int32), torch.empty(n), torch.empty(n)
    for lo, B, args, feats, _ in _dict_batches(store, donor_store, bsz):
        o, info = mark_backselect(model, *args, players=players, mode=mode, frac=frac, target=t, scale=scale, donor=feats)
        order[lo:lo + B] = o.cpu()
        curve[lo:lo + B] = info["values"][..., t].cpu()
        size[lo:lo + B] = info["size"].cpu()
        subset[lo:lo + B] = info["subset"].cpu()
        thr[lo:lo + B] = info["threshold"].cpu()
        sign[lo:lo + B] = info["direction"].cpu()
        logits[lo:lo + B] = info["logits"][:, t].cpu()
        absent[lo:lo + B] = info["absent"][:, t].cpu()
    _savez(path, gene_ids=np.array(list(gene_ids)), players=np.array(names), mode=np.array(mode), frac=np.float32(frac), order=order.numpy(),
           curve=curve.numpy(), size=size.numpy(), subset=subset.numpy(), threshold=thr.numpy(), direction=sign.numpy(), logits=logits.numpy(),
           absent=absent.numpy())


def write_mark_sampled_interactions(model, ds, donor_ds, store, donor_store, bsz, gene_ids, path, regression=False, players="cells", top=4, focal=None,
                                    index="sii", n_perm=64, seed=0, scale=0.0):
    """Sampled pairwise Shapley interaction indices of each gene's focal mark players (attribution.mark_shapley_interactions_sampled:
    the gene's `top` players by |phi|, or `focal` for every gene) of every gene of a device-resident store, in store order, in LOGIT
    space of the prediction's column, into `path`, an .npz with gene_ids [n], players [P] (names), index, permutations uint8
    [n_perm, P], focal int32 [n, n_focal] (the focal players of each gene), interactions [n, n_focal, P] (row f: focal player f with
    every player; not symmetric between focal players), stderr [n, n_focal, P] (the standard error over the orders: the sampling error
    is reported, not bounded), phi and phi_stderr [n, P] (the sampled Shapley values from the same forwards), logits [n] and absent [n].
    ds / donor_ds: the datasets the stores were built from; donor_ds None: the scale rule."""
    from .attribution import mark_shapley_interactions_sampled
    t = 0 if regression else 1
    res = list(mark_shapley_interactions_sampled(model, ds, donor_ds, genes=list(gene_ids), players=players, top=top, focal=focal, index=index,
                                                 n_perm=n_perm, seed=seed, scale=scale, bsz=bsz, store=store, donor_store=donor_store))
    _savez(path, gene_ids=np.array(list(gene_ids)), players=np.array(res[0]["players"]), index=np.array(index), permutations=res[0]["permutations"],
           focal=np.stack([r["focal"] for r in res]), interactions=np.stack([r["interactions"][..., t] for r in res]),
           stderr=np.stack([r["stderr"][..., t] for r in res]), phi=np.stack([r["phi"][..., t] for r in res]),
           phi_stderr=np.stack([r["phi_stderr"][..., t] for r in res]), logits=np.array([r["logits"][t] for r in res], dtype=np.float32),
           absent=np.array([r["absent"][t] for r in res], dtype=np.float32))


def write_mark_window_values(model, ds, donor_ds, store, donor_store, bsz, gene_ids, path, regression=False, players="promoter", width=1, n_perm=64,
                             seed=0, scale=0.0):
    """Shapley values of window players (model.mark_window_shapley_dataset: exact with at most 16 players, else sampled) of every gene
    of a device-resident store, in store order, in LOGIT space of the prediction's column, into `path`, an .npz with gene_ids [n],
    players [P] (names), estimator ("exact" or "sampled": which one ran), phi [n, P], stderr [n, P] (zeros from the exact call), logits
    [n], absent [n] (every player absent; phi sums to their difference), null bool [n, P] (the player's window holds no real bin of
    the gene: phi = 0), chroms [n, P] and windows int64 [n, P, 2] (the genomic start and end of the player's window in its region; ""
    and -1 where null) and, sampled, permutations uint8 [n_perm, P].  ds / donor_ds: the datasets the stores were built from (strand
    and coordinates); donor_ds None: the scale rule."""
    n, t = len(gene_ids), 0 if regression else 1
    rows = list(model.mark_window_shapley_dataset(ds, donor_ds, genes=list(gene_ids), players=players, width=width, n_perm=n_perm, seed=seed,
                                                  scale=scale, bsz=bsz, store=store, donor_store=donor_store))
    P = len(rows[0]["players"])
    chroms, windows = np.full((n, P), "", dtype=object), np.full((n, P, 2), -1, dtype=np.int64)
    for i, r in enumerate(rows):
        for p, real in enumerate(r["windows"]):
            if real:      # (the named specs give every player one region)
                chroms[i, p], windows[i, p] = real[0][1], real[0][2:]
    out = dict(gene_ids=np.array(list(gene_ids)), players=np.array(rows[0]["players"]), estimator=np.array(rows[0]["estimator"]),
               phi=np.stack([r["phi"][:, t] for r in rows]), stderr=np.stack([r["stderr"][:, t] for r in rows]),
               logits=np.array([r["logits"][t] for r in rows], dtype=np.float32), absent=np.array([r["absent"][t] for r in rows], dtype=np.float32),
               null=np.stack([r["null"] for r in rows]), chroms=chroms.astype(str), windows=windows)
    if "permutations" in rows[0]:
        out["permutations"] = rows[0]["permutations"]
    _savez(path, **out)


def write_mark_fine_window_values(model, ds, donor_ds, store, donor_store, bsz, gene_ids, path, regression=False, region="promoter", width=2,
                                  players="windows", zoom=1, n_perm=64, seed=0, scale=0.0):
    """Shapley values of FINE window players (model.mark_fine_window_shapley_dataset: the coarse window game first, then the fine game
    inside each gene's `zoom` most important coarse windows) of every gene of a device-resident store, in store order, in LOGIT space
    of the prediction's column, into `path`, an .npz with gene_ids [n], players [P] (the fine game's names, windows relative to the
    zoomed coarse window), exact (whether the fine game was exact), zoom int64 [n, k] (the chosen coarse windows, most important first;
    -1 where the gene has fewer), coarse_phi [n, n_cwin] (the coarse game's values; NaN past the region's real coarse windows), phi and
    stderr [n, k, P] (stderr zeros when exact), logits [n], absent [n, k] (every fine player absent; phi[:, r] sums to logits - absent[:, r];
    NaN where zoom is -1), null bool [n, k, P] (the player has no real window in the gene: phi = 0), chroms [n] (the region's
    chromosome; "" without the region) and windows int64 [n, k, P, 2] (genomic start and end; -1 where null).  ds / donor_ds: the
    datasets the stores were built from (strand, coordinates, lengths); donor_ds None: the scale rule."""
    n, t = len(gene_ids), 0 if regression else 1
    rows = list(model.mark_fine_window_shapley_dataset(ds, donor_ds, genes=list(gene_ids), region=region, zoom=zoom, width=width, players=players,
                                                       n_perm=n_perm, seed=seed, scale=scale, bsz=bsz, store=store, donor_store=donor_store))
    from .attribution import fine_window_players
    rf, rc = int(np.argmin(model.binsizes)), int(np.argmin(model.n_bins))
    names = fine_window_players(players, model.n_feats, width, -(-(model.n_bins[rf] // model.n_bins[rc]) // width))[3]
    P, k, Pc = len(names), int(zoom), model.n_bins[rc]
    out = dict(gene_ids=np.array(list(gene_ids)), players=np.array(names), exact=np.array(bool(rows[0]["exact"])),
               zoom=np.full((n, k), -1, dtype=np.int64), coarse_phi=np.full((n, Pc), np.nan, dtype=np.float32),
               phi=np.zeros((n, k, P), dtype=np.float32), stderr=np.zeros((n, k, P), dtype=np.float32),
               logits=np.array([r["logits"][t] for r in rows], dtype=np.float32), absent=np.full((n, k), np.nan, dtype=np.float32),
               null=np.ones((n, k, P), dtype=bool), chroms=np.array([r["region"][0] if r["region"] else "" for r in rows]),
               windows=np.full((n, k, P, 2), -1, dtype=np.int64))
    for i, r in enumerate(rows):
        out["zoom"][i, :len(r["zoom"])] = r["zoom"]
        out["coarse_phi"][i, :len(r["coarse_phi"])] = r["coarse_phi"][:, t]
        out["absent"][i, :len(r["absent"])] = r["absent"][:, t]
        at = (i, r["rank"], r["index"])
        out["phi"][at], out["null"][at] = r["phi"][:, t], False
        if r["stderr"] is not None:
            out["stderr"][at] = r["stderr"][:, t]
        if len(r["windows"]):
            out["windows"][at] = np.array([w[1:] for w in r["windows"]], dtype=np.int64)
    _savez(path, **out)


def write_contact_values(model, ds, donor_ds, store, donor_store, bsz, gene_ids, shapley_out, interactions_out=None, dividends_out=None,
                         regression=False, players="contacts", scale=0.0, marks="own", index="sii"):
    """Exact Shapley values of contact players (contact.contact_shapley_dataset: an absent player deletes its pCRE slots and / or edits
    their promoter contact frequencies) of every gene of a device-resident store, in store order, in LOGIT space of the prediction's
    column, into `shapley_out`, an .npz with gene_ids [n], players [P] (names), phi [n, P], logits [n] (every player present), erased [n]
    (every player absent) or, with donor_ds, donor [n], freq [n, i_max] (the genes' contact frequencies) and n_pcres [n]; with donor_ds
    (the donor rule: an absent contact takes the donor cell type's frequency) also donor_freq [n, i_max] and marks ("own" / "donor":
    whose features the game was played on).  interactions_out: a float32 .npy [n, P, P], the pairwise index `index` (the batch's one
    call then serves phi too); dividends_out: an .npz with gene_ids, players, sets [2^P], dividends and mass [n, 2^P], from the table of
    the same call.  ds / donor_ds: the datasets the stores were built from; donor_ds None: the scale rule (`scale` applies)."""
    from .attribution import set_names
    from .contact import contact_shapley_dataset
    t = 0 if regression else 1
    rows = list(contact_shapley_dataset(model, ds, donor_ds, genes=list(gene_ids), players=players, scale=scale, marks=marks,
                                              interactions=index if interactions_out else None, dividends=bool(dividends_out), bsz=bsz, store=store,
                                              donor_store=donor_store))
    names, absent = rows[0]["players"], "erased" if donor_ds is None else "donor"
    ids = np.array(list(gene_ids))
    if shapley_out:
        out = dict(gene_ids=ids, players=np.array(names), phi=np.stack([r["phi"][:, t] for r in rows]),
                   logits=np.array([r["logits"][t] for r in rows], dtype=np.float32), freq=np.stack([r["freq"] for r in rows]),
                   n_pcres=np.array([len(r["pcres"]) for r in rows], dtype=np.int32))
        out[absent] = np.array([r[absent][t] for r in rows], dtype=np.float32)
        if donor_ds is not None:
            out["donor_freq"], out["marks"] = np.stack([r["donor_freq"] for r in rows]), np.array(marks)
        _savez(shapley_out, **out)
    if interactions_out:
        np.save(interactions_out, np.stack([r["interactions"][..., t] for r in rows]).astype(np.float32))
    if dividends_out:
        sets = set_names(np.arange(1 << len(names), dtype=np.uint32), names)
        _savez(dividends_out, gene_ids=ids, players=np.array(names), sets=np.array(sets), dividends=np.stack([r["dividends"][..., t] for r in rows]),
               mass=np.stack([r["mass"][..., t] for r in rows]))


def write_transplant(model, ds, store, bsz, gene_ids, bed, out, regression=False, freqs=(1.0, 5.0, 10.0), slot="append"):
    """pCRE transplant screen (transplant.pcre_transplant_dataset) of every gene of a device-resident store, in store order, into `out`,
    an .npz: gene_ids [n], prediction [n], transplant [n, C, Q] -- the prediction with candidate c of the BED file `bed`
    (`chrom start end [name]` lines; the raw chrom:start-end.npy files are in the dataset's directory) in the gene's slot at contact
    frequency freqs[q], in the prediction column's quantity --, slot [n] (-1 = not placed), placed [n], candidates [C] (names),
    freqs [Q].  ds: the dataset the store was built from."""
    from .transplant import library_from_regions, pcre_transplant_dataset, read_bed
    library = library_from_regions(ds, read_bed(bed))
    rows = list(pcre_transplant_dataset(model, ds, library, list(freqs), slot=slot, genes=list(gene_ids), bsz=bsz, store=store))

    def quantity(lg):
        lg = np.asarray(lg, dtype=np.float32)
        return lg[..., 0] if regression else torch.sigmoid(torch.from_numpy(lg)).numpy()[..., 1]

    _savez(out, gene_ids=np.array(list(gene_ids)), prediction=quantity(np.stack([r["logits"] for r in rows])),
           transplant=quantity(np.stack([r["transplant"] for r in rows])), slot=np.array([r["slot"] for r in rows], dtype=np.int32),
           placed=np.array([r["placed"] for r in rows], dtype=bool), candidates=np.array(library.names),
           freqs=np.array(list(freqs), dtype=np.float32))


def write_integrated_gradients(model, store, bsz, ig_dir, n_steps=50, method="gausslegendre", target=None):
    """Integrated gradients of every gene of a device-resident store, in store order, into `ig_dir`: promoter_feats_{b}.npy
    [n, L, F], pcre_feats_{b}.npy [n, i_max, L, F], interaction_freq.npy [n, T, T] and delta.npy [n] (float32 .npy memory maps;
    nothing is gathered in host memory).  Zero baseline, every float input interpolated.  Per batch: one device gather into a Slot
    and one model.integrated_gradients."""
    import os
    n, S, T, F = len(store), model.i_max, model.i_max + 1, model.n_feats
    os.makedirs(ig_dir, exist_ok=True)

    def mm(name, shape):
        return np.lib.format.open_memmap(os.path.join(ig_dir, name + ".npy"), mode="w+", dtype=np.float32, shape=(n,) + shape)

    outs = {}
    for b, nb in zip(model.binsizes, model.n_bins):
        outs["promoter_feats", b] = mm("promoter_feats_%d" % b, (nb, F))
        outs["pcre_feats", b] = mm("pcre_feats_%d" % b, (S, nb, F))
    outs["interaction_freq", None] = mm("interaction_freq", (T, T))
    outs["delta", None] = mm("delta", ())
    for lo, B, slot in _slot_batches("write_integrated_gradients", model, store, bsz):
        attr, info = model.integrated_gradients(slot, target=target, n_steps=n_steps, method=method)
        attr["delta"] = info["delta"]
        for (key, b), m in outs.items():
            m[lo:lo + B] = (attr[key] if b is None else attr[key][b]).cpu().numpy()
    for m in outs.values():
        m.flush()


def write_perturbation_scan(model, store, bsz, path, gene_ids, strands, regression=False, scale=0.0, width=1, regions="promoter",
                            mark_sets=None):
    """In-silico perturbation scan of every gene of a device-resident store, in store order (model.perturbation_scan: the marks of a
    mark set scaled by `scale` in raw-signal space over each window of `width` coarsest bins) into `path`, an .npz holding

        gene_ids     [n]
        mark_sets    [n_sets, n_feats] bool: the marks of each set (default: each mark alone, then all together)
        prediction   float32 [n]: the prediction column's quantity (sigmoid(logits)[:, 1], or logits[:, 0] for the regressor) of the
                     unperturbed gene, through the very sigmoid call predict() makes: the CSV column bit for bit
        promoter     float32 [n, n_sets, W], W = the coarsest resolution's bins: the same quantity with set k scaled over window g of
                     the promoter (genomic order: `strands` undoes the mirror of '-' strand promoters); NaN where the window holds no
                     real bin
        pcres        float32 [n, i_max, n_sets, W], with regions="all": the same per pCRE slot (NaN for dummy slots)

    Per batch: one device gather into a Slot and one model.perturbation_scan_regions over the scanned regions."""
    from .attribution import scan_mark_sets, scan_regions_expand, scan_row
    n, S, F = len(store), model.i_max, model.n_feats
    mark_sets = scan_mark_sets(mark_sets, F)
    K = len(mark_sets)
    rc = int(np.argmin(model.n_bins))
    W = model.n_bins[rc]
    V = 1 + K * W
    scanned = scan_regions_expand("all" if regions == "all" else "promoter", S, "write_perturbation_scan")
    logits = torch.empty(len(scanned), n, V, model.n_out)
    live = torch.zeros(len(scanned), n, W, dtype=torch.bool)      # window g of the region holds a real bin
    flip = torch.tensor([s != "+" for s in strands], dtype=torch.uint8, device=model._device)
    for lo, B, slot in _slot_batches("write_perturbation_scan", model, store, bsz):
        out, _ = model.perturbation_scan_regions(slot, regions=scanned, scale=scale, width=width, mark_sets=mark_sets, flip=flip[lo:lo + B])
        logits[:, lo:lo + B] = out.cpu()
        for k, region in enumerate(scanned):
            m = (store.pm[rc][lo:lo + B] if region == 0 else store.cm[rc][lo:lo + B, region - 1]).reshape(B, W).cpu() == 0
            pos = torch.arange(W)
            first = torch.where(m, pos, W).amin(1)
            last = torch.where(m, pos, -1).amax(1)
            live[k, lo:lo + B] = pos[None, :] < (last - first + 1).clamp(min=0)[:, None]

    def column(lg):          # [n, n_out], laid out as the logits predict() turns into its column
        lg = lg.contiguous()
        return lg.numpy().reshape(-1) if regression else torch.sigmoid(lg).numpy()[:, 1]

    vals = np.empty((len(scanned), n, V), dtype=np.float32)
    for k in range(len(scanned)):
        for v in range(V):
            vals[k, :, v] = column(logits[k, :, v])
    scan = vals[:, :, scan_row(0, 0, 0, K, W):].reshape(len(scanned), n, K, W)
    scan[~np.broadcast_to(live.numpy()[:, :, None, :], scan.shape)] = np.nan
    sets = np.zeros((K, F), dtype=bool)
    for k, ms in enumerate(mark_sets):
        sets[k, list(ms)] = True
    arrays = dict(gene_ids=np.array(list(gene_ids)), mark_sets=sets, prediction=vals[0, :, scan_row(0, None, None, K, W)].copy(), promoter=scan[0])
    if regions == "all":
        arrays["pcres"] = np.ascontiguousarray(scan[1:].transpose(1, 0, 2, 3))
    _savez(path, **arrays)


def write_perturbation_scan_fine(model, dataset, store, bsz, path, gene_ids, regression=False, region="promoter", width=1, stride=None, zoom=None,
                                 scale=0.0, mark_sets=None):
    """Fine-resolution perturbation scan of every gene of `dataset` (attribution.perturbation_scan_fine on the device-resident `store`,
    which holds `gene_ids` in order: windows of `width` finest bins, `stride` apart, of the promoter or of one pCRE slot) into `path`, an
    .npz holding

        gene_ids     [n]
        mark_sets    [n_sets, n_feats] bool: the marks of each set (default: each mark alone, then all together)
        prediction   float32 [n]: the prediction column's quantity (sigmoid(logits)[:, 1], or logits[:, 0] for the regressor)
        chroms       [n] and windows int64 [n, n_win, 2]: genomic start and end of each window (-1 where the gene has fewer windows)
        scan         float32 [n, n_sets, n_win]: the same quantity with set k scaled by `scale` over window g; NaN where windows is -1
        zoom         int64 [n, k], coarse_windows int64 [n, W, 2] and coarse float32 [n, n_sets, W], with zoom = k: the k coarse windows
                     that were fine-scanned, most important first, and the coarse scan they were chosen from (-1 / NaN padding)"""
    from .attribution import perturbation_scan_fine
    col = (lambda lg: lg[..., 0]) if regression else (lambda lg: torch.sigmoid(torch.from_numpy(np.ascontiguousarray(lg))).numpy()[..., 1])
    res = list(perturbation_scan_fine(model, dataset, genes=list(gene_ids), region=region, zoom=zoom, scale=scale, width=width, stride=stride,
                                      mark_sets=mark_sets, bsz=bsz, store=store))
    n, K, F = len(res), len(res[0]["mark_sets"]) if res else 0, model.n_feats
    n_win = max([len(d["windows"]) for d in res] + [0])
    windows = np.full((n, n_win, 2), -1, dtype=np.int64)
    scan = np.full((n, K, n_win), np.nan, dtype=np.float32)
    for i, d in enumerate(res):
        m = len(d["windows"])
        windows[i, :m] = np.array([w[1:] for w in d["windows"]], dtype=np.int64).reshape(m, 2)
        scan[i, :, :m] = col(d["scan"])
    sets = np.zeros((K, F), dtype=bool)
    for k, ms in enumerate(res[0]["mark_sets"] if res else []):
        sets[k, list(ms)] = True
    arrays = dict(gene_ids=np.array(list(gene_ids)), mark_sets=sets, prediction=np.array([col(d["logits"]) for d in res], dtype=np.float32),
                  chroms=np.array([d["region"][0] if d["region"] else "" for d in res]), windows=windows, scan=scan)
    if zoom is not None:
        W = max([len(d["coarse_windows"]) for d in res] + [0])
        arrays["zoom"] = np.full((n, int(zoom)), -1, dtype=np.int64)
        arrays["coarse_windows"] = np.full((n, W, 2), -1, dtype=np.int64)
        arrays["coarse"] = np.full((n, K, W), np.nan, dtype=np.float32)
        for i, d in enumerate(res):
            m = len(d["coarse_windows"])
            arrays["zoom"][i, :len(d["zoom"])] = d["zoom"]
            arrays["coarse_windows"][i, :m] = np.array([w[1:] for w in d["coarse_windows"]], dtype=np.int64).reshape(m, 2)
            arrays["coarse"][i, :, :m] = col(d["coarse_scan"])
    _savez(path, **arrays)


def require_raw_signals(dataset, genes=None):
    """Raw-signal saliency reads the raw .npy regions themselves; a packed store holds binned features only.  Raises FileNotFoundError
    naming the first region file of `genes` (default: the dataset's) that is missing."""
    import os
    ds = dataset
    for gene in (ds.target_genes if genes is None else genes):
        g = ds.genes[gene]
        chrom, tss, _ = g["tss"]
        for region in [(chrom, tss - 20000, tss + 20000)] + list(g["pcres"]):
            path = "%s/%s:%d-%d.npy" % ((ds.npy_dir,) + tuple(region))
            if not os.path.exists(path):
                raise FileNotFoundError("raw-signal saliency: %s is missing (gene %s); raw signals are required -- a packed store holds the "
                                        "binned features only, keep the .npy files next to it" % (path, gene))


def write_raw_saliency(model, dataset, bsz, saliency_dir, target=None, times_input=False):
    """Raw-signal saliency of every gene of a dataset (model.raw_signal_gradients) into `saliency_dir`/<gene_id>.npz: `promoter`
    float32 [F, window] and `pcre_<s>` float32 [F, len_s] in genomic orientation, `regions` (a string array "chrom:start-end", the
    promoter window first: sample s of a track is position start + s), `logits` [n_out]."""
    import os
    os.makedirs(saliency_dir, exist_ok=True)
    require_raw_signals(dataset)
    for d in model.raw_signal_gradients(dataset, target=target, times_input=times_input, bsz=bsz):
        arrays = {"promoter": d["promoter"], "logits": d["logits"],
                  "regions": np.array(["%s:%d-%d" % tuple(r) for r in d["regions"]])}
        for s, t in enumerate(d["pcres"]):
            arrays["pcre_%d" % s] = t
        np.savez(os.path.join(saliency_dir, "%s.npz" % d["gene_id"]), **arrays)


def write_raw_integrated_gradients(model, dataset, bsz, ig_dir, n_steps=50, method="gausslegendre", target=None, donor_dataset=None):
    """Integrated gradients in raw-signal space of every gene of a dataset (model.raw_integrated_gradients: zero-signal baseline, path
    a * x) into `ig_dir`/<gene_id>.npz: the keys of write_raw_saliency (`promoter`, `pcre_<s>`, `regions`, `logits`; the tracks hold
    the per-sample attributions) plus `baseline_logits` [n_out] and `delta` (the tracks' sum minus logits - baseline_logits at the
    target: the quadrature error).  With donor_dataset the baseline is that cell type's signal over the same regions (path
    xd + a (x - xd)) and every file also holds `donor_prediction` [n_out], the donor dataset's own forward of the gene."""
    import os
    os.makedirs(ig_dir, exist_ok=True)
    require_raw_signals(dataset)
    if donor_dataset is not None:
        require_raw_signals(donor_dataset)
    for d in model.raw_integrated_gradients(dataset, target=target, n_steps=n_steps, method=method, bsz=bsz, donor_dataset=donor_dataset):
        arrays = {"promoter": d["promoter"], "logits": d["logits"], "baseline_logits": d["baseline_logits"], "delta": d["delta"],
                  "regions": np.array(["%s:%d-%d" % tuple(r) for r in d["regions"]])}
        if donor_dataset is not None:
            arrays["donor_prediction"] = d["donor_prediction"]
        for s, t in enumerate(d["pcres"]):
            arrays["pcre_%d" % s] = t
        np.savez(os.path.join(ig_dir, "%s.npz" % d["gene_id"]), **arrays)


# the outputs that read the donor cell type, predict()'s arguments and main()'s options alike, in the order the refusals list them
_CONTACT_DONOR_OUTS = ("contact_donor_shapley_out",)          # (reads the donor too; apart, as the next)
_BACKSELECT_DONOR_OUTS = ("mark_donor_backselect_out",)      # (reads the donor too; apart, so that the refusals below keep their wording)
_DONOR_OUTS = ("mark_donor_shapley_out", "mark_donor_epistasis_out", "mark_donor_sampled_shapley_out", "window_donor_shapley_out",
               "fine_window_donor_shapley_out", "mark_donor_interactions_out", "mark_donor_sampled_interactions_out", "mark_donor_dividends_out")


def predict(meta_path, npy_dir, weights=None, regression=False, bsz=32, seed=123, i_max=8, w_prom=40000, w_max=40000,
            binsizes=(2000, 500, 100), progress=False, store_path=None, attention_dir=None, embeddings_out=None,
            pcre_ablation_out=None, ig_dir=None, ig_steps=50, ig_method="gausslegendre", ig_target=None, raw_saliency_dir=None,
            raw_saliency_target=None, raw_saliency_times_input=False, raw_ig_dir=None, scan_out=None, scan_scale=0.0, scan_width=1,
            scan_regions="promoter", pcre_shapley_out=None, pcre_epistasis_out=None, mark_shapley_out=None, mark_epistasis_out=None,
            mark_players="marks", mark_scale=0.0, donor_npy_dir=None, donor_meta=None, donor_store_path=None, mark_donor_shapley_out=None,
            mark_donor_epistasis_out=None, mark_sampled_shapley_out=None, mark_donor_sampled_shapley_out=None, mark_sampled_players="cells",
            mark_perms=64, mark_seed=0, window_shapley_out=None, window_donor_shapley_out=None, window_players="promoter", window_width=1,
            window_perms=64, window_seed=0, window_scale=0.0, raw_donor_ig_dir=None, fine_scan_out=None, fine_scan_region="promoter",
            fine_scan_width=1, fine_scan_stride=None, fine_scan_zoom=None, fine_scan_scale=0.0, fine_window_shapley_out=None,
            fine_window_donor_shapley_out=None, fine_window_region="promoter", fine_window_width=2, fine_window_players="windows",
            fine_window_zoom=1, fine_window_perms=64, fine_window_seed=0, fine_window_scale=0.0, pcre_interactions_out=None,
            mark_interactions_out=None, mark_donor_interactions_out=None, interaction_index="sii", mark_sampled_interactions_out=None,
            mark_donor_sampled_interactions_out=None, mark_focal=4, pcre_dividends_out=None, mark_dividends_out=None,
            mark_donor_dividends_out=None, mark_backselect_out=None, mark_donor_backselect_out=None, mark_backselect_players="cells",
            backselect_mode="backward", backselect_frac=0.9, contact_shapley_out=None, contact_players="contacts", contact_scale=0.0,
            contact_interactions_out=None, contact_dividends_out=None, contact_donor_shapley_out=None, contact_donor_marks="own",
            transplant_bed=None, transplant_out=None, transplant_freq=(1.0, 5.0, 10.0), transplant_slot="append"):
    """-> (meta DataFrame, predictions float32 [n_genes]) in the order of the metadata file.  attention_dir / embeddings_out: also
    write the attention maps / regulatory embeddings of every gene, in the same order (write_attention_maps); pcre_ablation_out:
    the predictions with each pCRE deleted (write_pcre_ablation); ig_dir: integrated gradients of every gene
    (write_integrated_gradients); raw_saliency_dir: the gradient (or gradient x input) of the prediction with respect to the raw
    signals, one .npz per gene (write_raw_saliency; needs the raw .npy files also when a packed store serves the predictions);
    raw_ig_dir: integrated gradients with respect to the raw signals, one .npz per gene (write_raw_integrated_gradients; ig_steps,
    ig_method and ig_target apply; needs the raw .npy files too); scan_out: the in-silico perturbation scan of every gene, one .npz
    (write_perturbation_scan; scan_scale, scan_width and scan_regions apply; served by a packed store as well); pcre_shapley_out /
    pcre_epistasis_out: exact Shapley values / pair-deletion epistasis of the pCREs, in logit space (write_exact_values, game "pcre");
    mark_shapley_out / mark_epistasis_out: exact Shapley values / pair epistasis of the histone marks, in logit space
    (game "mark"; mark_players and mark_scale apply); mark_donor_shapley_out / mark_donor_epistasis_out: the same against a donor
    cell type (game "mark_donor"; mark_players applies), whose signals are read from donor_npy_dir with the metadata donor_meta
    (default: meta_path) or the packed store donor_store_path -- both cell types must hold the genes' regions at the same coordinates
    (attribution.same_regions); mark_sampled_shapley_out / mark_donor_sampled_shapley_out: permutation-sampled Shapley values of up
    to 128 mark players, by default one per (mark, region) pair, under the scale rule (mark_scale applies) / against the donor
    (write_mark_sampled_values; mark_sampled_players, mark_perms and mark_seed apply); window_shapley_out /
    window_donor_shapley_out: Shapley values of window players -- stretches of the promoter or of every region -- under the scale
    rule (window_scale applies) / against the donor, exact with at most 16 players and sampled otherwise (write_mark_window_values;
    window_players, window_width, window_perms and window_seed apply); raw_donor_ig_dir: integrated gradients with respect to the raw
    signals against the donor cell type's signals of donor_npy_dir, one .npz per gene (write_raw_integrated_gradients with the donor's
    dataset; ig_steps, ig_method and ig_target apply; needs the raw .npy files of both cell types); fine_scan_out: the fine-resolution
    perturbation scan of every gene, one .npz (write_perturbation_scan_fine; fine_scan_region -- "promoter" or a pCRE slot --,
    fine_scan_width, fine_scan_stride, fine_scan_zoom and fine_scan_scale apply; served by a packed store as well);
    fine_window_shapley_out / fine_window_donor_shapley_out: Shapley values of fine window players inside each gene's most important
    coarse windows, under the scale rule (fine_window_scale applies) / against the donor (write_mark_fine_window_values;
    fine_window_region, fine_window_width, fine_window_players, fine_window_zoom, fine_window_perms and fine_window_seed apply);
    pcre_interactions_out / mark_interactions_out / mark_donor_interactions_out: the pairwise Shapley interaction index
    interaction_index ("sii" / "sti") of the pCREs / the histone marks / the marks against the donor, a float32 .npy [n_genes, P, P] in
    logit space, by the writers of the Shapley values of the same game (one interactions call serves both outputs);
    mark_sampled_interactions_out / mark_donor_sampled_interactions_out: the SAMPLED interaction index of each gene's focal players
    among up to 128 mark players, one .npz, under the scale rule (mark_scale applies) / against the donor
    (write_mark_sampled_interactions; mark_focal -- an int: each gene's strongest players by |phi|; a list of names or indices: those
    for every gene --, mark_sampled_players, mark_perms, mark_seed and interaction_index apply); pcre_dividends_out /
    mark_dividends_out / mark_donor_dividends_out: the Harsanyi dividends of every set of pCREs / histone marks / marks against the
    donor, one .npz in logit space (write_dividends; mark_players applies to the mark games, mark_scale to mark_dividends_out);
    mark_backselect_out / mark_donor_backselect_out: the greedy selection order, the deletion curve and the smallest sufficient subset
    of up to 128 mark players, one .npz, under the scale rule (mark_scale applies) / against the donor (write_mark_backselect;
    mark_backselect_players, backselect_mode and backselect_frac apply); contact_shapley_out / contact_interactions_out /
    contact_dividends_out: exact Shapley values / the pairwise interaction index interaction_index / the Harsanyi dividends of contact
    players, whose absence scales the promoter-pCRE contact frequencies by contact_scale (write_contact_values; contact_players --
    "contacts", "pcres", "pcres_and_contacts" or "all" -- applies); contact_donor_shapley_out: the Shapley values of the same players
    against the donor cell type's contact frequencies, on the gene's own features or, with contact_donor_marks="donor", on the
    donor's (contact_players applies); transplant_bed + transplant_out: the pCRE transplant screen of the BED file's regions, each in
    the slot transplant_slot ("append" or a slot) of every gene at the contact frequencies transplant_freq (write_transplant)."""
    if transplant_bed or transplant_out:      # (refusals before anything is computed)
        from .transplant import broadcast_freq, read_bed, slot_argument
        if not (transplant_bed and transplant_out):
            raise ValueError("predict: transplant_bed and transplant_out go together")
        read_bed(transplant_bed)
        transplant_freq = [float(f) for f in np.atleast_1d(np.asarray(transplant_freq, dtype=np.float64))]
        broadcast_freq(transplant_freq, 1, 1, "predict")
        if not isinstance(transplant_slot, (str, int, np.integer)):
            raise ValueError("predict: transplant_slot = %r: 'append' or a slot" % (transplant_slot,))
        slot_argument(transplant_slot, 1, i_max, "predict")
    if contact_shapley_out or contact_interactions_out or contact_dividends_out or contact_donor_shapley_out:      # (refusals before anything is computed)
        from .attribution import contact_players as _contact
        _contact(contact_players, i_max)
        if contact_interactions_out and len(_contact(contact_players, i_max)[2]) < 2:
            raise ValueError("predict: contact_interactions_out needs at least 2 players; contact_players = %r has 1" % (contact_players,))
        if not np.isfinite(contact_scale):
            raise ValueError("predict: contact_scale = %r: a finite factor" % (contact_scale,))
        if contact_donor_marks not in ("own", "donor"):
            raise ValueError("predict: contact_donor_marks = %r: 'own' or 'donor'" % (contact_donor_marks,))
    if mark_backselect_out or mark_donor_backselect_out:      # (refusals before anything is computed)
        from .attribution import mark_players_wide as _wide
        _wide(mark_backselect_players, 7, i_max)
        if backselect_mode not in ("backward", "forward") or not np.isfinite(backselect_frac):
            raise ValueError("predict: backselect_mode = %r ('backward' / 'forward'), backselect_frac = %r (finite)" % (backselect_mode, backselect_frac))
    from .attribution import interaction_index as _index_check
    _index_check(interaction_index, "predict")      # (before anything is computed)
    pairs_ds, pairs_kw = None, {}
    if mark_sampled_interactions_out or mark_donor_sampled_interactions_out:      # (refusals before anything is computed)
        from .attribution import focal_players, mark_players_wide
        pair_names = mark_players_wide(mark_sampled_players, 7, i_max)[2]
        if isinstance(mark_focal, (int, np.integer)) and not isinstance(mark_focal, bool):
            if not 1 <= mark_focal <= len(pair_names):
                raise ValueError("predict: mark_focal = %d outside 1..%d" % (mark_focal, len(pair_names)))
            pairs_kw = dict(top=int(mark_focal))
        else:
            pairs_kw = dict(focal=focal_players(mark_focal, pair_names, len(pair_names)))
        pairs_kw.update(players=mark_sampled_players, index=interaction_index, n_perm=mark_perms, seed=mark_seed)
    seed_everything(seed)
    meta = pd.read_csv(meta_path)
    genes = meta.gene_id.tolist()
    raw_ds = None
    if raw_saliency_dir or raw_ig_dir or raw_donor_ig_dir:
        raw_ds = ChromoformerDataset(meta_path, npy_dir, genes, 7, i_max, list(binsizes), w_prom, w_max, regression=regression)
        require_raw_signals(raw_ds)      # (before anything is computed)
    from . import pack
    given = locals()      # (the arguments by name)
    donor_out = any(given[name] for name in _DONOR_OUTS + _BACKSELECT_DONOR_OUTS + _CONTACT_DONOR_OUTS)
    plain = []

    def plain_ds():      # the run's dataset with regression=False: strand, coordinates and geometry for the generators; built at its first use
        if not plain:
            plain.append(ChromoformerDataset(meta_path, npy_dir, genes, 7, i_max, list(binsizes), w_prom, w_max, regression=False))
        return plain[0]

    if pairs_kw:      # (the geometry the generator checks the model against)
        pairs_ds = plain_ds()
    raw_donor_ds = None
    if raw_donor_ig_dir:      # (before anything is computed)
        from .attribution import same_regions
        if not donor_npy_dir:
            raise ValueError("predict: raw_donor_ig_dir needs donor_npy_dir")
        raw_donor_ds = ChromoformerDataset(donor_meta or meta_path, donor_npy_dir, genes, 7, i_max, list(binsizes), w_prom, w_max, regression=regression)
        require_raw_signals(raw_donor_ds)
        same_regions(raw_ds, raw_donor_ds)
    window_ds = None
    if window_shapley_out or window_donor_shapley_out:      # (strand and coordinates; refusals before anything is computed)
        from .attribution import window_players as window_game
        window_game(window_players, 7, i_max, w_max // max(binsizes), window_width)
        window_ds = plain_ds()
    fine_window_ds = None
    if fine_window_shapley_out or fine_window_donor_shapley_out:      # (strand, coordinates, lengths; refusals before anything is computed)
        from .attribution import fine_window_players as fine_window_game
        fine_window_game(fine_window_players, 7, fine_window_width, -(-(max(binsizes) // min(binsizes)) // max(int(fine_window_width), 1)))
        fine_window_ds = plain_ds()
    if donor_out:      # (before anything is computed)
        from .attribution import same_regions
        if not donor_npy_dir:
            raise ValueError("predict: %s need donor_npy_dir" % " / ".join(_DONOR_OUTS + _CONTACT_DONOR_OUTS))
        donor_ds = ChromoformerDataset(donor_meta or meta_path, donor_npy_dir, genes, 7, i_max, list(binsizes), w_prom, w_max, regression=False)
        same_regions(plain_ds(), donor_ds)
    packed = pack.find(npy_dir, store_path, list(binsizes), i_max, w_prom, w_max, 7, genes, meta=meta)
    dev = torch.device("cuda", torch.cuda.current_device())
    if packed is not None:
        store = packed.store(genes, device=dev, regression=False)          # labels are not used for prediction
    else:
        ds = ChromoformerDataset(meta_path, npy_dir, genes, 7, i_max, list(binsizes), w_prom, w_max, regression=regression)
        store = GeneStore(ds, progress=progress, device=dev, resident=True)      # binned on the GPU, resident (126 KB per gene)
    Model = ChromoformerRegressor if regression else ChromoformerClassifier
    model = Model(7, 128, 128, dict(n_layers=1, n_heads=2, d_model=128, d_ff=128), dict(n_layers=2, n_heads=2, d_model=128, d_ff=256),
                  dict(n_layers=6, n_heads=8, d_model=256, d_ff=256), binsizes=list(binsizes), seed=seed, i_max=i_max, w_max=w_max,
                  max_batch=bsz)
    if weights is not None:
        ckpt = torch.load(weights, map_location="cpu", weights_only=False)
        model.load_state_dict(modernise_keys(ckpt["net"] if "net" in ckpt else ckpt))
    model.cuda()
    trainer = Trainer(model, use_graph=False)
    out = trainer.evaluate_store(store, bsz).cpu()          # device gather + forward per batch, logits in store order
    preds = [out.numpy().reshape(-1) if regression else torch.sigmoid(out).numpy()[:, 1]]
    write_attention_maps(model, store, bsz, attention_dir, embeddings_out)
    if pcre_ablation_out:
        write_pcre_ablation(model, store, bsz, pcre_ablation_out, regression)
    if pcre_shapley_out or pcre_epistasis_out or pcre_interactions_out:
        write_exact_values(model, "pcre", store, None, bsz, genes, pcre_shapley_out, pcre_epistasis_out, pcre_interactions_out, regression,
                           index=interaction_index)
    if mark_shapley_out or mark_epistasis_out or mark_interactions_out:
        write_exact_values(model, "mark", store, None, bsz, genes, mark_shapley_out, mark_epistasis_out, mark_interactions_out, regression,
                           mark_players, mark_scale, interaction_index)
    if pcre_dividends_out:
        write_dividends(model, store, None, bsz, genes, pcre_dividends_out, "pcre", regression)
    if mark_dividends_out:
        write_dividends(model, store, None, bsz, genes, mark_dividends_out, "mark", regression, mark_players, mark_scale)
    if donor_out:
        donor_packed = pack.find(donor_npy_dir, donor_store_path, list(binsizes), i_max, w_prom, w_max, 7, genes, meta=donor_ds.meta)
        donor_store = (donor_packed.store(genes, device=dev, regression=False) if donor_packed is not None
                       else GeneStore(donor_ds, progress=progress, device=dev, resident=True))
        if mark_donor_shapley_out or mark_donor_epistasis_out or mark_donor_interactions_out:
            write_exact_values(model, "mark_donor", store, donor_store, bsz, genes, mark_donor_shapley_out, mark_donor_epistasis_out,
                               mark_donor_interactions_out, regression, mark_players, index=interaction_index)
        if mark_donor_dividends_out:
            write_dividends(model, store, donor_store, bsz, genes, mark_donor_dividends_out, "mark_donor", regression, mark_players)
        if mark_donor_sampled_shapley_out:
            write_mark_sampled_values(model, store, donor_store, bsz, genes, mark_donor_sampled_shapley_out, regression, mark_sampled_players,
                                      mark_perms, mark_seed)
        if mark_donor_sampled_interactions_out:
            write_mark_sampled_interactions(model, pairs_ds, donor_ds, store, donor_store, bsz, genes, mark_donor_sampled_interactions_out, regression,
                                            **pairs_kw)
        if contact_donor_shapley_out:
            write_contact_values(model, plain_ds(), donor_ds, store, donor_store, bsz, genes, contact_donor_shapley_out, None, None, regression,
                                 contact_players, marks=contact_donor_marks)
        if mark_donor_backselect_out:
            write_mark_backselect(model, store, donor_store, bsz, genes, mark_donor_backselect_out, regression, mark_backselect_players,
                                  backselect_mode, backselect_frac)
        if window_donor_shapley_out:
            write_mark_window_values(model, window_ds, donor_ds, store, donor_store, bsz, genes, window_donor_shapley_out, regression, window_players,
                                     window_width, window_perms, window_seed)
        if fine_window_donor_shapley_out:
            write_mark_fine_window_values(model, fine_window_ds, donor_ds, store, donor_store, bsz, genes, fine_window_donor_shapley_out, regression,
                                          fine_window_region, fine_window_width, fine_window_players, fine_window_zoom, fine_window_perms,
                                          fine_window_seed)
        del donor_store
    if contact_shapley_out or contact_interactions_out or contact_dividends_out:
        write_contact_values(model, plain_ds(), None, store, None, bsz, genes, contact_shapley_out, contact_interactions_out, contact_dividends_out,
                             regression, contact_players, contact_scale, index=interaction_index)
    if mark_sampled_shapley_out:
        write_mark_sampled_values(model, store, None, bsz, genes, mark_sampled_shapley_out, regression, mark_sampled_players, mark_perms, mark_seed,
                                  mark_scale)
    if mark_sampled_interactions_out:
        write_mark_sampled_interactions(model, pairs_ds, None, store, None, bsz, genes, mark_sampled_interactions_out, regression, scale=mark_scale,
                                        **pairs_kw)
    if mark_backselect_out:
        write_mark_backselect(model, store, None, bsz, genes, mark_backselect_out, regression, mark_backselect_players, backselect_mode,
                              backselect_frac, mark_scale)
    if window_shapley_out:
        write_mark_window_values(model, window_ds, None, store, None, bsz, genes, window_shapley_out, regression, window_players, window_width,
                                 window_perms, window_seed, window_scale)
    if fine_window_shapley_out:
        write_mark_fine_window_values(model, fine_window_ds, None, store, None, bsz, genes, fine_window_shapley_out, regression, fine_window_region,
                                      fine_window_width, fine_window_players, fine_window_zoom, fine_window_perms, fine_window_seed, fine_window_scale)
    if ig_dir:
        write_integrated_gradients(model, store, bsz, ig_dir, ig_steps, ig_method, ig_target)
    if transplant_out:      # (the candidates' raw files are binned by the dataset's own code)
        write_transplant(model, plain_ds(), store, bsz, genes, transplant_bed, transplant_out, regression, transplant_freq, transplant_slot)
    if fine_scan_out:      # (strand, coordinates and region lengths come from the metadata)
        write_perturbation_scan_fine(model, plain_ds(), store, bsz, fine_scan_out, genes, regression, fine_scan_region, fine_scan_width, fine_scan_stride,
                                     fine_scan_zoom, fine_scan_scale)
    if scan_out:
        write_perturbation_scan(model, store, bsz, scan_out, genes, meta.strand.tolist(), regression, scan_scale, scan_width, scan_regions)
    if raw_saliency_dir:
        write_raw_saliency(model, raw_ds, bsz, raw_saliency_dir, raw_saliency_target, raw_saliency_times_input)
    if raw_ig_dir:
        write_raw_integrated_gradients(model, raw_ds, bsz, raw_ig_dir, ig_steps, ig_method, ig_target)
    if raw_donor_ig_dir:
        write_raw_integrated_gradients(model, raw_ds, bsz, raw_donor_ig_dir, ig_steps, ig_method, ig_target, donor_dataset=raw_donor_ds)
    return meta, np.concatenate(preds).astype(np.float32)


def build_parser():
    ap = argparse.ArgumentParser(description="Chromoformer expression prediction on the MI355X path")
    ap.add_argument("-m", "--meta", required=True, help="Path to input metadata file.")
    ap.add_argument("-d", "--npy-dir", required=True, help="Path to directory containing histone signals in .npy files.")
    ap.add_argument("-o", "--output", required=True, help="Path to output expression prediction.")
    ap.add_argument("-w", "--weights", default=None, help="Path to pretrained Chromoformer weights in .pt format.")
    ap.add_argument("--regression", action="store_true", help="ChromoformerRegressor (run_demo_regression.py)")
    ap.add_argument("--store", default=None, help="packed store of `python -m chromoformer_amd.pack` (default: <npy-dir>/chromoformer.cfstore if present)")
    ap.add_argument("--attention-dir", default=None, help="also write DIR/{embed,pairwise_interaction,regulation}_{binsize}.npy: the "
                    "attention maps of every gene, in metadata order (model.attention_maps)")
    ap.add_argument("--embeddings-out", default=None, help="also write the regulatory embedding of every gene (the fc_head input, "
                    "[n_genes, 3 * d_emb]) to this .npy file, in metadata order")
    ap.add_argument("--pcre-ablation-out", default=None, help="also write in-silico pCRE deletion to this .npy file: [n_genes, i_max + 2] "
                    "predictions in metadata order, column 0 as --output, column 1 + j with pCRE j deleted, the last with the promoter "
                    "alone (model.pcre_ablation)")
    ap.add_argument("--pcre-shapley-out", default=None, help="also write the exact Shapley values of the pCREs to this .npz file, in metadata "
                    "order and in LOGIT space of the prediction's column (efficiency holds there, not after the sigmoid): phi [n_genes, i_max] "
                    "(0 for dummy slots), logits, promoter_only (phi sums to their difference) and n_pcres (model.pcre_shapley)")
    ap.add_argument("--pcre-epistasis-out", default=None, help="also write the pair-deletion epistasis of the pCREs to this .npy file: "
                    "[n_genes, i_max, i_max] in logit space, symmetric, the leave-one-out effects on the diagonal (model.pcre_epistasis)")
    from .attribution import INTERACTION_INDICES
    ap.add_argument("--pcre-interactions-out", default=None, help="also write the pairwise Shapley interaction index of the pCREs to this .npy "
                    "file: [n_genes, i_max, i_max] in logit space, symmetric, how much one pCRE's marginal contribution changes with the other "
                    "present, averaged over every coalition of the rest (negative: redundant, positive: cooperating); the diagonal as "
                    "--interaction-index says (model.pcre_shapley_interactions)")
    ap.add_argument("--interaction-index", default=None, choices=INTERACTION_INDICES, help="the index of --pcre-interactions-out / "
                    "--mark-interactions-out / --mark-donor-interactions-out: sii, the Shapley interaction index, the Shapley values on the "
                    "diagonal (default), or sti, Shapley-Taylor of order 2, v({i}) - v(nobody) on the diagonal (diagonal and upper triangle then "
                    "sum to the prediction's logit minus every player absent)")
    from .attribution import METHODS
    ap.add_argument("--ig-dir", default=None, help="also write integrated gradients (zero baseline, every float input) of every gene, in "
                    "metadata order, as DIR/promoter_feats_{binsize}.npy [n, L, F], DIR/pcre_feats_{binsize}.npy [n, i_max, L, F], "
                    "DIR/interaction_freq.npy [n, T, T] and DIR/delta.npy [n] (model.integrated_gradients).  About 126 KB per gene at the "
                    "default configuration: 2.4 GB for 18,955 genes")
    ap.add_argument("--ig-steps", type=int, default=None, help="quadrature nodes of --ig-dir (default 50)")
    ap.add_argument("--ig-method", default=None, choices=METHODS, help="quadrature of --ig-dir (default gausslegendre)")
    ap.add_argument("--ig-target", type=int, default=None, help="logit column of --ig-dir (default 1 for the classifier, 0 with --regression)")
    ap.add_argument("--raw-ig-dir", default=None, help="also write integrated gradients in raw-signal space (zero-signal baseline, path a * x): "
                    "DIR/<gene_id>.npz with the keys of --raw-saliency-dir, the tracks holding the per-sample attributions, plus "
                    "baseline_logits and delta (model.raw_integrated_gradients).  Takes --ig-steps, --ig-method and --ig-target; needs the "
                    "raw .npy files, also next to a packed store")
    ap.add_argument("--raw-saliency-dir", default=None, help="also write raw-signal saliency: DIR/<gene_id>.npz with the gradient of the "
                    "prediction's logit with respect to the raw .npy signals (promoter [7, window], pcre_<s> [7, len], genomic orientation, "
                    "regions, logits; model.raw_signal_gradients).  Needs the raw .npy files, also next to a packed store")
    ap.add_argument("--raw-saliency-target", type=int, default=None, help="logit column of --raw-saliency-dir (default 1 for the classifier, 0 "
                    "with --regression)")
    ap.add_argument("--raw-saliency-times-input", action="store_true", help="--raw-saliency-dir writes gradient x input")
    ap.add_argument("--scan-out", default=None, help="also write the in-silico perturbation scan to this .npz file: gene_ids, mark_sets "
                    "[n_sets, 7], prediction [n] (as --output) and promoter [n, n_sets, W]: the prediction with each mark alone, then all "
                    "marks, scaled by --scan-scale in raw-signal space over each window of the promoter, genomic order, NaN where a window "
                    "holds no real bin (model.perturbation_scan)")
    ap.add_argument("--scan-scale", type=float, default=None, help="scale factor of --scan-out: 0 erases the marks (default), 2 doubles them")
    ap.add_argument("--scan-width", type=int, default=None, help="window width of --scan-out in coarsest bins (default 1)")
    ap.add_argument("--scan-regions", default=None, choices=("promoter", "all"), help="--scan-out scans the promoter (default) or also every "
                    "pCRE slot: pcres [n, i_max, n_sets, W]")
    ap.add_argument("--fine-scan-out", default=None, help="also write the FINE-resolution perturbation scan to this .npz file: gene_ids, "
                    "mark_sets [n_sets, 7], prediction [n] (as --output), chroms [n], windows [n, n_win, 2] (genomic start and end, -1 padding) and "
                    "scan [n, n_sets, n_win]: the prediction with each mark alone, then all marks, scaled by --fine-scan-scale in raw-signal space "
                    "over windows of --fine-scan-width finest bins (100 bp), NaN padding (model.perturbation_scan_fine)")
    ap.add_argument("--fine-scan-region", default=None, help="the region --fine-scan-out scans: promoter (default) or a pCRE slot 0 .. 7")
    ap.add_argument("--fine-scan-width", type=int, default=None, help="window width of --fine-scan-out in finest bins (default 1)")
    ap.add_argument("--fine-scan-stride", type=int, default=None, help="distance between windows of --fine-scan-out in finest bins (default: the width)")
    ap.add_argument("--fine-scan-zoom", type=int, default=None, help="--fine-scan-out first runs the coarse scan and fine-scans, per gene, the K "
                    "coarse windows that move the prediction's logit most; also writes zoom [n, K], coarse_windows and coarse (default: the whole region)")
    ap.add_argument("--fine-scan-scale", type=float, default=None, help="scale factor of --fine-scan-out: 0 erases the marks (default), 2 doubles them")
    from .attribution import MARK_PLAYER_SPECS
    ap.add_argument("--mark-shapley-out", default=None, help="also write the exact Shapley values of the histone marks to this .npz file, in "
                    "metadata order and in LOGIT space of the prediction's column: gene_ids, players (names), phi [n_genes, P], logits and "
                    "erased (every player absent; phi sums to their difference) (model.mark_shapley)")
    ap.add_argument("--mark-epistasis-out", default=None, help="also write the pair epistasis of the histone marks to this .npy file: "
                    "[n_genes, P, P] in logit space, symmetric, the leave-one-out effects on the diagonal (model.mark_epistasis)")
    ap.add_argument("--mark-interactions-out", default=None, help="also write the pairwise Shapley interaction index of the histone marks to "
                    "this .npy file: [n_genes, P, P] in logit space, symmetric (model.mark_shapley_interactions).  --mark-players, --mark-scale "
                    "and --interaction-index apply")
    ap.add_argument("--mark-players", default=None, choices=MARK_PLAYER_SPECS, help="the players of --mark-shapley-out / --mark-epistasis-out: "
                    "each mark in every region (marks, the default), each mark in the promoter and in the pCREs (compartments), or all marks "
                    "per region (regions)")
    ap.add_argument("--mark-scale", type=float, default=None, help="what an absent mark's raw signal is scaled by: 0 erases it (default)")
    ap.add_argument("--raw-donor-ig-dir", default=None, help="also write integrated gradients in raw-signal space against the DONOR cell type of "
                    "--donor-npy-dir (path xd + a * (x - xd) between the two raw signals): DIR/<gene_id>.npz with the keys of --raw-ig-dir plus "
                    "donor_prediction; baseline_logits is the donor's signal under the gene's masks and frequencies "
                    "(model.raw_integrated_gradients(donor_dataset=...)).  Takes --ig-steps, --ig-method and --ig-target; needs the raw .npy "
                    "files of both cell types")
    ap.add_argument("--donor-npy-dir", default=None, help="directory of the .npy histone signals of a DONOR cell type over the same regions: "
                    "what an absent mark becomes in --mark-donor-shapley-out / --mark-donor-epistasis-out")
    ap.add_argument("--donor-meta", default=None, help="metadata file of the donor cell type (default: --meta); TSS, strand and pCREs of every "
                    "gene must equal those of --meta")
    ap.add_argument("--donor-store", default=None, help="packed store of the donor cell type (default: <donor-npy-dir>/chromoformer.cfstore if present)")
    ap.add_argument("--mark-donor-shapley-out", default=None, help="also write the exact Shapley values of the histone marks against the donor "
                    "cell type to this .npz file, in metadata order and in LOGIT space of the prediction's column: gene_ids, players (names), "
                    "phi [n_genes, P], logits, donor (every player's marks from the donor, the gene's masks and frequencies; phi sums to logits "
                    "- donor) and donor_prediction (the donor's own prediction) (model.mark_donor_shapley).  --mark-players applies")
    ap.add_argument("--mark-donor-epistasis-out", default=None, help="also write the pair epistasis of the histone marks against the donor cell "
                    "type to this .npy file: [n_genes, P, P] in logit space, symmetric, the leave-one-out effects on the diagonal "
                    "(model.mark_donor_epistasis).  --mark-players applies")
    ap.add_argument("--mark-donor-interactions-out", default=None, help="also write the pairwise Shapley interaction index of the histone marks "
                    "against the donor cell type to this .npy file: [n_genes, P, P] in logit space, symmetric "
                    "(model.mark_donor_shapley_interactions).  --mark-players and --interaction-index apply")
    from .attribution import MARK_WIDE_PLAYER_SPECS
    ap.add_argument("--mark-sampled-shapley-out", default=None, help="also write permutation-SAMPLED Shapley values of up to 128 histone-mark "
                    "players to this .npz file, in metadata order and in LOGIT space of the prediction's column: gene_ids, players (names), "
                    "permutations [n_perm, P], phi [n_genes, P], stderr [n_genes, P] (the standard error over the sampled orders: the sampling "
                    "error is reported, not bounded), logits and absent (every player absent; phi sums to their difference) "
                    "(model.mark_shapley_sampled).  --mark-scale applies")
    ap.add_argument("--mark-donor-sampled-shapley-out", default=None, help="the same against the donor cell type of --donor-npy-dir: an absent "
                    "player takes the donor's signal")
    ap.add_argument("--mark-sampled-players", default=None, choices=MARK_WIDE_PLAYER_SPECS, help="the players of --mark-sampled-shapley-out / "
                    "--mark-donor-sampled-shapley-out: one per (mark, region) pair (cells, the default: 63 players, phi reshapes to "
                    "[n_genes, i_max + 1, 7]), or the specs of --mark-players")
    ap.add_argument("--mark-perms", type=int, default=None, help="sampled orders of adding the players (default 64); each costs P - 1 forwards per gene")
    ap.add_argument("--mark-seed", type=int, default=None, help="seed of the sampled orders (default 0)")
    ap.add_argument("--mark-backselect-out", default=None, help="also write the greedy player selection of up to 128 histone-mark players to "
                    "this .npz file, in metadata order, on the prediction's logit column: gene_ids, players (names), mode, frac, order "
                    "[n_genes, P] (the player of each move), curve [n_genes, P + 1] (the logit after t moves: the deletion curve), size and "
                    "subset [n_genes, P] (the smallest sufficient set on the path: which few cells are enough on their own), threshold, "
                    "direction, logits and absent (chromoformer_amd.backselect.mark_backselect; deterministic, P (P + 1) / 2 + 1 forwards per gene).  "
                    "--mark-scale applies")
    ap.add_argument("--mark-donor-backselect-out", default=None, help="the same against the donor cell type of --donor-npy-dir: an absent "
                    "player takes the donor's signal")
    ap.add_argument("--mark-backselect-players", default=None, choices=MARK_WIDE_PLAYER_SPECS, help="the players of --mark-backselect-out / "
                    "--mark-donor-backselect-out: one per (mark, region) pair (cells, the default), or the specs of --mark-players")
    ap.add_argument("--backselect-mode", default=None, choices=("backward", "forward"), help="backward (default): start from every player and "
                    "remove the least needed one per round; forward: start from none and add the most useful one")
    ap.add_argument("--backselect-frac", type=float, default=None, help="a set is sufficient when it keeps this share of logits - absent "
                    "(default 0.9)")
    ap.add_argument("--mark-sampled-interactions-out", default=None, help="also write the SAMPLED pairwise Shapley interaction index of each gene's "
                    "focal mark players with every player to this .npz file, in metadata order and in LOGIT space of the prediction's column: "
                    "gene_ids, players (names), index, permutations, focal [n_genes, n_focal], interactions and stderr [n_genes, n_focal, P] (the "
                    "standard error over the sampled orders: the sampling error is reported, not bounded), phi and phi_stderr [n_genes, P], "
                    "logits and absent (model.mark_shapley_interactions_sampled).  --mark-focal, --mark-sampled-players, --mark-perms, "
                    "--mark-seed, --mark-scale and --interaction-index apply")
    ap.add_argument("--mark-donor-sampled-interactions-out", default=None, help="the same against the donor cell type of --donor-npy-dir: an "
                    "absent player takes the donor's signal")
    ap.add_argument("--mark-focal", default=None, help="the focal players of --mark-sampled-interactions-out / "
                    "--mark-donor-sampled-interactions-out: a number K (default 4): each gene's K strongest players by |phi| of a sampled Shapley "
                    "estimate on the same orders; or player names separated by commas (mark3@pcre0,mark0@promoter): those for every gene")
    ap.add_argument("--pcre-dividends-out", default=None, help="also write the Harsanyi dividends (the Moebius transform of the coalition "
                    "table) of every set of pCRE slots to this .npz file, in metadata order and in LOGIT space of the prediction's column: "
                    "gene_ids, players (names), sets [2^P] (set names by word), dividends [n_genes, 2^P] (they add up to the logit of every "
                    "coalition: which pCREs act alone, which together, in which combinations) and mass (the scale of a dividend's rounding "
                    "error) (model.pcre_dividends)")
    ap.add_argument("--mark-dividends-out", default=None, help="the same for the histone marks (model.mark_dividends).  --mark-players and "
                    "--mark-scale apply")
    ap.add_argument("--mark-donor-dividends-out", default=None, help="the same against the donor cell type of --donor-npy-dir: an absent mark "
                    "takes the donor's signal (model.mark_donor_dividends).  --mark-players applies")
    from .attribution import CONTACT_PLAYER_SPECS
    ap.add_argument("--contact-shapley-out", default=None, help="also write the exact Shapley values of CONTACT players -- the promoter-pCRE "
                    "contact frequencies of the pCRE slots, and / or the slots themselves -- to this .npz file, in metadata order and in LOGIT "
                    "space of the prediction's column: gene_ids, players (names), phi [n_genes, P] (0 for dummy slots), logits, erased (every "
                    "player absent; phi sums to their difference), freq [n_genes, i_max] and n_pcres (contact.contact_shapley): does a pCRE matter "
                    "through its chromatin state or through its contact with the promoter?")
    ap.add_argument("--contact-players", default=None, choices=CONTACT_PLAYER_SPECS, help="the players of the --contact-* outputs: each slot's "
                    "contact (contacts, the default), each slot deleted (pcres: the pCRE game), both, slot by slot (pcres_and_contacts: 16 "
                    "players) or one player holding every contact (all: the model without Hi-C)")
    ap.add_argument("--contact-scale", type=float, default=None, help="what an absent contact's frequency is scaled by: 0 erases it (default), "
                    "2 doubles it; any finite value")
    ap.add_argument("--contact-interactions-out", default=None, help="also write the pairwise Shapley interaction index of the contact players "
                    "to this .npy file: [n_genes, P, P] in logit space, symmetric (contact.contact_shapley_interactions).  --contact-players, "
                    "--contact-scale and --interaction-index apply")
    ap.add_argument("--contact-dividends-out", default=None, help="also write the Harsanyi dividends of every set of contact players to this "
                    ".npz file: gene_ids, players, sets [2^P], dividends and mass [n_genes, 2^P] (contact.contact_dividends).  --contact-players "
                    "and --contact-scale apply")
    ap.add_argument("--contact-donor-shapley-out", default=None, help="the Shapley values of the contact players against the donor cell type of "
                    "--donor-npy-dir: an absent contact takes the donor's frequency.  The keys of --contact-shapley-out with donor in place of "
                    "erased, plus donor_freq and marks.  --contact-players applies")
    ap.add_argument("--contact-donor-marks", default=None, choices=("own", "donor"), help="--contact-donor-shapley-out plays on the gene's own "
                    "features (own, the default) or on the donor's under the gene's masks (donor: logits is then the donor row of "
                    "--mark-donor-shapley-out, and the two games together account for the whole difference between the two cell types)")
    from .attribution import WINDOW_PLAYER_SPECS
    ap.add_argument("--window-shapley-out", default=None, help="also write the Shapley values of WINDOW players -- stretches of a region, in "
                    "coarsest bins -- to this .npz file, in metadata order and in LOGIT space of the prediction's column: gene_ids, players "
                    "(names), estimator (exact with at most 16 players, else sampled), phi [n_genes, P], stderr, logits, absent (every player "
                    "absent; phi sums to their difference), null (the window holds no real bin of the gene), chroms and windows [n_genes, P, 2] "
                    "(genomic start and end) and, sampled, permutations (model.mark_window_shapley / mark_window_shapley_sampled)")
    ap.add_argument("--window-donor-shapley-out", default=None, help="the same against the donor cell type of --donor-npy-dir: an absent "
                    "player's window takes the donor's signal")
    ap.add_argument("--window-players", default=None, choices=WINDOW_PLAYER_SPECS, help="the players of --window-shapley-out / "
                    "--window-donor-shapley-out: all marks per promoter window (promoter, the default), each mark per promoter window "
                    "(promoter_cells) or all marks per window of every region (regions); at most 128: widen the windows")
    ap.add_argument("--window-width", type=int, default=None, help="window width in coarsest bins (default 1)")
    ap.add_argument("--window-perms", type=int, default=None, help="sampled orders when there are more than 16 players (default 64)")
    ap.add_argument("--window-seed", type=int, default=None, help="seed of the sampled orders (default 0)")
    ap.add_argument("--window-scale", type=float, default=None, help="what an absent player's raw signal is scaled by inside its window: 0 "
                    "erases it (default); --window-shapley-out only")
    from .attribution import FINE_WINDOW_PLAYER_SPECS
    ap.add_argument("--fine-window-shapley-out", default=None, help="also write the Shapley values of FINE window players -- stretches of "
                    "finest bins inside each gene's most important coarse windows (the coarse window game runs first) -- to this .npz file, in "
                    "metadata order and in LOGIT space of the prediction's column: gene_ids, players (names), exact, zoom [n_genes, k] (the "
                    "chosen coarse windows), coarse_phi, phi and stderr [n_genes, k, P], logits, absent [n_genes, k], null, chroms and "
                    "windows [n_genes, k, P, 2] (genomic start and end) (model.mark_fine_window_shapley_dataset)")
    ap.add_argument("--fine-window-donor-shapley-out", default=None, help="the same against the donor cell type of --donor-npy-dir: an absent "
                    "player's window takes the donor's signal, in the coarse and in the fine game")
    ap.add_argument("--fine-window-region", default=None, help="the region the game plays in: promoter (default) or a pCRE slot 0..7")
    ap.add_argument("--fine-window-width", type=int, default=None, help="window width in finest bins (default 2)")
    ap.add_argument("--fine-window-players", default=None, choices=FINE_WINDOW_PLAYER_SPECS, help="all marks per fine window (windows, the "
                    "default) or each mark per fine window (cells); at most 128: widen the windows")
    ap.add_argument("--fine-window-zoom", type=int, default=None, help="coarse windows to zoom into per gene (default 1)")
    ap.add_argument("--fine-window-perms", type=int, default=None, help="sampled orders when a game has more than 16 players (default 64)")
    ap.add_argument("--fine-window-seed", type=int, default=None, help="seed of the sampled orders (default 0)")
    ap.add_argument("--fine-window-scale", type=float, default=None, help="what an absent player's raw signal is scaled by inside its window: 0 "
                    "erases it (default); --fine-window-shapley-out only")
    ap.add_argument("--transplant-bed", default=None, help="pCRE transplant screen: a BED file of candidate regions, `chrom start end [name]` "
                    "lines, whose raw chrom:start-end.npy files are in --npy-dir; each is tried in one pCRE slot of every gene "
                    "(transplant.pcre_transplant).  Needs --transplant-out")
    ap.add_argument("--transplant-out", default=None, help="write the transplant screen to this .npz file, in metadata order: prediction "
                    "[n_genes], transplant [n_genes, C, Q] (the prediction with candidate c in the gene's slot at contact frequency q), slot "
                    "(-1: not placed), placed, candidates, freqs.  Needs --transplant-bed")
    ap.add_argument("--transplant-freq", default=None, help="the contact frequencies of the screen, comma-separated (default 1,5,10)")
    ap.add_argument("--transplant-slot", default=None, help="append (default: each gene's first free slot; a gene without one is not "
                    "placed) or a slot in [0, 8), whose pCRE is replaced")
    return ap


_DEFAULTS = dict(      # what predict() gets for an option that was not given; main() tells "not given" by None until its checks are through
    ig_steps=50, ig_method="gausslegendre", ig_target=None, raw_saliency_target=None, scan_scale=0.0, scan_width=1, scan_regions="promoter",
    fine_scan_region="promoter", fine_scan_width=1, fine_scan_stride=None, fine_scan_zoom=None, fine_scan_scale=0.0, mark_players="marks",
    mark_scale=0.0, mark_sampled_players="cells", mark_perms=64, mark_seed=0, mark_focal=4, interaction_index="sii", window_players="promoter",
    window_width=1, window_perms=64, window_seed=0, window_scale=0.0, fine_window_region="promoter", fine_window_width=2,
    fine_window_players="windows", fine_window_zoom=1, fine_window_perms=64, fine_window_seed=0, fine_window_scale=0.0,
    mark_backselect_players="cells", backselect_mode="backward", backselect_frac=0.9, contact_players="contacts", contact_scale=0.0,
    contact_donor_marks="own", transplant_freq="1,5,10", transplant_slot="append")
_BACKSELECT_OUTS = ("mark_backselect_out",) + _BACKSELECT_DONOR_OUTS
_CONTACT_OUTS = ("contact_shapley_out", "contact_interactions_out", "contact_dividends_out")
_MARK_OUTS = ("mark_shapley_out", "mark_epistasis_out", "mark_interactions_out", "mark_dividends_out")
_DONOR_EXACT_OUTS = ("mark_donor_shapley_out", "mark_donor_epistasis_out", "mark_donor_interactions_out", "mark_donor_dividends_out")
_SAMPLED_OUTS = ("mark_sampled_shapley_out", "mark_donor_sampled_shapley_out")
_PAIRS_OUTS = ("mark_sampled_interactions_out", "mark_donor_sampled_interactions_out")
_WINDOW_OUTS = ("window_shapley_out", "window_donor_shapley_out")
_FINE_WINDOW_OUTS = ("fine_window_shapley_out", "fine_window_donor_shapley_out")
_MARK_NEED = ("--mark-players / --mark-scale need --mark-shapley-out, --mark-epistasis-out, --mark-interactions-out or --mark-dividends-out"
              " (--mark-players also applies to --mark-donor-shapley-out / --mark-donor-epistasis-out, --mark-scale to"
              " --mark-sampled-shapley-out)")
_NEEDS = [      # (flags, the flags they apply to, the refusal where one of the former is given and none of the latter), in the order checked
    (("raw_saliency_target", "raw_saliency_times_input"), ("raw_saliency_dir",),
     "--raw-saliency-target / --raw-saliency-times-input need --raw-saliency-dir"),
    (("ig_steps", "ig_method", "ig_target"), ("ig_dir", "raw_ig_dir", "raw_donor_ig_dir"),
     "--ig-steps / --ig-method / --ig-target need --ig-dir or --raw-ig-dir (or --raw-donor-ig-dir)"),
    (("scan_scale", "scan_width", "scan_regions"), ("scan_out",), "--scan-scale / --scan-width / --scan-regions need --scan-out"),
    (("fine_scan_region", "fine_scan_width", "fine_scan_stride", "fine_scan_zoom", "fine_scan_scale"), ("fine_scan_out",),
     "--fine-scan-region / --fine-scan-width / --fine-scan-stride / --fine-scan-zoom / --fine-scan-scale need --fine-scan-out"),
    (("interaction_index",), ("pcre_interactions_out", "mark_interactions_out", "mark_donor_interactions_out", "contact_interactions_out") + _PAIRS_OUTS,
     "--interaction-index needs --pcre-interactions-out, --mark-interactions-out or --mark-donor-interactions-out"
     " (or --mark-sampled-interactions-out, --mark-donor-sampled-interactions-out)"),
    (("mark_focal",), _PAIRS_OUTS, "--mark-focal needs --mark-sampled-interactions-out or --mark-donor-sampled-interactions-out"),
    (("raw_donor_ig_dir",), ("donor_npy_dir",), "--raw-donor-ig-dir needs --donor-npy-dir"),
    (_DONOR_OUTS, ("donor_npy_dir",), "%s need --donor-npy-dir" % " / ".join("--" + name.replace("_", "-") for name in _DONOR_OUTS)),
    (_BACKSELECT_DONOR_OUTS, ("donor_npy_dir",), "--mark-donor-backselect-out needs --donor-npy-dir"),
    (_CONTACT_DONOR_OUTS, ("donor_npy_dir",), "--contact-donor-shapley-out needs --donor-npy-dir"),
    (("contact_players",), _CONTACT_OUTS + _CONTACT_DONOR_OUTS,
     "--contact-players needs --contact-shapley-out, --contact-interactions-out, --contact-dividends-out or --contact-donor-shapley-out"),
    (("contact_scale",), _CONTACT_OUTS,
     "--contact-scale needs --contact-shapley-out, --contact-interactions-out or --contact-dividends-out (the donor rule has no scale)"),
    (("contact_donor_marks",), _CONTACT_DONOR_OUTS, "--contact-donor-marks needs --contact-donor-shapley-out"),
    (("mark_backselect_players", "backselect_mode", "backselect_frac"), _BACKSELECT_OUTS,
     "--mark-backselect-players / --backselect-mode / --backselect-frac need --mark-backselect-out or --mark-donor-backselect-out"),
    (("donor_npy_dir", "donor_meta", "donor_store"), _DONOR_OUTS + _BACKSELECT_DONOR_OUTS + _CONTACT_DONOR_OUTS + ("raw_donor_ig_dir",),
     "--donor-npy-dir / --donor-meta / --donor-store need --mark-donor-shapley-out, --mark-donor-epistasis-out or "
     "--mark-donor-sampled-shapley-out (or --window-donor-shapley-out, --fine-window-donor-shapley-out, "
     "--mark-donor-interactions-out, --mark-donor-sampled-interactions-out, --mark-donor-dividends-out)"),
    (("mark_sampled_players", "mark_perms", "mark_seed"), _SAMPLED_OUTS + _PAIRS_OUTS,
     "--mark-sampled-players / --mark-perms / --mark-seed need --mark-sampled-shapley-out or --mark-donor-sampled-shapley-out"
     " (or --mark-sampled-interactions-out, --mark-donor-sampled-interactions-out)"),
    (("mark_scale",), _MARK_OUTS + ("mark_sampled_shapley_out", "mark_sampled_interactions_out", "mark_backselect_out"), _MARK_NEED),
    (("mark_players",), _MARK_OUTS + _DONOR_EXACT_OUTS, _MARK_NEED),
    (("window_players", "window_width", "window_perms", "window_seed"), _WINDOW_OUTS,
     "--window-players / --window-width / --window-perms / --window-seed need --window-shapley-out or --window-donor-shapley-out"),
    (("window_scale",), ("window_shapley_out",), "--window-scale needs --window-shapley-out (the donor rule has no scale)"),
    (("fine_window_region", "fine_window_width", "fine_window_players", "fine_window_zoom", "fine_window_perms", "fine_window_seed"), _FINE_WINDOW_OUTS,
     "--fine-window-region / --fine-window-width / --fine-window-players / --fine-window-zoom / --fine-window-perms / "
     "--fine-window-seed need --fine-window-shapley-out or --fine-window-donor-shapley-out"),
    (("fine_window_scale",), ("fine_window_shapley_out",), "--fine-window-scale needs --fine-window-shapley-out (the donor rule has no scale)"),
    (("transplant_bed",), ("transplant_out",), "--transplant-bed needs --transplant-out"),
    (("transplant_out",), ("transplant_bed",), "--transplant-out needs --transplant-bed"),
    (("transplant_freq", "transplant_slot"), ("transplant_out",), "--transplant-freq / --transplant-slot need --transplant-out"),
]


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)

    def given(name):      # (an option of _DEFAULTS: it was given; an output, a directory or a switch: it is set)
        return getattr(args, name) is not None if name in _DEFAULTS else bool(getattr(args, name))

    for flags, owners, message in _NEEDS:
        if any(given(name) for name in flags) and not any(given(name) for name in owners):
            ap.error(message)
    for name, default in _DEFAULTS.items():
        if getattr(args, name) is None:
            setattr(args, name, default)
    n_out = 1 if args.regression else 2
    if args.raw_saliency_target is not None and not 0 <= args.raw_saliency_target < n_out:
        ap.error("--raw-saliency-target must be in [0, %d)" % n_out)
    if args.ig_steps < (2 if args.ig_method == "riemann_trapezoid" else 1):
        ap.error("--ig-steps must be at least %d" % (2 if args.ig_method == "riemann_trapezoid" else 1))
    if args.ig_target is not None and not 0 <= args.ig_target < n_out:
        ap.error("--ig-target must be in [0, %d)" % n_out)
    for name in ("scan_scale", "fine_scan_scale", "mark_scale", "window_scale", "fine_window_scale"):
        if not (getattr(args, name) >= 0 and np.isfinite(getattr(args, name))):
            ap.error("--%s must be a finite factor >= 0" % name.replace("_", "-"))
    if not np.isfinite(args.backselect_frac):
        ap.error("--backselect-frac must be a finite number")
    if not np.isfinite(args.contact_scale):
        ap.error("--contact-scale must be a finite factor")
    if args.contact_interactions_out and args.contact_players == "all":
        ap.error("--contact-interactions-out needs at least 2 players; --contact-players all has 1")
    for name in ("scan_width", "fine_scan_width", "fine_scan_stride", "fine_scan_zoom", "mark_perms", "window_width", "window_perms",
                 "fine_window_width", "fine_window_zoom", "fine_window_perms"):
        if getattr(args, name) is not None and getattr(args, name) < 1:
            ap.error("--%s must be at least 1" % name.replace("_", "-"))
    for name in ("fine_scan_region", "fine_window_region"):
        region = getattr(args, name)
        if region != "promoter":
            if not region.isdigit() or int(region) >= 8:
                ap.error("--%s must be promoter or a pCRE slot in [0, 8)" % name.replace("_", "-"))
            setattr(args, name, int(region))
    try:
        args.transplant_freq = [float(s) for s in args.transplant_freq.split(",")]
        if not args.transplant_freq or not np.isfinite(args.transplant_freq).all():
            raise ValueError
    except ValueError:
        ap.error("--transplant-freq must be a comma-separated list of finite frequencies")
    if args.transplant_slot != "append":
        if not args.transplant_slot.isdigit() or int(args.transplant_slot) >= 8:
            ap.error("--transplant-slot must be append or a pCRE slot in [0, 8)")
        args.transplant_slot = int(args.transplant_slot)
    if args.transplant_bed:
        from .transplant import read_bed
        try:
            read_bed(args.transplant_bed)
        except (OSError, ValueError) as e:
            ap.error("--transplant-bed: %s" % e)
    if isinstance(args.mark_focal, str):
        if args.mark_focal.strip().lstrip("+-").isdigit():
            args.mark_focal = int(args.mark_focal)
            if args.mark_focal < 1:
                ap.error("--mark-focal must be at least 1 player (or a list of player names)")
        else:
            args.mark_focal = [s.strip() for s in args.mark_focal.split(",")]
    if any(given(name) for name in _PAIRS_OUTS):      # (the players' names: a bad count or name is a usage error)
        from .attribution import focal_players, mark_players_wide
        pair_names = mark_players_wide(args.mark_sampled_players, 7, 8)[2]      # (predict()'s n_feats and default i_max)
        try:
            if isinstance(args.mark_focal, int):
                if args.mark_focal > len(pair_names):
                    raise ValueError("K = %d exceeds the %d players" % (args.mark_focal, len(pair_names)))
            else:
                focal_players(args.mark_focal, pair_names, len(pair_names))
        except ValueError as e:
            ap.error("--mark-focal: %s" % e)
    if args.raw_donor_ig_dir and args.donor_store:
        ap.error("--raw-donor-ig-dir reads the donor's raw .npy signals; --donor-store does not serve it")
    try:      # (the window games' players at predict()'s default geometry: too many is a usage error)
        if any(given(name) for name in _WINDOW_OUTS):
            from .attribution import window_players
            window_players(args.window_players, 7, 8, 20, args.window_width)
        if any(given(name) for name in _FINE_WINDOW_OUTS):
            from .attribution import fine_window_players
            fine_window_players(args.fine_window_players, 7, args.fine_window_width, -(-20 // args.fine_window_width))
    except ValueError as e:
        ap.error(str(e))
    kw = {name: value for name, value in vars(args).items() if name not in ("meta", "npy_dir", "weights", "regression", "output", "store", "donor_store")}
    meta, pred = predict(args.meta, args.npy_dir, args.weights, args.regression, progress=True, store_path=args.store,
                         donor_store_path=args.donor_store, **kw)
    print("Predicting expressions for %d genes." % len(meta))
    meta["prediction"] = pred
    meta.to_csv(args.output, index=False)
    from sklearn import metrics
    if args.regression:
        from scipy.stats import pearsonr
        y = np.log2(meta["expression"] + 1)
        print("R2 : %s" % metrics.r2_score(y, meta["prediction"]))
        print("Pearson's r : %s" % pearsonr(y, meta["prediction"])[0])
    else:
        print("ROC-AUC : %s" % metrics.roc_auc_score(meta["label"], meta["prediction"]))
        print("Average Precision : %s" % metrics.average_precision_score(meta["label"], meta["prediction"]))
        print("Accuracy : %s" % metrics.accuracy_score(meta["label"], (meta["prediction"] > 0.5).astype(int)))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
