"""The writers of `chromoformer_amd.predict`: one function per kind of output file, all of one shape,

    write_x(run, <the output path(s)>, **<the options that apply>)

`run` (Run) is what one predict() call shares among them: the model, the device-resident store, bsz, the gene ids, `regression`, the
metadata, and the datasets and the donor store that several writers need, built on first use.  Every writer covers every gene of
the store, in store order.  With donor=True a writer plays against the donor cell type (run.donor_store / run.dataset(donor=True): the same genes
in the same order); without, an absent player's raw signal is scaled by `scale`.  predict.py's table says which writer serves which
output with which options."""
from __future__ import annotations

import os
from functools import cached_property

import numpy as np
import torch

from .data import ChromoformerDataset, GeneStore
from .engine import Slot


class Refusal(ValueError):
    """A refusal before anything is computed, in predict()'s words; `cli`: main()'s words for the same, where they differ."""

    def __init__(self, message, cli):
        super().__init__(message)
        self.cli = cli


class Run:
    """One predict() call as its writers see it.  geometry: dict(n_feats, i_max, binsizes, w_prom, w_max); predict() sets store and model
    once they exist.  The datasets are built at their first use; so is the donor store, which release_donor() drops."""

    def __init__(self, meta_path, npy_dir, meta, regression, bsz, geometry, progress=False, store_path=None, donor_npy_dir=None,
                 donor_meta=None, donor_store_path=None):
        self.meta_path, self.npy_dir, self.meta, self.regression, self.bsz, self.progress = meta_path, npy_dir, meta, regression, bsz, progress
        self.geometry, self.gene_ids = dict(geometry), meta.gene_id.tolist()
        self.store_path, self.donor_npy_dir, self.donor_meta, self.donor_store_path = store_path, donor_npy_dir, donor_meta, donor_store_path
        self.model = self.store = None
        self._datasets = {}

    def dataset(self, donor=False, raw=False):
        """The run's (the donor's) dataset, built at its first use.  Plain: regression=False -- strand, coordinates and geometry for the
        generators; raw: with the run's `regression` -- the raw-signal writers read its .npy files, and it fills the store where none is packed."""
        if (donor, raw) not in self._datasets:
            g, meta, npy_dir = self.geometry, (self.donor_meta or self.meta_path) if donor else self.meta_path, self.donor_npy_dir if donor else self.npy_dir
            self._datasets[donor, raw] = ChromoformerDataset(meta, npy_dir, self.gene_ids, g["n_feats"], g["i_max"], list(g["binsizes"]), g["w_prom"],
                                                             g["w_max"], regression=raw and self.regression)
        return self._datasets[donor, raw]

    def find_store(self, donor=False):
        """The device-resident store of the run's (the donor's) genes: from a packed store where one serves them, else binned on the GPU
        from the dataset (126 KB per gene).  Labels are not used for prediction."""
        from . import pack
        g = self.geometry
        dev = torch.device("cuda", torch.cuda.current_device())
        npy_dir, path, meta = (self.donor_npy_dir, self.donor_store_path, self.dataset(donor=True).meta) if donor else (self.npy_dir, self.store_path, self.meta)
        packed = pack.find(npy_dir, path, list(g["binsizes"]), g["i_max"], g["w_prom"], g["w_max"], g["n_feats"], self.gene_ids, meta=meta)
        if packed is not None:
            return packed.store(self.gene_ids, device=dev, regression=False)
        return GeneStore(self.dataset(donor, raw=not donor), progress=self.progress, device=dev, resident=True)

    @cached_property
    def donor_store(self):
        return self.find_store(donor=True)

    def release_donor(self):
        self.__dict__.pop("donor_store", None)

    def donor(self, wanted):
        """(the donor's dataset, the donor's store) for a writer under the donor rule, else (None, None)."""
        return (self.dataset(donor=True), self.donor_store) if wanted else (None, None)

    @property
    def target(self):      # the prediction's logit column
        return 0 if self.regression else 1


def _savez(path, **arrays):
    """np.savez to exactly `path` (through a file object: given a name without .npz, np.savez would append it)."""
    with open(path, "wb") as f:
        np.savez(f, **arrays)


def _slot_batches(who, run):
    """The genes of run.store in batches of at most run.bsz -> (lo, B, slot) per batch: genes lo .. lo + B - 1 gathered on the device
    (cf_gather_batch) into a Slot of B genes, one Slot per size.  The gather's error word is read when the caller comes back for the
    next batch, after its own work on this one: an error raises RuntimeError naming `who`, the writer."""
    import ctypes as C

    from . import _lib
    model, store, bsz = run.model, run.store, run.bsz
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


def _dict_batches(run, donor_store=None):
    """The genes of run.store in batches of at most run.bsz -> (lo, B, forward()'s six arguments from store.batch, the donor pair from
    donor_store.batch or None without a donor store, the donor's batch dict or None) per batch."""
    from .attribution import _BATCH_KEYS, _donor_pair
    for lo in range(0, len(run.store), run.bsz):
        idx = list(range(lo, min(lo + run.bsz, len(run.store))))
        d = run.store.batch(idx)
        dd = donor_store.batch(idx) if donor_store is not None else None
        yield lo, len(idx), tuple(d[k] for k in _BATCH_KEYS), None if dd is None else _donor_pair(dd), dd


def _same_genes(who, run, donor_store):
    if donor_store is not None and len(donor_store) != len(run.store):
        raise ValueError("%s: the donor store holds %d genes, the store %d" % (who, len(donor_store), len(run.store)))


def write_attention_maps(run, attention_dir=None, embeddings_out=None):
    """Attention maps (`attention_dir`/{embed,pairwise_interaction,regulation}_{binsize}.npy) and / or the regulatory embedding
    (`embeddings_out`, [n_genes, 3 * d_emb]).  Per batch: one device gather into a Slot and one model.attention_maps; the rows go
    straight into .npy memory maps (nothing is gathered in host memory)."""
    model = run.model
    which = (("embed", "pairwise_interaction", "regulation") if attention_dir else ()) + (("regulatory_embedding",) if embeddings_out else ())
    n = len(run.store)
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
    for lo, B, slot in _slot_batches("write_attention_maps", run):
        _, maps = model.attention_maps(slot, which=which)
        for (key, b), mm in outs.items():
            mm[lo:lo + B] = (maps[key] if b is None else maps[key][b]).cpu().numpy()
    for mm in outs.values():
        mm.flush()


def write_pcre_ablation(run, path):
    """In-silico pCRE deletion: `path`, a float32 .npy [n_genes, i_max + 2] holding the prediction column's quantity
    (sigmoid(logits)[:, 1], or logits[:, 0] for the regressor) with nothing deleted (column 0), pCRE slot j deleted (column 1 + j) and
    the promoter alone (last column).  Per batch: one device gather into a Slot and one model.pcre_ablation.  The logits (8 bytes per
    gene and column) are kept on the host; each column goes through the very sigmoid call predict() makes on the [n_genes, 2] logits,
    so column 0 is the prediction bit for bit."""
    model = run.model
    n, V = len(run.store), model.i_max + 2
    logits = torch.empty(n, V, model.n_out)
    for lo, B, slot in _slot_batches("write_pcre_ablation", run):
        logits[lo:lo + B] = model.pcre_ablation(slot).cpu()
    mm = np.lib.format.open_memmap(path, mode="w+", dtype=np.float32, shape=(n, V))
    for v in range(V):
        col = logits[:, v].contiguous()          # [n_genes, n_out], laid out as the logits predict() turns into its column
        mm[:, v] = col.numpy().reshape(-1) if run.regression else torch.sigmoid(col).numpy()[:, 1]
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


def write_exact_values(run, game, shapley_out=None, epistasis_out=None, interactions_out=None, players="marks", scale=0.0, index="sii"):
    """Exact Shapley values, pair epistasis and / or pairwise Shapley interaction indices of one game, in LOGIT space of the prediction's
    column (1 for the classifier, 0 for the regressor: the efficiency identity phi.sum(1) = logits - absent holds there, not after the
    sigmoid).  game (_EXACT_GAMES):

        "pcre"         the pCREs (P = i_max).  shapley_out: an .npz with phi [n, P], logits [n], promoter_only [n] and n_pcres [n] (the
                       slots that are no dummies)
        "mark"         the histone marks; players (attribution.mark_players) and scale apply.  shapley_out: an .npz with gene_ids [n],
                       players [P] (names), phi [n, P], logits [n] and erased [n]
        "mark_donor"   the marks against the donor store; players applies.  shapley_out: gene_ids, players, phi, logits, donor [n]
                       (every player's marks from the donor, under the gene's masks and frequencies) and donor_prediction [n] (the
                       plain forward of the donor's own batch)

    epistasis_out: a float32 .npy [n, P, P]; interactions_out: a float32 .npy [n, P, P], the index `index` ("sii" / "sti").  Per batch:
    one device gather into a Slot (the donor game: one store.batch per store), one model.<game>_shapley and / or one
    model.<game>_epistasis; with interactions_out one model.<game>_shapley_interactions, which serves shapley_out too (the 2^P forwards
    run once); the donor game's shapley_out adds one plain forward of the donor's batch."""
    from .attribution import _BATCH_KEYS, mark_players
    model, who, desc = run.model, "write_exact_values", _EXACT_GAMES[game]
    n, t, with_donor = len(run.store), run.target, "donor" in desc["kw"]
    if with_donor:
        _same_genes(who, run, run.donor_store)
    names = mark_players(players, model.n_feats, model.i_max)[2] if "players" in desc["kw"] else None
    P = model.i_max if names is None else len(names)
    phi, logits, absent = torch.empty(n, P), torch.empty(n), torch.empty(n)
    extra = torch.empty(n, dtype=torch.int32 if game == "pcre" else torch.float32)
    eps = np.lib.format.open_memmap(epistasis_out, mode="w+", dtype=np.float32, shape=(n, P, P)) if epistasis_out else None
    inter = np.lib.format.open_memmap(interactions_out, mode="w+", dtype=np.float32, shape=(n, P, P)) if interactions_out else None
    if with_donor:
        batches = _dict_batches(run, run.donor_store)
    else:      # (the Slot alone: the packed form of the methods' first argument)
        batches = ((lo, B, (slot,), None, None) for lo, B, slot in _slot_batches(who, run))
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
            cols = dict(gene_ids=np.array(run.gene_ids), players=np.array(names), **cols)
        _savez(shapley_out, **cols)
    for mm in (eps, inter):
        if mm is not None:
            mm.flush()


def write_dividends(run, path, game="mark", players="marks", scale=0.0):
    """Harsanyi dividends of an exact game, in LOGIT space of the prediction's column, into `path`, an .npz with gene_ids [n], players [P]
    (names), sets [2^P] (the set names by word, "" for the empty set), dividends [n, 2^P] float32 (word m at column m; they add up to
    the logit of every coalition) and mass [n, 2^P] (the scale of a dividend's rounding error, attribution.dividend_bound).  game:
    "pcre" (model.pcre_dividends), "mark" (model.mark_dividends; players and scale apply) or "mark_donor" (model.mark_donor_dividends
    against the donor store; players applies).  Per batch: one gather per store and one such call (its own 2^P forwards)."""
    n = len(run.store)
    if game not in _EXACT_GAMES:
        raise ValueError("write_dividends: unknown game %r; choose from %s" % (game, list(_EXACT_GAMES)))
    donor_store = run.donor_store if "donor" in _EXACT_GAMES[game]["kw"] else None
    if donor_store is not None and len(donor_store) != n:
        raise ValueError("write_dividends: the donor store must hold the store's %d genes" % n)
    div, mass, names, sets = None, None, None, None
    for lo, B, args, feats, _ in _dict_batches(run, donor_store):
        x, info = getattr(run.model, game + "_dividends")(*args, **_game_kw(game, players, scale, feats))
        if div is None:
            div, mass = np.empty((n, x.shape[1]), np.float32), np.empty((n, x.shape[1]), np.float32)
            names, sets = info["names"], info["sets"]
        div[lo:lo + B] = x[..., run.target].cpu().numpy()
        mass[lo:lo + B] = info["mass"][..., run.target].cpu().numpy()
    _savez(path, gene_ids=np.array(run.gene_ids), players=np.array(names), sets=np.array(sets), dividends=div, mass=mass)


def write_mark_sampled_values(run, path, donor=False, players="cells", n_perm=64, seed=0, scale=0.0):
    """Permutation-sampled Shapley values of up to 128 histone-mark players (model.mark_shapley_sampled), in LOGIT space of the
    prediction's column, into `path`, an .npz with gene_ids [n], players [P] (names), permutations uint8 [n_perm, P] (the orders, the
    same for every gene), phi [n, P], stderr [n, P] (the standard error of phi over the orders: the sampling error is reported, not
    bounded), logits [n] and absent [n] (every player absent; phi sums to their difference).  Per batch: one gather per store and one
    model.mark_shapley_sampled."""
    from .attribution import mark_players_wide, shapley_permutations
    model, n, t, donor_store = run.model, len(run.store), run.target, run.donor(donor)[1]
    _same_genes("write_mark_sampled_values", run, donor_store)
    names = mark_players_wide(players, model.n_feats, model.i_max)[2]
    P = len(names)
    perms = shapley_permutations(P, n_perm, seed)
    phi, se, logits, absent = torch.empty(n, P), torch.empty(n, P), torch.empty(n), torch.empty(n)
    for lo, B, args, feats, _ in _dict_batches(run, donor_store):
        p, info = model.mark_shapley_sampled(*args, players=players, permutations=perms, scale=scale, donor=feats)
        phi[lo:lo + B] = p[..., t].cpu()
        se[lo:lo + B] = info["stderr"][..., t].cpu()
        logits[lo:lo + B] = info["logits"][:, t].cpu()
        absent[lo:lo + B] = info["absent"][:, t].cpu()
    _savez(path, gene_ids=np.array(run.gene_ids), players=np.array(names), permutations=perms, phi=phi.numpy(), stderr=se.numpy(),
           logits=logits.numpy(), absent=absent.numpy())


def write_mark_backselect(run, path, donor=False, players="cells", mode="backward", frac=0.9, scale=0.0):
    """Greedy player selection among up to 128 histone-mark players (backselect.mark_backselect), on the prediction's logit column, into
    `path`, an .npz with gene_ids [n], players [P] (names), mode, frac, order int32 [n, P] (the player of each move), curve [n, P + 1]
    (the logit after t moves), size [n] and subset bool [n, P] (the smallest sufficient set on the path), threshold [n], direction [n],
    logits [n] and absent [n].  Per batch: one gather per store and one backselect.mark_backselect."""
    from .attribution import mark_players_wide
    from .backselect import mark_backselect
    model, n, t, donor_store = run.model, len(run.store), run.target, run.donor(donor)[1]
    _same_genes("write_mark_backselect", run, donor_store)
    names = mark_players_wide(players, model.n_feats, model.i_max)[2]
    P = len(names)
    order, curve, size, subset = torch.empty(n, P, dtype=torch.int32), torch.empty(n, P + 1), torch.empty(n, dtype=torch.int32), torch.empty(n, P, dtype=torch.bool)
    thr, sign, logits, absent = torch.empty(n), torch.empty(n, dtype=torch.int32), torch.empty(n), torch.empty(n)
    for lo, B, args, feats, _ in _dict_batches(run, donor_store):
        o, info = mark_backselect(model, *args, players=players, mode=mode, frac=frac, target=t, scale=scale, donor=feats)
        order[lo:lo + B] = o.cpu()
        curve[lo:lo + B] = info["values"][..., t].cpu()
        size[lo:lo + B] = info["size"].cpu()
        subset[lo:lo + B] = info["subset"].cpu()
        thr[lo:lo + B] = info["threshold"].cpu()
        sign[lo:lo + B] = info["direction"].cpu()
        logits[lo:lo + B] = info["logits"][:, t].cpu()
        absent[lo:lo + B] = info["absent"][:, t].cpu()
    _savez(path, gene_ids=np.array(run.gene_ids), players=np.array(names), mode=np.array(mode), frac=np.float32(frac), order=order.numpy(),
           curve=curve.numpy(), size=size.numpy(), subset=subset.numpy(), threshold=thr.numpy(), direction=sign.numpy(), logits=logits.numpy(),
           absent=absent.numpy())


def focal_argument(focal, players, n_feats, i_max):
    """focal, an int (each gene's strongest players by |phi|) or a list of player names or indices (those for every gene) -> the
    keyword argument of mark_shapley_interactions_sampled, dict(top=...) or dict(focal=...); ValueError where the players do not allow it."""
    from .attribution import focal_players, mark_players_wide
    names = mark_players_wide(players, n_feats, i_max)[2]
    if isinstance(focal, (int, np.integer)) and not isinstance(focal, bool):
        if not 1 <= focal <= len(names):
            raise Refusal("predict: mark_focal = %d outside 1..%d" % (focal, len(names)), "K = %d exceeds the %d players" % (focal, len(names)))
        return dict(top=int(focal))
    return dict(focal=focal_players(focal, names, len(names)))


def write_mark_sampled_interactions(run, path, donor=False, players="cells", focal=4, index="sii", n_perm=64, seed=0, scale=0.0):
    """Sampled pairwise Shapley interaction indices of each gene's focal mark players (attribution.mark_shapley_interactions_sampled:
    `focal` as focal_argument reads it), in LOGIT space of the prediction's column, into `path`, an .npz with gene_ids [n], players [P]
    (names), index, permutations uint8 [n_perm, P], focal int32 [n, n_focal] (the focal players of each gene), interactions
    [n, n_focal, P] (row f: focal player f with every player; not symmetric between focal players), stderr [n, n_focal, P] (the standard
    error over the orders: the sampling error is reported, not bounded), phi and phi_stderr [n, P] (the sampled Shapley values from the
    same forwards), logits [n] and absent [n]."""
    from .attribution import mark_shapley_interactions_sampled
    t, (donor_ds, donor_store) = run.target, run.donor(donor)
    res = list(mark_shapley_interactions_sampled(run.model, run.dataset(), donor_ds, genes=list(run.gene_ids), players=players, index=index,
                                                 n_perm=n_perm, seed=seed, scale=scale, bsz=run.bsz, store=run.store, donor_store=donor_store,
                                                 **focal_argument(focal, players, run.model.n_feats, run.model.i_max)))
    _savez(path, gene_ids=np.array(run.gene_ids), players=np.array(res[0]["players"]), index=np.array(index), permutations=res[0]["permutations"],
           focal=np.stack([r["focal"] for r in res]), interactions=np.stack([r["interactions"][..., t] for r in res]),
           stderr=np.stack([r["stderr"][..., t] for r in res]), phi=np.stack([r["phi"][..., t] for r in res]),
           phi_stderr=np.stack([r["phi_stderr"][..., t] for r in res]), logits=np.array([r["logits"][t] for r in res], dtype=np.float32),
           absent=np.array([r["absent"][t] for r in res], dtype=np.float32))


def write_mark_window_values(run, path, donor=False, players="promoter", width=1, n_perm=64, seed=0, scale=0.0):
    """Shapley values of window players (model.mark_window_shapley_dataset: exact with at most 16 players, else sampled), in LOGIT space
    of the prediction's column, into `path`, an .npz with gene_ids [n], players [P] (names), estimator ("exact" or "sampled": which one
    ran), phi [n, P], stderr [n, P] (zeros from the exact call), logits [n], absent [n] (every player absent; phi sums to their
    difference), null bool [n, P] (the player's window holds no real bin of the gene: phi = 0), chroms [n, P] and windows int64
    [n, P, 2] (the genomic start and end of the player's window in its region; "" and -1 where null) and, sampled, permutations uint8
    [n_perm, P].  Strand and coordinates come from the datasets."""
    n, t, (donor_ds, donor_store) = len(run.gene_ids), run.target, run.donor(donor)
    rows = list(run.model.mark_window_shapley_dataset(run.dataset(), donor_ds, genes=list(run.gene_ids), players=players, width=width, n_perm=n_perm,
                                                      seed=seed, scale=scale, bsz=run.bsz, store=run.store, donor_store=donor_store))
    P = len(rows[0]["players"])
    chroms, windows = np.full((n, P), "", dtype=object), np.full((n, P, 2), -1, dtype=np.int64)
    for i, r in enumerate(rows):
        for p, real in enumerate(r["windows"]):
            if real:      # (the named specs give every player one region)
                chroms[i, p], windows[i, p] = real[0][1], real[0][2:]
    out = dict(gene_ids=np.array(run.gene_ids), players=np.array(rows[0]["players"]), estimator=np.array(rows[0]["estimator"]),
               phi=np.stack([r["phi"][:, t] for r in rows]), stderr=np.stack([r["stderr"][:, t] for r in rows]),
               logits=np.array([r["logits"][t] for r in rows], dtype=np.float32), absent=np.array([r["absent"][t] for r in rows], dtype=np.float32),
               null=np.stack([r["null"] for r in rows]), chroms=chroms.astype(str), windows=windows)
    if "permutations" in rows[0]:
        out["permutations"] = rows[0]["permutations"]
    _savez(path, **out)


def write_mark_fine_window_values(run, path, donor=False, region="promoter", width=2, players="windows", zoom=1, n_perm=64, seed=0, scale=0.0):
    """Shapley values of FINE window players (model.mark_fine_window_shapley_dataset: the coarse window game first, then the fine game
    inside each gene's `zoom` most important coarse windows), in LOGIT space of the prediction's column, into `path`, an .npz with
    gene_ids [n], players [P] (the fine game's names, windows relative to the zoomed coarse window), exact (whether the fine game was
    exact), zoom int64 [n, k] (the chosen coarse windows, most important first; -1 where the gene has fewer), coarse_phi [n, n_cwin] (the
    coarse game's values; NaN past the region's real coarse windows), phi and stderr [n, k, P] (stderr zeros when exact), logits [n],
    absent [n, k] (every fine player absent; phi[:, r] sums to logits - absent[:, r]; NaN where zoom is -1), null bool [n, k, P] (the
    player has no real window in the gene: phi = 0), chroms [n] (the region's chromosome; "" without the region) and windows int64
    [n, k, P, 2] (genomic start and end; -1 where null).  Strand, coordinates and lengths come from the datasets."""
    from .attribution import fine_window_players
    model, n, t, (donor_ds, donor_store) = run.model, len(run.gene_ids), run.target, run.donor(donor)
    rows = list(model.mark_fine_window_shapley_dataset(run.dataset(), donor_ds, genes=list(run.gene_ids), region=region, zoom=zoom, width=width,
                                                       players=players, n_perm=n_perm, seed=seed, scale=scale, bsz=run.bsz, store=run.store,
                                                       donor_store=donor_store))
    rf, rc = int(np.argmin(model.binsizes)), int(np.argmin(model.n_bins))
    names = fine_window_players(players, model.n_feats, width, -(-(model.n_bins[rf] // model.n_bins[rc]) // width))[3]
    P, k, Pc = len(names), int(zoom), model.n_bins[rc]
    out = dict(gene_ids=np.array(run.gene_ids), players=np.array(names), exact=np.array(bool(rows[0]["exact"])),
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


def write_contact_values(run, shapley_out=None, interactions_out=None, dividends_out=None, donor=False, players="contacts", scale=0.0,
                         marks="own", index="sii"):
    """Exact Shapley values of contact players (contact.contact_shapley_dataset: an absent player deletes its pCRE slots and / or edits
    their promoter contact frequencies), in LOGIT space of the prediction's column, into `shapley_out`, an .npz with gene_ids [n],
    players [P] (names), phi [n, P], logits [n] (every player present), erased [n] (every player absent) or, with donor, donor [n], freq
    [n, i_max] (the genes' contact frequencies) and n_pcres [n]; with donor (the donor rule: an absent contact takes the donor cell
    type's frequency) also donor_freq [n, i_max] and marks ("own" / "donor": whose features the game was played on).  interactions_out:
    a float32 .npy [n, P, P], the pairwise index `index` (the batch's one call then serves phi too); dividends_out: an .npz with
    gene_ids, players, sets [2^P], dividends and mass [n, 2^P], from the table of the same call.  Without donor `scale` applies."""
    from .attribution import set_names
    from .contact import contact_shapley_dataset
    t, (donor_ds, donor_store) = run.target, run.donor(donor)
    rows = list(contact_shapley_dataset(run.model, run.dataset(), donor_ds, genes=list(run.gene_ids), players=players, scale=scale, marks=marks,
                                        interactions=index if interactions_out else None, dividends=bool(dividends_out), bsz=run.bsz,
                                        store=run.store, donor_store=donor_store))
    names, absent = rows[0]["players"], "donor" if donor else "erased"
    ids = np.array(run.gene_ids)
    if shapley_out:
        out = dict(gene_ids=ids, players=np.array(names), phi=np.stack([r["phi"][:, t] for r in rows]),
                   logits=np.array([r["logits"][t] for r in rows], dtype=np.float32), freq=np.stack([r["freq"] for r in rows]),
                   n_pcres=np.array([len(r["pcres"]) for r in rows], dtype=np.int32))
        out[absent] = np.array([r[absent][t] for r in rows], dtype=np.float32)
        if donor:
            out["donor_freq"], out["marks"] = np.stack([r["donor_freq"] for r in rows]), np.array(marks)
        _savez(shapley_out, **out)
    if interactions_out:
        np.save(interactions_out, np.stack([r["interactions"][..., t] for r in rows]).astype(np.float32))
    if dividends_out:
        sets = set_names(np.arange(1 << len(names), dtype=np.uint32), names)
        _savez(dividends_out, gene_ids=ids, players=np.array(names), sets=np.array(sets), dividends=np.stack([r["dividends"][..., t] for r in rows]),
               mass=np.stack([r["mass"][..., t] for r in rows]))


def transplant_freqs(freqs):
    """The contact frequencies of the transplant screen, a number or a sequence -> a list of floats."""
    return [float(f) for f in np.atleast_1d(np.asarray(freqs, dtype=np.float64))]


def write_transplant(run, out, bed, freqs=(1.0, 5.0, 10.0), slot="append"):
    """pCRE transplant screen (transplant.pcre_transplant_dataset) into `out`, an .npz: gene_ids [n], prediction [n], transplant
    [n, C, Q] -- the prediction with candidate c of the BED file `bed` (`chrom start end [name]` lines; the raw chrom:start-end.npy
    files are in the dataset's directory, binned by the dataset's own code) in the gene's slot at contact frequency freqs[q], in the
    prediction column's quantity --, slot [n] (-1 = not placed), placed [n], candidates [C] (names), freqs [Q]."""
    from .transplant import library_from_regions, pcre_transplant_dataset, read_bed
    freqs = transplant_freqs(freqs)
    library = library_from_regions(run.dataset(), read_bed(bed))
    rows = list(pcre_transplant_dataset(run.model, run.dataset(), library, freqs, slot=slot, genes=list(run.gene_ids), bsz=run.bsz, store=run.store))

    def quantity(lg):
        lg = np.asarray(lg, dtype=np.float32)
        return lg[..., 0] if run.regression else torch.sigmoid(torch.from_numpy(lg)).numpy()[..., 1]

    _savez(out, gene_ids=np.array(run.gene_ids), prediction=quantity(np.stack([r["logits"] for r in rows])),
           transplant=quantity(np.stack([r["transplant"] for r in rows])), slot=np.array([r["slot"] for r in rows], dtype=np.int32),
           placed=np.array([r["placed"] for r in rows], dtype=bool), candidates=np.array(library.names),
           freqs=np.array(freqs, dtype=np.float32))


def write_integrated_gradients(run, ig_dir, n_steps=50, method="gausslegendre", target=None):
    """Integrated gradients into `ig_dir`: promoter_feats_{b}.npy [n, L, F], pcre_feats_{b}.npy [n, i_max, L, F], interaction_freq.npy
    [n, T, T] and delta.npy [n] (float32 .npy memory maps; nothing is gathered in host memory).  Zero baseline, every float input
    interpolated.  Per batch: one device gather into a Slot and one model.integrated_gradients."""
    model = run.model
    n, S, T, F = len(run.store), model.i_max, model.i_max + 1, model.n_feats
    os.makedirs(ig_dir, exist_ok=True)

    def mm(name, shape):
        return np.lib.format.open_memmap(os.path.join(ig_dir, name + ".npy"), mode="w+", dtype=np.float32, shape=(n,) + shape)

    outs = {}
    for b, nb in zip(model.binsizes, model.n_bins):
        outs["promoter_feats", b] = mm("promoter_feats_%d" % b, (nb, F))
        outs["pcre_feats", b] = mm("pcre_feats_%d" % b, (S, nb, F))
    outs["interaction_freq", None] = mm("interaction_freq", (T, T))
    outs["delta", None] = mm("delta", ())
    for lo, B, slot in _slot_batches("write_integrated_gradients", run):
        attr, info = model.integrated_gradients(slot, target=target, n_steps=n_steps, method=method)
        attr["delta"] = info["delta"]
        for (key, b), m in outs.items():
            m[lo:lo + B] = (attr[key] if b is None else attr[key][b]).cpu().numpy()
    for m in outs.values():
        m.flush()


def write_perturbation_scan(run, path, scale=0.0, width=1, regions="promoter", mark_sets=None):
    """In-silico perturbation scan (model.perturbation_scan: the marks of a mark set scaled by `scale` in raw-signal space over each
    window of `width` coarsest bins) into `path`, an .npz holding

        gene_ids     [n]
        mark_sets    [n_sets, n_feats] bool: the marks of each set (default: each mark alone, then all together)
        prediction   float32 [n]: the prediction column's quantity (sigmoid(logits)[:, 1], or logits[:, 0] for the regressor) of the
                     unperturbed gene, through the very sigmoid call predict() makes: the CSV column bit for bit
        promoter     float32 [n, n_sets, W], W = the coarsest resolution's bins: the same quantity with set k scaled over window g of
                     the promoter (genomic order: the metadata's strands undo the mirror of '-' strand promoters); NaN where the window
                     holds no real bin
        pcres        float32 [n, i_max, n_sets, W], with regions="all": the same per pCRE slot (NaN for dummy slots)

    Per batch: one device gather into a Slot and one model.perturbation_scan_regions over the scanned regions."""
    from .attribution import scan_mark_sets, scan_regions_expand, scan_row
    model, store = run.model, run.store
    n, S, F = len(store), model.i_max, model.n_feats
    mark_sets = scan_mark_sets(mark_sets, F)
    K = len(mark_sets)
    rc = int(np.argmin(model.n_bins))
    W = model.n_bins[rc]
    V = 1 + K * W
    scanned = scan_regions_expand("all" if regions == "all" else "promoter", S, "write_perturbation_scan")
    logits = torch.empty(len(scanned), n, V, model.n_out)
    live = torch.zeros(len(scanned), n, W, dtype=torch.bool)      # window g of the region holds a real bin
    flip = torch.tensor([s != "+" for s in run.meta.strand.tolist()], dtype=torch.uint8, device=model._device)
    for lo, B, slot in _slot_batches("write_perturbation_scan", run):
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
        return lg.numpy().reshape(-1) if run.regression else torch.sigmoid(lg).numpy()[:, 1]

    vals = np.empty((len(scanned), n, V), dtype=np.float32)
    for k in range(len(scanned)):
        for v in range(V):
            vals[k, :, v] = column(logits[k, :, v])
    scan = vals[:, :, scan_row(0, 0, 0, K, W):].reshape(len(scanned), n, K, W)
    scan[~np.broadcast_to(live.numpy()[:, :, None, :], scan.shape)] = np.nan
    sets = np.zeros((K, F), dtype=bool)
    for k, ms in enumerate(mark_sets):
        sets[k, list(ms)] = True
    arrays = dict(gene_ids=np.array(run.gene_ids), mark_sets=sets, prediction=vals[0, :, scan_row(0, None, None, K, W)].copy(), promoter=scan[0])
    if regions == "all":
        arrays["pcres"] = np.ascontiguousarray(scan[1:].transpose(1, 0, 2, 3))
    _savez(path, **arrays)


def write_perturbation_scan_fine(run, path, region="promoter", width=1, stride=None, zoom=None, scale=0.0, mark_sets=None):
    """Fine-resolution perturbation scan (attribution.perturbation_scan_fine: windows of `width` finest bins, `stride` apart, of the
    promoter or of one pCRE slot; strand, coordinates and region lengths come from the metadata) into `path`, an .npz holding

        gene_ids     [n]
        mark_sets    [n_sets, n_feats] bool: the marks of each set (default: each mark alone, then all together)
        prediction   float32 [n]: the prediction column's quantity (sigmoid(logits)[:, 1], or logits[:, 0] for the regressor)
        chroms       [n] and windows int64 [n, n_win, 2]: genomic start and end of each window (-1 where the gene has fewer windows)
        scan         float32 [n, n_sets, n_win]: the same quantity with set k scaled by `scale` over window g; NaN where windows is -1
        zoom         int64 [n, k], coarse_windows int64 [n, W, 2] and coarse float32 [n, n_sets, W], with zoom = k: the k coarse windows
                     that were fine-scanned, most important first, and the coarse scan they were chosen from (-1 / NaN padding)"""
    from .attribution import perturbation_scan_fine
    col = (lambda lg: lg[..., 0]) if run.regression else (lambda lg: torch.sigmoid(torch.from_numpy(np.ascontiguousarray(lg))).numpy()[..., 1])
    res = list(perturbation_scan_fine(run.model, run.dataset(), genes=list(run.gene_ids), region=region, zoom=zoom, scale=scale, width=width,
                                      stride=stride, mark_sets=mark_sets, bsz=run.bsz, store=run.store))
    n, K, F = len(res), len(res[0]["mark_sets"]) if res else 0, run.model.n_feats
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
    arrays = dict(gene_ids=np.array(run.gene_ids), mark_sets=sets, prediction=np.array([col(d["logits"]) for d in res], dtype=np.float32),
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
    ds = dataset
    for gene in (ds.target_genes if genes is None else genes):
        g = ds.genes[gene]
        chrom, tss, _ = g["tss"]
        for region in [(chrom, tss - 20000, tss + 20000)] + list(g["pcres"]):
            path = "%s/%s:%d-%d.npy" % ((ds.npy_dir,) + tuple(region))
            if not os.path.exists(path):
                raise FileNotFoundError("raw-signal saliency: %s is missing (gene %s); raw signals are required -- a packed store holds the "
                                        "binned features only, keep the .npy files next to it" % (path, gene))


def _raw_arrays(d, keys):
    """One gene's .npz members of the raw-signal writers: `keys` of the generator's row d in that order -- `regions` as strings
    "chrom:start-end", the promoter window first: sample s of a track is position start + s --, then `pcre_<s>` per pCRE."""
    arrays = {k: np.array(["%s:%d-%d" % tuple(r) for r in d[k]]) if k == "regions" else d[k] for k in keys}
    for s, t in enumerate(d["pcres"]):
        arrays["pcre_%d" % s] = t
    return arrays


def write_raw_saliency(run, saliency_dir, target=None, times_input=False):
    """Raw-signal saliency (model.raw_signal_gradients) into `saliency_dir`/<gene_id>.npz: `promoter` float32 [F, window] and `pcre_<s>`
    float32 [F, len_s] in genomic orientation, `regions` and `logits` (_raw_arrays)."""
    os.makedirs(saliency_dir, exist_ok=True)
    require_raw_signals(run.dataset(raw=True))
    for d in run.model.raw_signal_gradients(run.dataset(raw=True), target=target, times_input=times_input, bsz=run.bsz):
        np.savez(os.path.join(saliency_dir, "%s.npz" % d["gene_id"]), **_raw_arrays(d, ("promoter", "logits", "regions")))


def write_raw_integrated_gradients(run, ig_dir, donor=False, n_steps=50, method="gausslegendre", target=None):
    """Integrated gradients in raw-signal space (model.raw_integrated_gradients: zero-signal baseline, path a * x) into
    `ig_dir`/<gene_id>.npz: the keys of write_raw_saliency (the tracks hold the per-sample attributions) plus `baseline_logits` [n_out]
    and `delta` (the tracks' sum minus logits - baseline_logits at the target: the quadrature error).  With donor the baseline is the
    donor cell type's signal over the same regions (path xd + a (x - xd)) and every file also holds `donor_prediction` [n_out], the
    donor dataset's own forward of the gene."""
    os.makedirs(ig_dir, exist_ok=True)
    require_raw_signals(run.dataset(raw=True))
    donor_dataset = run.dataset(donor=True, raw=True) if donor else None
    if donor:
        require_raw_signals(donor_dataset)
    keys = ("promoter", "logits", "baseline_logits", "delta", "regions") + (("donor_prediction",) if donor else ())
    for d in run.model.raw_integrated_gradients(run.dataset(raw=True), target=target, n_steps=n_steps, method=method, bsz=run.bsz, donor_dataset=donor_dataset):
        np.savez(os.path.join(ig_dir, "%s.npz" % d["gene_id"]), **_raw_arrays(d, keys))
