"""Unstructured inputs: everything the public surface accepts that neither orc.synthetic_batch nor the dataset ever produces.

The dataset's batches are structured: one leading unmasked block as interaction mask (symmetric, the same at every resolution),
frequencies in row 0 only, centred contiguous pad ranges, features zeroed under the masks.  unstructured_batch() keeps the shapes and
the labels of orc.synthetic_batch(regime="realistic") and replaces the rest:

  interaction_freq    dense signed normal(0, 1.5) in all T x T entries
  interaction_masks   random bits (about 40 % masked), drawn per resolution, not symmetric, the resolutions pairwise different;
                      planted in the last three genes: a fully masked row ROW > 0 whose column stays visible from row 0 (gene B - 3),
                      row 0 fully masked (gene B - 2), everything masked (gene B - 1); every other gene keeps [0, 0] unmasked
  pad masks           5-d reference layout.  Centre rows of the pCRE slots cycle, slot (g * S + s) % 6, through PCRE_PATTERNS: random
                      holes, only bin 0 valid, only bin L - 1 valid, only the centre bin valid, the centre bin masked and the rest valid,
                      fully masked.  Promoters cycle g % 5 through PROMOTER_PATTERNS: fully masked, holes, a single valid bin (L - 1),
                      the centre bin masked, all valid.  Non-centre rows: independent random bits (rows="random", their own RNG stream
                      `rows_seed`) or the centre row repeated (rows="repeat").  In the promoter masks about half of the columns masked in
                      the centre row are masked in EVERY row, so that a model that reads all rows (embed.n_layers > 1) still has bins
                      nothing can look at
  features            drawn everywhere: non-zero under the masks and in fully masked slots

Every component has an RNG stream of its own, so two calls that differ in one argument differ in that component only.
with_garbage() writes large values where the reference cannot look, centre_rows() gives the compact [.., L] mask form."""
import numpy as np
import torch

from oracle import chromoformer_oracle as orc

PCRE_PATTERNS = ("holes", "first", "last", "centre_only", "centre_masked", "none_valid")
PROMOTER_PATTERNS = ("none_valid", "holes", "last", "centre_masked", "all_valid")
ROW = 2                      # the planted fully masked Regulation row of gene B - 3
GARBAGE_FEAT, GARBAGE_FREQ = 37.0, 1e3
SEED = 1                     # chosen so that the fp64 oracle's logits move by >= 1e-3 under every corruption of CORRUPTIONS (B = 6, default configuration)


def planted_genes(B):
    """-> (gene with row ROW fully masked, gene with row 0 fully masked, gene with everything masked)."""
    return B - 3, B - 2, B - 1


def pcre_pattern(g, s, S):
    return PCRE_PATTERNS[(g * S + s) % len(PCRE_PATTERNS)]


def promoter_pattern(g):
    return PROMOTER_PATTERNS[g % len(PROMOTER_PATTERNS)]


def _centre_row(kind, L, rng):
    """One centre query row of a pad mask (True = masked)."""
    row = np.ones(L, dtype=bool)
    if kind == "holes":
        while True:
            row = rng.random(L) < 0.5
            inner = np.flatnonzero(~row)
            if len(inner) >= 2 and row[inner[0]:inner[-1]].any():      # at least two valid bins with a masked one between them
                return row
    if kind == "first":
        row[0] = False
    elif kind == "last":
        row[L - 1] = False
    elif kind == "centre_only":
        row[L // 2] = False
    elif kind == "centre_masked":
        row[:] = False
        row[L // 2] = True
    elif kind == "all_valid":
        row[:] = False
    else:
        assert kind == "none_valid", kind
    return row


def _full(centre, rows, rng, dead_columns):
    """centre [N, L] -> [N, L, L]: the centre row at L // 2, the other rows random or the centre row repeated."""
    N, L = centre.shape
    if rows == "repeat":
        return np.repeat(centre[:, None, :], L, axis=1)
    assert rows == "random", rows
    full = rng.integers(0, 2, size=(N, L, L), dtype=np.uint8).astype(bool)
    if dead_columns:
        dead = centre & (rng.random((N, L)) < 0.5)
        dead[:, L // 2] = False
        full |= dead[:, None, :]
    full[:, L // 2] = centre
    return full


def unstructured_batch(B, cfg=None, seed=SEED, regression=False, rows="random", rows_seed=0):
    c = orc._cfg(cfg)
    S, T, F_ = c["i_max"], c["i_max"] + 1, c["n_feats"]
    assert B >= 4 and T > ROW + 1
    batch = orc.synthetic_batch(B, cfg=c, seed=seed, regime="realistic", regression=regression)      # shapes and labels
    stream = lambda *tag: np.random.default_rng([seed, *tag])      # noqa: E731
    g_row, g_row0, g_all = planted_genes(B)

    batch["interaction_freq"] = torch.from_numpy(stream(1).normal(0.0, 1.5, size=(B, T, T)).astype(np.float32))

    rng = stream(2)
    nres = len(c["binsizes"])
    im = np.zeros((nres, B, T, T), dtype=bool)
    for g in range(B):
        while True:
            m = rng.random((nres, T, T)) < 0.4
            if g == g_all:
                m[:] = True
                break
            if g == g_row:
                m[:, ROW, :] = True
                m[:, 0, ROW] = False
            if g == g_row0:
                m[:, 0, :] = True
            else:
                m[:, 0, 0] = False
            if all((m[r] != m[r].T).any() for r in range(nres)) and all((m[r] != m[q]).any() for r in range(nres) for q in range(r)):
                break
        im[:, g] = m
    for r, b in enumerate(c["binsizes"]):
        batch["interaction_masks"][b] = torch.from_numpy(im[r].reshape(B, 1, T, T).copy())

    for r, b in enumerate(c["binsizes"]):
        L = c["w_max"] // b
        rng = stream(3, r)
        batch["promoter_feats"][b] = torch.from_numpy(np.log1p(rng.gamma(0.6, 1.0, size=(B, 1, L, F_))).astype(np.float32))
        batch["pcre_feats"][b] = torch.from_numpy(np.log1p(rng.gamma(0.6, 1.0, size=(B, S, L, F_))).astype(np.float32))
        rng = stream(4, r)
        pc = np.stack([_centre_row(promoter_pattern(g), L, rng) for g in range(B)])
        cc = np.stack([_centre_row(pcre_pattern(g, s, S), L, rng) for g in range(B) for s in range(S)])
        rng = stream(5, r, rows_seed)
        batch["promoter_pad_masks"][b] = torch.from_numpy(_full(pc, rows, rng, True).reshape(B, 1, 1, L, L))
        batch["pcre_pad_masks"][b] = torch.from_numpy(_full(cc, rows, rng, False).reshape(B, S, 1, L, L))
    return batch


def copy_batch(batch):
    return {k: ({b: t.clone() for b, t in v.items()} if isinstance(v, dict) else v.clone()) for k, v in batch.items()}


def centre_rows(batch):
    """The same batch with compact pad masks: promoter [B, 1, L], pCRE [B, S, L] (the centre query rows)."""
    out = dict(batch)
    for key in ("promoter_pad_masks", "pcre_pad_masks"):
        out[key] = {b: m[:, :, 0, m.shape[-1] // 2, :].contiguous() for b, m in batch[key].items()}
    return out


def masked_everywhere(batch):
    """[B, T, T] bool: interaction entries masked at every resolution."""
    return torch.stack([m[:, 0] for m in batch["interaction_masks"].values()]).all(0)


def dead_bins(batch, all_promoter_rows=False):
    """Bins whose features the reference cannot look at -> ({b: [B, 1, L]}, {b: [B, S, L]}) bool.

    pCRE bins are keys and values of the centre query only: dead where the centre row masks them and has a valid bin (a fully masked
    row is a uniform softmax over ALL its keys).  A promoter bin is also the query and the residual of its own row, so the centre bin
    is never dead; with one Embedding layer the other bins are keys of the centre row alone.  all_promoter_rows = True (embed.n_layers
    > 1: every row is read, and every row's output is a key of the next layer): dead only if EVERY row masks the column and no row
    of that promoter is fully masked."""
    pd, cd = {}, {}
    for b, m in batch["pcre_pad_masks"].items():
        c = m[:, :, 0, m.shape[-1] // 2, :]
        cd[b] = c & ~c.all(-1, keepdim=True)
    for b, m in batch["promoter_pad_masks"].items():
        L = m.shape[-1]
        if all_promoter_rows:
            d = m[:, :, 0].all(-2) & ~m[:, :, 0].all(-1).any(-1, keepdim=True)
        else:
            c = m[:, :, 0, L // 2, :]
            d = c & ~c.all(-1, keepdim=True)
        d = d.clone()
        d[..., L // 2] = False
        pd[b] = d
    return pd, cd


def with_garbage(batch, all_promoter_rows=False):
    """A copy that differs only where the reference cannot look: features GARBAGE_FEAT in dead bins (dead_bins), interaction_freq
    GARBAGE_FREQ at entries masked at every resolution."""
    out = copy_batch(batch)
    pd, cd = dead_bins(batch, all_promoter_rows)
    for b in out["promoter_feats"]:
        out["promoter_feats"][b][pd[b]] = GARBAGE_FEAT
        out["pcre_feats"][b][cd[b]] = GARBAGE_FEAT
    out["interaction_freq"][masked_everywhere(batch)] = GARBAGE_FREQ
    return out


# ----------------------------------------------------------------------------- corruptions a wrong kernel would amount to
def corrupt(batch, kind, cfg=None):
    """The batch as a kernel with the named indexing fault would see it (for the sensitivity tests: the oracle on corrupt(batch) must
    differ from the oracle on batch, or the batch cannot detect that fault)."""
    out = copy_batch(batch)
    bins = list(batch["interaction_masks"])
    if kind == "mask_transposed":
        for b in bins:
            out["interaction_masks"][b] = batch["interaction_masks"][b].transpose(-1, -2).contiguous()
    elif kind == "freq_transposed":
        out["interaction_freq"] = batch["interaction_freq"].transpose(-1, -2).contiguous()
    elif kind == "resolution_0_mask_everywhere":
        for b in bins:
            out["interaction_masks"][b] = batch["interaction_masks"][bins[0]].clone()
    elif kind == "freq_rows_above_0_zeroed":
        out["interaction_freq"][:, 1:] = 0.0
    elif kind == "pad_mask_of_a_hole_slot_ignored":
        S = batch["pcre_feats"][bins[0]].shape[1]
        g, s = next((g, s) for g in range(len(batch["label"])) for s in range(S) if pcre_pattern(g, s, S) == "holes"
                    and not bool(torch.stack([m[g, 0, 0, s + 1] for m in batch["interaction_masks"].values()]).all()))
        for b in bins:
            out["pcre_pad_masks"][b][g, s] = False
    else:
        raise KeyError(kind)
    return out


CORRUPTIONS = ("mask_transposed", "freq_transposed", "resolution_0_mask_everywhere", "freq_rows_above_0_zeroed",
               "pad_mask_of_a_hole_slot_ignored")
