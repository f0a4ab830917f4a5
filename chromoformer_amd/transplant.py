"""pCRE transplant screen: what would a gene's prediction be if another enhancer were brought into contact with its promoter, and how
does the answer depend on contact strength?  A library of candidate regions -- binned from raw files as the dataset bins a partner,
or gathered from the slots of a batch -- is tried in one pCRE slot of every gene, each candidate at several contact frequencies
(cf_pcre_transplant; csrc/cf_transplant.h).  Structural variants and enhancer hijacking are the questions it serves.

Functions on a model (a chromoformer_amd.net class on a GPU), not methods of it: the public names of the model classes are a kept
surface (tests/golden/model_api.json), as for chromoformer_amd.contact and chromoformer_amd.backselect.  There is no PyTorch fallback:
the rows come from the library's kernels.

The rule.  Candidate c in slot j of gene b at frequency f: the slot's features and centre pad-mask row become the candidate's at every
resolution; row and column j + 1 of the interaction mask become "masked where the other token is dead" with the diagonal entry live, at
every resolution; interaction_freq[b, 0, j + 1] becomes f and every other entry of row and column j + 1 becomes 0 -- what
ChromoformerDataset builds for the gene with that partner replaced (j < n_part) or appended (j = n_part) at score f.  The result is
model(...) under no_grad on those tensors, bit for bit.  A slot's Pairwise output depends on the promoter and on that slot alone and the
Regulation stack has no positional encoding, so i_max candidates share one pass of the Embedding + Pairwise stage as the slots of a
pseudo-gene, and a dose-response over Q frequencies costs Regulation + head rows only.

Limits: one slot per row (combinations of transplants are not covered); promoters are not transplanted; candidates are never stored
mirrored; the edited features are not returned."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from . import attribution as A
from .data import bin_log1p, centred


class Library:
    """Candidate regions of a transplant screen: feats {binsize: float32 [C, L, F]}, mask_rows {binsize: uint8 [C, L]} (the centre
    pad-mask row, non-zero = masked), names [C] and coords, [(chrom, start, end)] or None."""

    def __init__(self, feats, mask_rows, names=None, coords=None):
        self.feats = {int(b): torch.as_tensor(t, dtype=torch.float32) for b, t in feats.items()}
        self.mask_rows = {int(b): torch.as_tensor(t).to(torch.uint8) for b, t in mask_rows.items()}
        if sorted(self.feats) != sorted(self.mask_rows) or not self.feats:
            raise ValueError("Library: feats and mask_rows must hold the same bin sizes, at least one")
        n = {t.shape[0] for t in self.feats.values()} | {t.shape[0] for t in self.mask_rows.values()}
        if len(n) != 1 or min(n) < 1:
            raise ValueError("Library: every resolution must hold the same number of candidates, at least 1")
        for b, t in self.feats.items():
            if t.dim() != 3 or self.mask_rows[b].shape != t.shape[:2]:
                raise ValueError("Library: feats[%d] must be [C, L, F] and mask_rows[%d] [C, L]" % (b, b))
        C_ = n.pop()
        self.names = ["cand%d" % c for c in range(C_)] if names is None else [str(s) for s in names]
        self.coords = None if coords is None else [tuple(c) for c in coords]
        if len(self.names) != C_ or (self.coords is not None and len(self.coords) != C_):
            raise ValueError("Library: %d candidates, %d names%s" % (C_, len(self.names), "" if self.coords is None else ", %d coords" % len(self.coords)))

    def __len__(self):
        return len(self.names)

    def select(self, index):
        """The candidates `index` (a sequence of ints), in that order -> Library."""
        idx = torch.as_tensor(list(index), dtype=torch.long)
        return Library({b: t[idx.to(t.device)] for b, t in self.feats.items()}, {b: t[idx.to(t.device)] for b, t in self.mask_rows.items()},
                       [self.names[i] for i in idx.tolist()], None if self.coords is None else [self.coords[i] for i in idx.tolist()])


def library_from_regions(dataset, regions):
    """Candidates from raw regions -> Library.  regions: (chrom, start, end[, name]) tuples; each raw `chrom:start-end.npy` file is
    loaded through dataset._load and binned exactly as the dataset bins a partner (bin_log1p, centred: never mirrored), so a candidate
    is bit-equal to what ChromoformerDataset puts in a slot for that partner.  A region longer than w_max is refused."""
    ds = dataset
    regions = [tuple(r) for r in regions]
    if not regions:
        raise ValueError("library_from_regions: at least 1 region")
    feats = {b: [] for b in ds.binsizes}
    rows = {b: [] for b in ds.binsizes}
    names, coords = [], []
    for reg in regions:
        if len(reg) not in (3, 4):
            raise ValueError("library_from_regions: a region is (chrom, start, end[, name]); got %r" % (reg,))
        chrom, start, end = str(reg[0]), int(reg[1]), int(reg[2])
        if end <= start:
            raise ValueError("library_from_regions: %s:%d-%d is empty" % (chrom, start, end))
        if end - start > ds.w_max:
            raise ValueError("library_from_regions: %s:%d-%d spans %d samples, more than w_max = %d" % (chrom, start, end, end - start, ds.w_max))
        raw = torch.as_tensor(ds._load(chrom, start, end)).to(torch.float32)
        if raw.shape[0] != ds.n_feats:
            raise ValueError("library_from_regions: expected %d feature rows, %s:%d-%d has %d" % (ds.n_feats, chrom, start, end, raw.shape[0]))
        for b in ds.binsizes:
            L = ds.w_max // b
            x, lo, n = centred(bin_log1p(raw, b), L)
            m = torch.ones(L, dtype=torch.uint8)
            m[lo:lo + n] = 0
            feats[b].append(x.t())
            rows[b].append(m)
        names.append(str(reg[3]) if len(reg) == 4 else "%s:%d-%d" % (chrom, start, end))
        coords.append((chrom, start, end))
    return Library({b: torch.stack(v) for b, v in feats.items()}, {b: torch.stack(v) for b, v in rows.items()}, names, coords)


def library_from_batch(batch, pairs):
    """Existing pCREs as candidates ("give gene A gene B's enhancer") -> Library.  batch: a batch dict (the reference's layout with
    [B, S, 1, L, L] pad masks, or a store's compact [B, S, L] rows); pairs: (gene, slot) index pairs of it.  Each candidate is the
    slot's features with its centre pad-mask row."""
    pairs = [(int(g), int(s)) for g, s in pairs]
    if not pairs:
        raise ValueError("library_from_batch: at least 1 (gene, slot) pair")
    feats, rows = {}, {}
    for b, cf in batch["pcre_feats"].items():
        B, S, L = cf.shape[0], cf.shape[1], cf.shape[2]
        for g, s in pairs:
            if not (0 <= g < B and 0 <= s < S):
                raise ValueError("library_from_batch: pair (%d, %d) outside the batch's %d genes x %d slots" % (g, s, B, S))
        m = torch.as_tensor(batch["pcre_pad_masks"][b])
        m = m.reshape(B, S, L, L)[:, :, L // 2] if m.numel() == B * S * L * L else m.reshape(B, S, L)
        gi, si = torch.as_tensor([g for g, _ in pairs], device=cf.device), torch.as_tensor([s for _, s in pairs], device=cf.device)
        feats[int(b)] = cf[gi, si].to(torch.float32)
        rows[int(b)] = m[gi.to(m.device), si.to(m.device)].to(torch.uint8)
    return Library(feats, rows, ["gene%d:slot%d" % p for p in pairs])


def broadcast_freq(freq, B, n_cand, who="pcre_transplant"):
    """freq: a scalar, [Q], [C, Q] or [B, C, Q] -> a float32 host tensor [B, C, Q], every value finite."""
    f = torch.as_tensor(freq, dtype=torch.float32).detach().cpu()
    if f.dim() == 0:
        f = f.reshape(1)
    if f.dim() > 3 or f.shape[-1] < 1:
        raise ValueError("%s: freq must be a scalar, [Q], [C, Q] or [B, C, Q] with Q >= 1; got shape %s" % (who, tuple(f.shape)))
    if f.dim() == 2 and f.shape[0] != n_cand:
        raise ValueError("%s: freq [C, Q] has %d rows, the library holds %d candidates" % (who, f.shape[0], n_cand))
    if f.dim() == 3 and tuple(f.shape[:2]) != (B, n_cand):
        raise ValueError("%s: freq [B, C, Q] is %s, the call has B = %d genes and C = %d candidates" % (who, tuple(f.shape), B, n_cand))
    if not bool(torch.isfinite(f).all()):
        raise ValueError("%s: freq must be finite" % who)
    return f.expand(B, n_cand, f.shape[-1]).contiguous()


def slot_argument(slot, B, i_max, who="pcre_transplant"):
    """slot: "append", an int in [0, i_max), or B ints each in [-1, i_max) -> (slot_all, int32 host tensor [B] or None)."""
    if isinstance(slot, str):
        if slot != "append":
            raise ValueError("%s: slot = %r: 'append', a slot in [0, i_max = %d) or one slot per gene" % (who, slot, i_max))
        return -1, None
    if isinstance(slot, (int, np.integer)) and not isinstance(slot, bool):
        if not 0 <= int(slot) < i_max:
            raise ValueError("%s: slot = %d outside [0, i_max = %d)" % (who, int(slot), i_max))
        return int(slot), None
    s = torch.as_tensor(slot).detach().cpu()
    if s.dim() != 1 or s.shape[0] != B or s.is_floating_point() or s.dtype == torch.bool:
        raise ValueError("%s: slot must be 'append', an int or %d ints (one per gene)" % (who, B))
    if bool(((s < -1) | (s >= i_max)).any()):
        raise ValueError("%s: every slot must lie in [-1, i_max = %d); -1 = the gene is not placed" % (who, i_max))
    return 0, s.to(torch.int32).contiguous()


@torch.no_grad()
def pcre_transplant(model, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                    interaction_freq=None, library=None, freq=1.0, slot="append"):
    """The prediction with each candidate of `library` in one pCRE slot of every gene, at each contact frequency (cf_pcre_transplant)
    -> (logits [B, C, Q, n_out], info), tensors on the model's device, no autograd graph.  logits[b, c, q] is model(...) under no_grad
    on gene b's tensors edited by the module's rule for candidate c at freq[b, c, q], bit-equal.

      library   a Library (library_from_regions, library_from_batch)
      freq      a scalar, [Q], [C, Q] or [B, C, Q]: the contact frequencies, the score the dataset would write for the partner
      slot      "append": each gene's first dead token (a gene whose i_max slots are all live is not placed); an int: that slot for
                every gene, replacing what it holds; B ints: one slot per gene, -1 = not placed
      info      logits [B, n_out]: the unedited prediction; slot int32 [B]: the slot used, -1 = not placed; placed bool [B]; names: the
                candidates' names.  Every row of a gene that is not placed carries the bits of its unedited prediction.

    The Embedding + Pairwise stage runs once on the B genes and once per ceil(C / i_max) pseudo-genes, the Regulation stack and the
    head on the B * (1 + C * Q) rows.  The first argument after the model may also be a packed batch (an engine.Slot or a pack_batch
    result), with nothing after it.  The pass overwrites the activations a grad-enabled model(...) keeps for its backward: such a
    pending backward() raises."""
    who = "pcre_transplant"
    if not isinstance(library, Library):
        raise ValueError("%s: library must be a transplant.Library (library_from_regions, library_from_batch)" % who)
    if sorted(library.feats) != sorted(int(b) for b in model.binsizes):
        raise ValueError("%s: the library holds bin sizes %s, the model %s" % (who, sorted(library.feats), list(model.binsizes)))
    for b, L in zip(model.binsizes, model.n_bins):
        if tuple(library.feats[int(b)].shape[1:]) != (L, model.n_feats):
            raise ValueError("%s: library.feats[%d] is %s per candidate, the model reads [%d, %d]" % (who, b, tuple(library.feats[int(b)].shape[1:]), L, model.n_feats))
    bs, book = model._attrib_call(who, promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq)
    B, n_cand, dev = bs.B, len(library), model._device
    f = broadcast_freq(freq, B, n_cand, who).to(dev)
    slot_all, slots = slot_argument(slot, B, model.i_max, who)
    Q = f.shape[-1]
    if B * (1 + n_cand * Q) > 0x7fffffff:
        raise ValueError("%s: B * (1 + C * Q) = %d rows do not fit an int" % (who, B * (1 + n_cand * Q)))
    opts = _lib.cf_transplant_opts()
    opts.n_cand, opts.n_freq, opts.slot_all = n_cand, Q, slot_all
    alive = [f]
    for r, b in enumerate(model.binsizes):
        lf = library.feats[int(b)].to(dev, torch.float32).contiguous()
        lm = library.mask_rows[int(b)].to(dev, torch.uint8).contiguous()
        alive += [lf, lm]
        opts.lib_feats[r], opts.lib_mask[r] = lf.data_ptr(), lm.data_ptr()
    opts.freq = f.data_ptr()
    if slots is not None:
        slots = slots.to(dev)
        opts.slot = slots.data_ptr()
    slot_out = torch.empty(B, dtype=torch.int32, device=dev)
    opts.slot_out = slot_out.data_ptr()
    rows = torch.empty(B, 1 + n_cand * Q, model.n_out, device=dev)      # (written in full by the library)
    st = book()
    _lib.check(_lib.lib().cf_pcre_transplant(model._handle, C.byref(bs), C.byref(opts), rows.data_ptr(), st), "cf_pcre_transplant")
    del alive
    info = {"logits": rows[:, 0].clone(), "slot": slot_out, "placed": slot_out >= 0, "names": list(library.names)}
    return rows[:, 1:].reshape(B, n_cand, Q, model.n_out), info


def pcre_transplant_dataset(model, dataset, regions_or_library, freqs, slot="append", genes=None, bsz=None, store=None):
    """pcre_transplant over the genes of a ChromoformerDataset: a generator over `genes` (ids; default: the dataset's) in chunks of
    at most min(bsz, model.max_batch) genes; per gene it yields a dict of host arrays:

        gene_id      the id
        logits       float32 [n_out]: the unedited prediction
        transplant   float32 [C, Q, n_out]: the logits with candidate c in the gene's slot at freqs[q]
        slot         the slot used, -1 = not placed;  placed  bool
        candidates   the candidates' names

    regions_or_library: a Library, or (chrom, start, end[, name]) tuples for library_from_regions (the raw files are in the dataset's
    directory).  freqs: a scalar or [Q]; slot: "append" or an int.  The genes' binned features come from `store` (a device-resident
    GeneStore holding `genes` in order) if given, else as for the other generators (attribution._batches)."""
    who = "pcre_transplant_dataset"
    ds = dataset
    binsizes, _, genes, chunk = A._open(who, model, ds, genes, bsz)
    library = regions_or_library if isinstance(regions_or_library, Library) else library_from_regions(ds, regions_or_library)
    f = torch.as_tensor(freqs, dtype=torch.float32).reshape(-1)
    broadcast_freq(f, 1, len(library), who)
    if not isinstance(slot, (str, int, np.integer)):
        raise ValueError("%s: slot = %r: 'append' or one slot for every gene" % (who, slot))
    slot_argument(slot, 1, model.i_max, who)
    for ids, _, _, args, _, _ in A._batches(who, model, ds, genes, chunk, binsizes, store):
        lg, info = pcre_transplant(model, *args, library=library, freq=f, slot=slot)
        lg, base, used = lg.cpu().numpy(), info["logits"].cpu().numpy(), info["slot"].cpu().numpy()
        for i, g in enumerate(ids):
            yield dict(gene_id=g, logits=base[i].copy(), transplant=lg[i].copy(), slot=int(used[i]), placed=bool(used[i] >= 0),
                       candidates=list(library.names))


def read_bed(path):
    """`chrom start end [name]` lines of a BED file (tab or blank separated; empty lines, `#`, `track` and `browser` lines skipped)
    -> [(chrom, start, end[, name])]."""
    regions = []
    with open(path) as fh:
        for n, line in enumerate(fh, 1):
            w = line.split()
            if not w or w[0].startswith("#") or w[0] in ("track", "browser"):
                continue
            if len(w) < 3 or not (w[1].isdigit() and w[2].isdigit()):
                raise ValueError("%s line %d: expected `chrom start end [name]`" % (path, n))
            regions.append((w[0], int(w[1]), int(w[2])) + ((w[3],) if len(w) > 3 else ()))
    if not regions:
        raise ValueError("%s holds no region" % path)
    return regions
