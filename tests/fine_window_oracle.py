"""Oracles of the fine window game (cf_mark_fine_coalitions, model.mark_fine_window_*), on the CPU.

  * fine_window_region / fine_window_rows / oracle_fine_window: the rule of include/chromoformer_hip.h evaluated with torch on a batch
    dict, on scan_oracle's extent, rule and centre_row and fine_scan_oracle's kinds.  Players are (marks, (lo, hi)) pairs in finest bins
    relative to the gene's start; gone_f(k) is the OR of the marks of the absent players whose clipped window holds finest bin k; for
    bin j of resolution r and mark m, C = {k in K_j : m in gone_f(k)}: C empty keeps the bits, C = K_j is the scan's log1p(s expm1(u))
    or the donor's element, otherwise the element is rebuilt from the finest children in fp64 (ascending k) as the header states.
  * region_from_edited_raw: the definition itself.  The samples of the absent players' marks inside their windows are multiplied by s
    (once, however many players cover a sample) or replaced by the donor's in the RAW region, which is then binned by
    oracle/dataset_oracle.region.  It never reads a stored feature: the identity between the two is what the tests check."""
import numpy as np
import torch

from oracle import chromoformer_oracle as orc
from oracle import dataset_oracle as dso
from tests import fine_scan_oracle as fo
from tests import scan_oracle as so

NONE, WHOLE, PART = fo.NONE, fo.WHOLE, fo.PART


def windows_players(F, width, n_windows):
    return [(tuple(range(F)), (g * width, (g + 1) * width)) for g in range(n_windows)]


def cells_players(F, width, n_windows):
    return [((f,), (g * width, (g + 1) * width)) for g in range(n_windows) for f in range(F)]


def gone_words(players, present, start, nf):
    """gone_f of one gene -> int64 [max(nf, 1)] of mark words.  present: P bools."""
    gone = np.zeros(max(nf, 1), dtype=np.int64)
    for (ms, (lo, hi)), here in zip(players, present):
        if not here:
            a, b = min(start + lo, nf), min(start + hi, nf)
            gone[a:b] |= sum(1 << f for f in set(ms))
    return gone


def fine_window_region(src, masks, binsizes, players, present, start=0, scale=0.0, flip=False, length=None, donor=None, dtype=torch.float32):
    """The rule on ONE region: src (and donor, or None: the scale rule) {binsize: [L, F]}, masks {binsize: [L] bool centre pad-mask row}
    -> (feats {binsize: [L, F]} in `dtype`, kinds {binsize: [L, F] of NONE / WHOLE / PART}, extra {binsize: [L, F] float64}: the donor
    rule's sum of cnt_k (|expm1 d_k| + |expm1 u_k|) / cnt_j over C of a partly covered element, else 0)."""
    bf = min(binsizes)
    qf, nf = so.extent(masks[bf])
    Lf, F = src[bf].shape
    gone = gone_words(players, present, start, nf)
    cnt = torch.full((max(nf, 1),), float(bf), dtype=torch.float64)
    if length is not None and nf:
        cnt[nf - 1] = length - (nf - 1) * bf
        assert 1 <= cnt[nf - 1] <= bf, (length, nf, bf)
    uf = src[bf].to(dtype)
    df = donor[bf].to(dtype) if donor is not None else None
    frow = (lambda k: qf + nf - 1 - k) if flip else (lambda k: qf + k)
    feats, kinds, extra = {}, {}, {}
    for b in binsizes:
        u = src[b].to(dtype)
        d = donor[b].to(dtype) if donor is not None else None
        L = u.shape[0]
        out, kind, ext = u.clone(), torch.zeros(L, F, dtype=torch.int8), torch.zeros(L, F, dtype=torch.float64)
        q, n = so.extent(masks[b])
        R = Lf // L
        for j in range(n) if gone.any() else ():
            K0, K1 = j * R, min((j + 1) * R, nf)
            if K0 >= K1:
                continue
            some, every = int(np.bitwise_or.reduce(gone[K0:K1])), int(np.bitwise_and.reduce(gone[K0:K1]))
            row = q + n - 1 - j if flip else q + j
            for f in range(F):
                if not some >> f & 1:
                    continue
                if every >> f & 1:
                    kind[row, f] = WHOLE
                    out[row, f] = so.rule(u[row, f], scale) if d is None else d[row, f]
                    continue
                C = [k for k in range(K0, K1) if gone[k] >> f & 1]
                cj = cnt[K0:K1].sum()
                S = torch.zeros((), dtype=torch.float64)
                if d is None:
                    for k in C:                                              # ascending genomic k, each product and sum rounded in fp64
                        S = S + cnt[k] * torch.expm1(uf[frow(k), f]).double()
                    S = (float(np.float32(scale)) - 1.0) * S
                else:
                    if all(torch.equal(df[frow(k), f].view(torch.int32), uf[frow(k), f].view(torch.int32)) for k in C):
                        continue                                             # the donor agrees inside the window: the element keeps its bits
                    for k in C:
                        dk, uk = torch.expm1(df[frow(k), f]).double(), torch.expm1(uf[frow(k), f]).double()
                        S = S + cnt[k] * (dk - uk)
                        ext[row, f] += float(cnt[k] * (dk.abs() + uk.abs()) / cj)
                kind[row, f] = PART
                out[row, f] = torch.log1p((torch.expm1(u[row, f]).double() + S / cj).to(dtype))
        feats[b], kinds[b], extra[b] = out, kind, ext
    return feats, kinds, extra


def keep_bools(keep, P):
    """keep: bool [n_coal, P] or Python ints (bit p set = present) -> bool array [n_coal, P]."""
    if len(keep) and isinstance(keep[0], (int, np.integer)):
        return np.array([[int(w) >> p & 1 for p in range(P)] for w in keep], dtype=bool)
    return np.asarray(keep, dtype=bool).reshape(-1, P)


def fine_window_rows(batch, players, keep, region=0, start=0, lengths=None, flip=None, scale=0.0, donor=None, dtype=torch.float32):
    """-> (feats {binsize: [B, n_coal, L, F]}, rows, kinds {binsize: [B, n_coal, L, F]}, extra): the region's features per (gene,
    coalition), the batch dict of the B * n_coal rows (gene-major), how each element is covered and the donor bound's extra term.
    donor: a batch dict (its features are read) or None."""
    bins = list(batch["promoter_feats"])
    n_bins = {b: batch["promoter_feats"][b].shape[-2] for b in bins}
    F = batch["promoter_feats"][bins[0]].shape[-1]
    B = batch["interaction_freq"].shape[0]
    S = batch["pcre_feats"][bins[0]].shape[1]
    P = len(players)
    keep = keep_bools(keep, P)
    nv = len(keep)
    start = [int(start)] * B if np.ndim(start) == 0 else [int(x) for x in start]
    flip = [False] * B if flip is None else [bool(f) for f in flip]
    feats = {b: torch.empty(B, nv, n_bins[b], F, dtype=dtype) for b in bins}
    kinds = {b: torch.zeros(B, nv, n_bins[b], F, dtype=torch.int8) for b in bins}
    extra = {b: torch.zeros(B, nv, n_bins[b], F, dtype=torch.float64) for b in bins}

    def region_of(bt, b, i):
        L = n_bins[b]
        return bt["promoter_feats"][b].reshape(B, L, F)[i] if region == 0 else bt["pcre_feats"][b].reshape(B, S, L, F)[i, region - 1]

    for i in range(B):
        src, don, masks = {}, ({} if donor is not None else None), {}
        for b in bins:
            L = n_bins[b]
            src[b] = region_of(batch, b, i)
            if donor is not None:
                don[b] = region_of(donor, b, i)
            if region == 0:
                masks[b] = so.centre_row(batch["promoter_pad_masks"][b], B, L)[i]
            else:
                masks[b] = so.centre_row(batch["pcre_pad_masks"][b], B * S, L).reshape(B, S, L)[i, region - 1]
        for c in range(nv):
            f, kd, ex = fine_window_region(src, masks, bins, players, keep[c], start[i], scale, flip[i],
                                           None if lengths is None else int(lengths[i]), don, dtype)
            for b in bins:
                feats[b][i, c], kinds[b][i, c], extra[b][i, c] = f[b], kd[b], ex[b]

    def rep(t):
        t = t.to(dtype) if t.is_floating_point() else t
        return t[:, None].expand(B, nv, *t.shape[1:]).reshape(B * nv, *t.shape[1:]).clone()

    rows = {k: ({b: rep(t) for b, t in v.items()} if isinstance(v, dict) else rep(v)) for k, v in batch.items() if k in so.KEYS}
    for b in bins:
        L = n_bins[b]
        if region == 0:
            rows["promoter_feats"][b] = feats[b].reshape(B * nv, 1, L, F).clone()
        else:
            rows["pcre_feats"][b].reshape(B * nv, S, L, F)[:, region - 1] = feats[b].reshape(B * nv, L, F)
    return feats, rows, kinds, extra


def oracle_fine_window(P, batch, players, keep, cfg=None, dtype=torch.float32, **kw):
    """-> (logits [B, n_coal, n_out], feats, kinds, extra) of fine_window_rows(batch, players, keep, **kw) by orc.forward in `dtype`."""
    feats, rows, kinds, extra = fine_window_rows(batch, players, keep, dtype=dtype, **kw)
    Pd = {k: v.detach().to(dtype) for k, v in P.items()}
    B = batch["interaction_freq"].shape[0]
    with torch.no_grad():
        lg = orc.forward(Pd, rows, cfg)
    return lg.reshape(B, -1, lg.shape[-1]), feats, kinds, extra


def edit_raw(raw, players, present, start, bf, scale=0.0, donor_raw=None, window=None):
    """The raw region [F, n] (fp32 copy) with the absent players' marks, inside their windows of finest bins (`bf` samples each),
    multiplied by `scale` or replaced by donor_raw's samples -- each sample once.  window: the promoter's width."""
    x = np.asarray(raw).astype(np.float32)
    col0, ncols = (0, x.shape[1]) if window is None else (20000 - window // 2, window)
    hit = np.zeros(x.shape, dtype=bool)
    for (ms, (lo, hi)), here in zip(players, present):
        if not here:
            a, b = col0 + min((start + lo) * bf, ncols), col0 + min((start + hi) * bf, ncols)
            if a < b:
                hit[sorted(set(ms)), a:b] = True
    if donor_raw is None:
        x[hit] *= np.float32(scale)
    else:
        x[hit] = np.asarray(donor_raw).astype(np.float32)[hit]
    return x


def region_from_edited_raw(raw, binsizes, n_bins, players, present, start=0, scale=0.0, strand="+", window=None, donor_raw=None):
    """The definition: edit_raw, then oracle/dataset_oracle.region -> {binsize: [L, F]}."""
    x = edit_raw(raw, players, present, start, min(binsizes), scale, donor_raw, window)
    return {bs: dso.region(x, bs, L, strand, window)[0].t() for bs, L in zip(binsizes, n_bins)}


def bound_factor(src, feats, kinds, extra):
    """((1 + m_j) + extra) / (1 + m') of every element -> tensor like feats (1 where the element is not partly covered): the factor of
    the bound c 2^-24 (...) on a partly covered element (extra = 0 under the scale rule)."""
    r = (torch.exp(src.double()) + extra) / torch.exp(feats.double())
    return torch.where(kinds == PART, r, torch.ones_like(r))
