"""Fine-resolution perturbation scan, host side (no GPU): the rule of include/chromoformer_hip.h (tests/fine_scan_oracle.fine_region,
evaluated in fp32 as the kernel does) equals binning the raw signal scaled inside the window; whole coarse bins reproduce the coarse
scan's rows bit for bit; the C ABI declares, exports and mirrors cf_perturbation_scan_fine.

Tolerances.  An element of a wholly covered bin (every finest element is one) passes through the scan's function: 3e-7, the scan's
figure.  An element of a partly covered bin is rebuilt from rounded fp32 features, m' = m_j + (s - 1) S / cnt_j, and a relative error
eps in 1 + m_j becomes eps (1 + m_j) / (1 + m') in u' = log(1 + m'): the bound is PART_C 2^-24 (1 + m_j) / (1 + m')."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from chromoformer_amd import _lib
from tests import fine_scan_oracle as fo
from tests import scan_oracle as so
from tests.test_perturbation_scan_cpu import BINS, NB, MARKS, _binned, _raw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHOLE_TOL = 3e-7
#: twice the worst |u' - from raw| / (2^-24 (1 + m_j) / (1 + m')) observed over every case of this file: 8.135 (the dataset test; 8.007
#: at length 39901, at most 3.83 at the other lengths).  The large ratios belong to s = 2.5, where (1 + m_j) / (1 + m') < 1 shrinks the
#: bound below the ulp of the result (2.4e-7 = 4 x 2^-24 for a feature in [2, 4)).
PART_C = 16.27
SCALES = (0.0, 0.5, 2.5)
LENGTHS = [100, 1999, 2000, 2001, 7300, 12345, 39901, 40000]


def _windows(nf):
    """The windows of a region of nf finest bins: width 1 at the first and the last child of coarse bins (the first, a middle one, the
    tail), width 7 at stride 3 from the start and across the tail (500-bp and 2-kb boundaries fall inside), windows that end inside the
    tail bins, one past the end."""
    w = set()
    for j in {0, (nf - 1) // 40, (nf - 1) // 20}:
        w |= {(20 * j, 20 * j + 1), (min(20 * j + 19, nf - 1), min(20 * j + 19, nf - 1) + 1), (20 * j + 4, 20 * j + 5), (20 * j + 5, 20 * j + 6)}
    for s0 in (0, 2, max(nf - 31, 0)):
        w |= {(s0 + 3 * g, s0 + 3 * g + 7) for g in range(10)}
    w |= {(nf - 1, nf), (max(nf - 3, 0), nf - 1), (max(nf - 8, 0), nf + 5), (nf, nf + 7)}
    return sorted((lo, hi) for lo, hi in w if lo >= 0)


def _check(src, masks, raw, strand, window, length, stats):
    """Every window of _windows and every scale on one region: the fp32 rule against the from-raw definition."""
    nf = so.extent(masks[100])[1]
    for lo, hi in _windows(nf):
        for s in SCALES:
            got, kinds = fo.fine_region(src, masks, BINS, lo, hi, MARKS, s, strand != "+", length)
            ref = fo.region_from_scaled_raw(raw, BINS, NB, lo, hi, MARKS, s, strand, window)
            for b in BINS:
                assert not torch.isnan(got[b]).any() and not torch.isnan(ref[b]).any()
                err = (got[b].double() - ref[b].double()).abs()
                part = (kinds[b] == fo.PART)[:, None].expand_as(err)
                fac = fo.partial_bound_factor(src[b], got[b], kinds[b])
                if lo >= nf:
                    assert torch.equal(got[b], src[b]), (lo, hi, "a window past the real bins changes nothing")
                if b == 100:
                    assert not part.any()
                stats["whole"] = max(stats["whole"], err[~part].max().item())
                if part.any():
                    stats["n_part"] += int(part[:, MARKS[0]].sum())
                    stats["ratio"] = max(stats["ratio"], (err[part] / (2.0 ** -24 * fac[part])).max().item())
                assert err[~part].max().item() <= WHOLE_TOL, (lo, hi, s, b, err[~part].max().item())
                assert bool((err <= torch.where(part, PART_C * 2.0 ** -24 * fac, torch.full_like(fac, WHOLE_TOL))).all()), (lo, hi, s, b)


@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("strand", ["+", "-"])
def test_rule_equals_binning_the_scaled_signal(length, strand):
    raw = _raw(length, length)
    base = _binned(raw, strand, None)
    src = {b: base["promoter_feats"][b][0, 0] for b in BINS}
    masks = {b: base["promoter_pad_masks"][b][0] for b in BINS}
    stats = dict(whole=0.0, ratio=0.0, n_part=0)
    _check(src, masks, raw, strand, None, length, stats)
    print("length %d strand %s: whole %.3e, partial ratio %.3f over %d partly covered bins" % (length, strand, stats["whole"], stats["ratio"], stats["n_part"]))
    assert stats["n_part"] or length <= 100


def test_rule_on_a_dataset_both_strands_and_the_narrowed_mirrored_promoter(tmp_path):
    """scan_oracle.scan_dataset at w_prom = 39000: a '-' strand promoter of 19.5 coarse bins stored mirrored (the short coarse bin, ten
    children, FIRST), a '+' strand one, pCREs with partial tails at every resolution; the batch is the dataset's own."""
    ds = so.scan_dataset(str(tmp_path), w_prom=39000)
    minus = [x for x in ds.target_genes if ds.genes[x]["tss"][2] == "-" and ds.genes[x]["pcres"]][0]
    plus = [x for x in ds.target_genes if ds.genes[x]["tss"][2] == "+" and ds.genes[x]["pcres"]][0]
    stats = dict(whole=0.0, ratio=0.0, n_part=0)
    for gid in (minus, plus):
        chrom, tss, strand = ds.genes[gid]["tss"]
        batch = so.dataset_batch(ds, [gid])
        raw = ds._load(chrom, tss - 20000, tss + 20000)
        src = {b: batch["promoter_feats"][b][0, 0] for b in BINS}
        masks = {b: so.centre_row(batch["promoter_pad_masks"][b], 1, 40000 // b)[0] for b in BINS}
        assert so.extent(masks[100])[1] == 390 and so.extent(masks[2000])[1] == 20
        _check(src, masks, raw, strand, 39000, 39000, stats)
        c, s, e = ds.genes[gid]["pcres"][0]
        src = {b: batch["pcre_feats"][b][0, 0] for b in BINS}
        masks = {b: so.centre_row(batch["pcre_pad_masks"][b], 8, 40000 // b)[0] for b in BINS}
        _check(src, masks, ds._load(c, s, e), "+", None, e - s, stats)
    print("dataset: whole %.3e, partial ratio %.3f over %d partly covered bins" % (stats["whole"], stats["ratio"], stats["n_part"]))
    # a wrong mirror mapping is caught: the first finest genomic bin of the '-' promoter is the LAST real row
    batch = so.dataset_batch(ds, [minus])
    got, _, kinds = fo.fine_rows(batch, scale=0.0, width=1, n_windows=1, mark_sets=[MARKS], flip=[True])
    assert (got[100][0, 1] != got[100][0, 0]).any(-1).nonzero().flatten().tolist() == [394]      # 390 real rows in [5, 395)
    assert kinds[2000][0, 1].nonzero().flatten().tolist() == [19] and int(kinds[2000][0, 1, 19]) == fo.PART


def test_lengths_none_is_a_full_last_bin_bit_for_bit():
    raw = _raw(12345, 3)
    base = _binned(raw, "+", None)
    nf = 124
    kw = dict(scale=0.5, width=7, stride=3, start=95, n_windows=10, mark_sets=[MARKS, (0,)])
    a, _, _ = fo.fine_rows(base, lengths=None, **kw)
    b, _, _ = fo.fine_rows(base, lengths=[nf * 100], **kw)
    c, _, _ = fo.fine_rows(base, lengths=[12345], **kw)
    assert all(torch.equal(a[bs], b[bs]) for bs in BINS)
    assert not torch.equal(a[2000], c[2000]) and torch.equal(a[100], c[100])      # the true length re-weights the tail's coarse bins only


@pytest.mark.parametrize("w", [1, 3])
def test_a_union_of_coarse_bins_is_the_coarse_scan_bit_for_bit(tmp_path, w):
    ds = so.scan_dataset(str(tmp_path), w_prom=39000)
    genes = ["ENSGSYN00001", "ENSGSYN00000", "ENSGSYN00002"]
    batch = so.dataset_batch(ds, genes)
    flips = [ds.genes[g]["tss"][2] != "+" for g in genes]
    for region, fl in ((0, flips), (1, None)):
        coarse, _ = so.scan_rows(batch, region=region, scale=2.5, width=w, mark_sets=[MARKS, (3,)], flip=fl)
        n_win = -(-20 // w)
        fine, _, kinds = fo.fine_rows(batch, region=region, scale=2.5, width=20 * w, stride=20 * w, mark_sets=[MARKS, (3,)], flip=fl)
        assert fine[100].shape[1] == 1 + 2 * n_win
        for k in range(2):
            for g in range(n_win):
                for b in BINS:
                    assert torch.equal(fine[b][:, 1 + k * n_win + g], coarse[b][:, 1 + k * 20 + g * w]), (region, k, g, b)
        assert not any((kinds[b] == fo.PART).any() for b in BINS)


def test_oracle_logits_equal_the_golden(tmp_path):
    """The reference's own dataset and model on raw files scaled inside fine windows (tests/golden/make_fine_scan_goldens.py) against
    the rule + orc.forward on the unscaled dataset: the project's 1e-4 (observed 2.68e-07 when the golden was made)."""
    from oracle import chromoformer_oracle as orc
    from tests.helpers import GOLDEN
    g = np.load(os.path.join(GOLDEN, "fine_scan.npz"))
    ds = so.scan_dataset(str(tmp_path), w_prom=int(g["w_prom"]))
    genes = [str(x) for x in g["genes"]]
    base = so.dataset_batch(ds, genes)
    flips = [ds.genes[x]["tss"][2] != "+" for x in genes]
    assert len(g["cases"]) == 6
    for head, regression in (("clf", False), ("reg", True)):
        P = orc.init_params(None, 42, regression)
        for k, (region, lo, hi, scale) in enumerate(g["cases"].tolist()):
            region, lo, hi = int(region), int(lo), int(hi)
            marks = tuple(np.flatnonzero(g["marks"][k]).tolist())
            lg, _, _ = fo.oracle_fine(P, base, region=region, scale=float(scale), width=hi - lo, start=lo, n_windows=1, mark_sets=[marks],
                                      lengths=g["lengths"][k].tolist(), flip=flips if region == 0 else None)
            d = (lg - torch.from_numpy(g[head][k])).abs().max().item()      # [B, 2, n_out]: unperturbed, perturbed
            print(head, "case", k, "oracle vs reference %.2e" % d)
            assert d < 1e-4, (head, k, d)


def test_abi_symbol_struct_and_null_handle():
    hdr = open(os.path.join(ROOT, "include", "chromoformer_hip.h")).read()
    assert re.search(r"int cf_perturbation_scan_fine\(cf_handle\* h, const cf_batch\* batch, const cf_scan_fine_opts\* opts, float\* logits, void\* stream\);", hdr)
    assert "cf_perturbation_scan_fine" in _lib.SYMBOLS
    o = _lib.cf_scan_fine_opts
    # int region, n_sets; const unsigned*; float scale; (pad) const uint8_t*; int width, stride, n_windows; (pad) const int* x 2; float* [3]
    assert C.sizeof(o) == 8 + 8 + 8 + 8 + 16 + 16 + 8 * _lib.MAX_RES == 88
    assert [o.region.offset, o.mark_sets.offset, o.scale.offset, o.flip.offset, o.width.offset, o.start.offset, o.lengths.offset,
            o.feats_out.offset] == [0, 8, 16, 24, 32, 48, 56, 64]
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct cf_scan_fine_opts \{(.*?)\} cf_scan_fine_opts;", hdr, re.S).group(1), flags=re.S)
    assert re.findall(r"(\w+)(?:\[CF_MAX_RES\])?[;,]", body) == [n for n, _ in o._fields_]
    # the existing structs keep their sizes
    assert C.sizeof(_lib.cf_scan_opts) == 64 and C.sizeof(_lib.cf_scan_regions_opts) == 40
    L = _lib.lib()
    assert L.cf_abi_version() == 1
    assert L.cf_perturbation_scan_fine(None, None, None, None, None) != 0
    assert L.cf_last_error() == b"cf_perturbation_scan_fine: null handle"
