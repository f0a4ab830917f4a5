"""In-silico perturbation scan, host side (no GPU): the rule log1p(s expm1(u)) on the covered rows equals binning the scaled raw
signal; the oracle reproduces the reference's logits on scaled raw files (golden); the C ABI declares, exports and mirrors
cf_perturbation_scan; real windows map to genomic coordinates and to stored rows as the header says, for both strands."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from chromoformer_amd import _lib
from oracle import chromoformer_oracle as orc
from oracle import dataset_oracle as dso
from tests import scan_oracle as so
from tests.helpers import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINS, NB, F = (2000, 500, 100), (20, 80, 400), 7
MARKS = (1, 4)


def _raw(length, seed):
    rng = np.random.default_rng(seed)
    x = rng.poisson(np.abs(np.cumsum(rng.normal(0, 0.04, size=(F, length)), axis=1)) * 0.9 + 0.3).astype(np.float16)
    x[:, rng.random(length) < 0.25] = 0
    return x


def _binned(raw, strand, window):
    """-> the one-gene batch dict whose promoter is the region binned by oracle/dataset_oracle.region (compact masks)."""
    b = {k: {} for k in so.KEYS[:5]}
    for bs, L in zip(BINS, NB):
        out, left, n, _ = dso.region(raw, bs, L, strand, window)
        m = torch.ones(1, L, dtype=torch.bool)
        m[0, left:left + n] = False
        b["promoter_feats"][bs], b["promoter_pad_masks"][bs] = out.t()[None, None], m
        b["pcre_feats"][bs], b["pcre_pad_masks"][bs] = torch.zeros(1, 1, L, F), torch.ones(1, 1, L, dtype=torch.bool)
        b["interaction_masks"][bs] = torch.zeros(1, 1, 2, 2, dtype=torch.bool)
    b["interaction_freq"] = torch.zeros(1, 2, 2)
    return b


def _worst(raw, strand, window, widths=(1, 3), scales=(0.0, 2.5), dtype=torch.float64):
    """max |rule - binning of the scaled signal| over every window, width, scale and resolution of one region."""
    col0, ncols = (0, raw.shape[1]) if window is None else (20000 - window // 2, window)
    base = _binned(raw, strand, window)
    n_c = -(-ncols // BINS[0])
    worst = 0.0
    for w in widths:
        for s in scales:
            feats, _ = so.scan_rows(base, region=0, scale=s, width=w, mark_sets=[MARKS], flip=[strand != "+"], dtype=dtype)
            for g in range(NB[0]):
                x = raw.astype(np.float32)
                lo, hi = col0 + g * BINS[0], col0 + min((g + w) * BINS[0], ncols)
                if lo < hi:
                    x[list(MARKS), lo:hi] *= np.float32(s)
                for bs, L in zip(BINS, NB):
                    ref = dso.region(x, bs, L, strand, window)[0].t().double()
                    got = feats[bs][0, 1 + g].double()
                    if g >= n_c:
                        assert torch.equal(got, base["promoter_feats"][bs][0, 0].double()), (g, "a dead window changes nothing")
                    worst = max(worst, (got - ref).abs().max().item())
    return worst


@pytest.mark.parametrize("length", [100, 1999, 2000, 2001, 7300, 12345, 39901, 40000])
@pytest.mark.parametrize("strand", ["+", "-"])
def test_rule_equals_binning_the_scaled_signal(length, strand):
    """fp64 evaluation of the rule on the fp32 features against oracle/dataset_oracle.region of the scaled raw signal: 1e-6, three
    times the 3.1e-7 measured over these cases (the features are fp32: log(1 + m) of means up to ~20 carries ~1e-7 each way)."""
    worst = _worst(_raw(length, length), strand, None)
    print("length %d strand %s: worst %.2e" % (length, strand, worst))
    assert worst <= 1e-6


def test_rule_on_a_narrowed_mirrored_promoter():
    """w_prom = 39000 on the '-' strand: 19.5 coarse bins, the short last one stored FIRST; a wrong mirror mapping scales the wrong rows."""
    raw = _raw(40000, 7)
    worst = _worst(raw, "-", 39000)
    print("narrowed '-' promoter: worst %.2e" % worst)
    assert worst <= 1e-6
    base = _binned(raw, "-", 39000)
    feats, _ = so.scan_rows(base, region=0, scale=0.0, width=1, mark_sets=[MARKS], flip=[True], dtype=torch.float64)
    ch = (feats[500][0, 1 + 19] != feats[500][0, 0]).any(-1).nonzero().flatten().tolist()      # the last genomic window: 2 bins of 500
    assert ch and set(ch) <= {1, 2}, ch                                                        # 78 real rows in [1, 79), mirrored
    wrong, _ = so.scan_rows(base, region=0, scale=0.0, width=1, mark_sets=[MARKS], flip=[False], dtype=torch.float64)
    x = raw.astype(np.float32)
    x[list(MARKS), 500 + 38000:500 + 39000] = 0
    ref = dso.region(x, 500, 80, "-", 39000)[0].t().double()
    assert (wrong[500][0, 1 + 19] - ref).abs().max().item() > 1e-3                             # the unmirrored mapping is caught


def test_fp32_evaluation_of_the_rule():
    """The same in fp32 (what the kernel computes, up to the last bit of log1pf / expm1f): 2.4e-7 here, one ulp of a feature in [2, 4).
    Bound: the fp64 bound above, 1e-6 = four such ulps -- the rule adds two rounded operations to the two the features already carry."""
    worst = max(_worst(_raw(n, n), s, None, dtype=torch.float32) for n in (1999, 7300, 12345) for s in "+-")
    print("fp32 evaluation: worst %.2e" % worst)
    assert worst <= 1e-6


def test_oracle_logits_equal_the_golden():
    """The reference's own dataset and model on scaled raw files (tests/golden/make_perturbation_scan_goldens.py) against the rule +
    orc.forward on the unscaled dataset."""
    import tempfile
    g = np.load(os.path.join(GOLDEN, "perturbation_scan.npz"))
    with tempfile.TemporaryDirectory() as tmp:
        ds = so.scan_dataset(tmp, w_prom=int(g["w_prom"]))
        genes = [str(x) for x in g["genes"]]
        base = so.dataset_batch(ds, genes)
        flips = [ds.genes[x]["tss"][2] != "+" for x in genes]
        for head, regression in (("clf", False), ("reg", True)):
            P = orc.init_params(None, 42, regression)
            for k, (region, win, width, scale) in enumerate(g["cases"].tolist()):
                marks = tuple(np.flatnonzero(g["marks"][k]).tolist())
                lg, _ = so.oracle_scan(P, base, region=int(region), scale=float(scale), width=int(width), mark_sets=[marks],
                                       flip=flips if region == 0 else None, variants=[0, 1 + int(win)])
                ref = torch.from_numpy(g[head][k])                                  # [B, 2, n_out]: unperturbed, perturbed
                d = (lg - ref).abs().max().item()
                print(head, "case", k, "oracle vs reference %.2e" % d)
                assert d < 1e-5, (head, k, d)


def test_abi_symbol_struct_and_null_handle():
    hdr = open(os.path.join(ROOT, "include", "chromoformer_hip.h")).read()
    assert re.search(r"int cf_perturbation_scan\(cf_handle\* h, const cf_batch\* batch, const cf_scan_opts\* opts, float\* logits, void\* stream\);", hdr)
    assert "cf_perturbation_scan" in _lib.SYMBOLS
    # int region, width, n_sets; (pad) const unsigned*; float scale; (pad) const uint8_t*; float* [3]
    assert C.sizeof(_lib.cf_scan_opts) == 16 + 8 + 8 + 8 + 8 * _lib.MAX_RES == 64
    assert [_lib.cf_scan_opts.region.offset, _lib.cf_scan_opts.mark_sets.offset, _lib.cf_scan_opts.scale.offset,
            _lib.cf_scan_opts.flip.offset, _lib.cf_scan_opts.feats_out.offset] == [0, 16, 24, 32, 40]
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct cf_scan_opts \{(.*?)\} cf_scan_opts;", hdr, re.S).group(1), flags=re.S)
    assert re.findall(r"(\w+)(?:\[CF_MAX_RES\])?;", body) == [n for n, _ in _lib.cf_scan_opts._fields_]
    L = _lib.lib()
    assert L.cf_perturbation_scan(None, None, None, None, None) != 0
    assert L.cf_last_error() == b"cf_perturbation_scan: null handle"


def test_windows_map_to_coordinates_and_rows_for_both_strands(tmp_path):
    from chromoformer_amd.attribution import scan_windows
    from chromoformer_amd.data import promoter_col0
    ds = so.scan_dataset(str(tmp_path), w_prom=39000)
    plus = [x for x in ds.target_genes if ds.genes[x]["tss"][2] == "+" and ds.genes[x]["pcres"]][0]
    minus = [x for x in ds.target_genes if ds.genes[x]["tss"][2] == "-" and ds.genes[x]["pcres"]][0]
    assert promoter_col0(ds) == 500
    for gid in (plus, minus):
        chrom, tss, strand = ds.genes[gid]["tss"]
        start = tss - 20000 + 500
        win = scan_windows(start, start + 39000, 2000, 1, 20)
        assert win.dtype == np.int64 and win.shape == (20, 2)
        assert win[0].tolist() == [start, start + 2000] and win[19].tolist() == [start + 38000, start + 39000]
        assert scan_windows(start, start + 39000, 2000, 3, 20)[18].tolist() == [start + 36000, start + 39000]
        base = so.dataset_batch(ds, [gid], torch.float64)
        # the definition: zero the raw samples of window g, bin; the rows that change are the rows the rule names
        for region, g in ((0, 0), (0, 19), (1, 0)):
            pert = so.batch_from_scaled_raw(ds, [gid], region, g, 1, range(F), 0.0, torch.float64)
            flip = region == 0 and strand == "-"
            for b in BINS:
                L = 40000 // b
                key, mk = ("promoter_feats", "promoter_pad_masks") if region == 0 else ("pcre_feats", "pcre_pad_masks")
                x0 = base[key][b].reshape(-1, L, F)[region - 1 if region else 0]
                x1 = pert[key][b].reshape(-1, L, F)[region - 1 if region else 0]
                row = so.centre_row(base[mk][b], 1 if region == 0 else 8, L)[region - 1 if region else 0]
                rowc = so.centre_row(base[mk][2000], 1 if region == 0 else 8, 20)[region - 1 if region else 0]
                q, n = so.extent(row)
                lo, hi = so.covered_rows(q, n, so.extent(rowc)[1], L // 20, g, 1, flip)
                changed = (x0 != x1).any(-1).nonzero().flatten().tolist()
                assert changed and set(changed) <= set(range(lo, hi)), (gid, region, g, b, changed, lo, hi)
                assert bool((x1[lo:hi] == 0).all())
        # the pCRE's windows: from its own start, the last one clipped to its end
        c, s, e = ds.genes[gid]["pcres"][0]
        n_win = -(-(e - s) // 2000)
        w = scan_windows(s, e, 2000, 1, n_win)
        assert w[0, 0] == s and w[-1, 1] == e and bool((w[:-1, 1] - w[:-1, 0] == 2000).all())
