"""The fine window game, host side (no GPU): the rule of include/chromoformer_hip.h (tests/fine_window_oracle.fine_window_region,
evaluated in fp32 as the kernels do) equals binning the raw signal edited inside the absent players' windows, for the scale rule and
against a donor; one absent player is the fine scan's rule bit for bit; attribution.fine_window_players; the golden from the reference;
the C ABI declares, exports and mirrors the three cf_mark_fine_* calls.

Tolerances.  A wholly covered or untouched element: WHOLE_TOL of tests/test_fine_scan_cpu.py.  A partly covered element is rebuilt from
rounded fp32 features, m' = m_j + (s - 1) S / cnt_j (the donor rule: m_j + D / cnt_j), and a relative error eps in each term becomes
eps x (the sum of the terms' magnitudes) / (1 + m') in u' = log(1 + m'): the bound is FINE_PART_C 2^-24 ((1 + m_j) + X) / (1 + m'), X = 0
under the scale rule and the sum over C of cnt_k (|expm1 d_k| + |expm1 u_k|) / cnt_j under the donor rule."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from chromoformer_amd import _lib
from chromoformer_amd import attribution as at
from tests import fine_scan_oracle as fo
from tests import fine_window_oracle as fw
from tests import scan_oracle as so
from tests.test_fine_scan_cpu import WHOLE_TOL
from tests.test_perturbation_scan_cpu import BINS, NB, F, _binned, _raw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = tuple(range(F))
#: twice the worst |u' - from raw| / (2^-24 ((1 + m_j) + X) / (1 + m')) observed over every case of this file against the from-raw
#: definition: 7.434 (the scale rule at length 40000; 7.203 in the dataset test, 7.017 at length 7300, at most 5.36 at the other
#: lengths; the donor rule's worst is 3.204, its X widens the bound).  As for PART_C of tests/test_fine_scan_cpu.py the large ratios
#: belong to s = 2.5, where (1 + m_j) / (1 + m') < 1 shrinks the bound below the ulp of the result.
FINE_PART_C = 14.87
SCALES = (0.0, 0.5, 2.5)
LENGTHS = [1999, 2001, 7300, 12345, 39901, 40000]

#: windows relative to `start`: different mark sets, overlaps (0/1, 2/3, 3/4), boundaries of 500 bp and 2 kb inside, one long window
PLAYERS = [((1, 4), (0, 7)), ((0, 1, 2), (5, 12)), (ALL, (18, 23)), ((3,), (19, 61)), ((3, 4, 5, 6), (40, 44)), ((2, 5), (25, 33))]
#: absent sets: everybody, pairs that overlap, players apart, nobody
ABSENT = [(0, 1, 2, 3, 4, 5), (0, 1), (2, 3), (1, 3, 4), (5,), ()]


def _present(absent):
    return [p not in absent for p in range(len(PLAYERS))]


def _starts(nf):
    return sorted({0, 2, max(nf - 31, 0)})


def _check(src, masks, raw, strand, window, length, stats, donor=None, donor_raw=None, scales=SCALES):
    """Every start, absent set and scale (or the donor) on one region: the fp32 rule against the from-raw definition."""
    nf = so.extent(masks[100])[1]
    for start in _starts(nf):
        for absent in ABSENT:
            for s in scales:
                got, kinds, extra = fw.fine_window_region(src, masks, BINS, PLAYERS, _present(absent), start, s, strand != "+", length, donor)
                ref = fw.region_from_edited_raw(raw, BINS, NB, PLAYERS, _present(absent), start, s, strand, window, donor_raw)
                for b in BINS:
                    assert not torch.isnan(got[b]).any() and not torch.isnan(ref[b]).any()
                    err = (got[b].double() - ref[b].double()).abs()
                    part = kinds[b] == fw.PART
                    fac = fw.bound_factor(src[b], got[b], kinds[b], extra[b])
                    if not absent:
                        assert torch.equal(got[b], src[b])
                    if b == 100:
                        assert not part.any()
                    stats["whole"] = max(stats["whole"], err[~part].max().item())
                    if part.any():
                        stats["n_part"] += int(part.sum())
                        stats["rows"] = max(stats["rows"], int(part.any(1).sum()))
                        stats["mixed"] += int(((kinds[b] != kinds[b][:, :1]).any(1)).sum())
                        stats["ratio"] = max(stats["ratio"], (err[part] / (2.0 ** -24 * fac[part])).max().item())
                    assert err[~part].max().item() <= WHOLE_TOL, (start, absent, s, b, err[~part].max().item())
                    assert bool((err <= torch.where(part, FINE_PART_C * 2.0 ** -24 * fac, torch.full_like(fac, WHOLE_TOL))).all()), (start, absent, s, b)


def _stats():
    return dict(whole=0.0, ratio=0.0, n_part=0, rows=0, mixed=0)


@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("strand", ["+", "-"])
def test_scale_rule_equals_binning_the_edited_signal(length, strand):
    raw = _raw(length, length)
    base = _binned(raw, strand, None)
    src = {b: base["promoter_feats"][b][0, 0] for b in BINS}
    masks = {b: base["promoter_pad_masks"][b][0] for b in BINS}
    stats = _stats()
    _check(src, masks, raw, strand, None, length, stats)
    print("scale, length %d strand %s: whole %.3e, partial ratio %.3f over %d partly covered elements (%d rows at once, %d rows with C "
          "differing between marks)" % (length, strand, stats["whole"], stats["ratio"], stats["n_part"], stats["rows"], stats["mixed"]))
    assert stats["rows"] > 2 and stats["mixed"]      # more partly covered bins at once than a scan's two, C differing between marks


@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("strand", ["+", "-"])
def test_donor_rule_equals_binning_the_edited_signal(length, strand):
    raw, draw = _raw(length, length), _raw(length, length + 1)
    base, dbase = _binned(raw, strand, None), _binned(draw, strand, None)
    src = {b: base["promoter_feats"][b][0, 0] for b in BINS}
    don = {b: dbase["promoter_feats"][b][0, 0] for b in BINS}
    masks = {b: base["promoter_pad_masks"][b][0] for b in BINS}
    stats = _stats()
    _check(src, masks, raw, strand, None, length, stats, don, draw, scales=(0.0,))
    print("donor, length %d strand %s: whole %.3e, partial ratio %.3f over %d partly covered elements" % (length, strand, stats["whole"], stats["ratio"],
                                                                                                         stats["n_part"]))
    assert stats["rows"] > 2 and stats["mixed"]
    # a donor that agrees with the gene inside the windows changes no bit: null players
    got, kinds, _ = fw.fine_window_region(src, masks, BINS, PLAYERS, _present(ABSENT[0]), 2, 0.0, strand != "+", length, src)
    assert all(torch.equal(got[b], src[b]) for b in BINS) and not any((kinds[b] == fw.PART).any() for b in BINS)


def test_rule_on_a_dataset_the_narrowed_mirrored_promoter_and_pcre_tails(tmp_path):
    ds = so.scan_dataset(str(tmp_path), w_prom=39000)
    minus = [x for x in ds.target_genes if ds.genes[x]["tss"][2] == "-" and ds.genes[x]["pcres"]][0]
    plus = [x for x in ds.target_genes if ds.genes[x]["tss"][2] == "+" and ds.genes[x]["pcres"]][0]
    stats = _stats()
    for gid in (minus, plus):
        chrom, tss, strand = ds.genes[gid]["tss"]
        batch = so.dataset_batch(ds, [gid])
        raw = ds._load(chrom, tss - 20000, tss + 20000)
        src = {b: batch["promoter_feats"][b][0, 0] for b in BINS}
        masks = {b: so.centre_row(batch["promoter_pad_masks"][b], 1, 40000 // b)[0] for b in BINS}
        _check(src, masks, raw, strand, 39000, 39000, stats, scales=(0.0, 2.5))
        c, s, e = ds.genes[gid]["pcres"][0]
        src = {b: batch["pcre_feats"][b][0, 0] for b in BINS}
        masks = {b: so.centre_row(batch["pcre_pad_masks"][b], 8, 40000 // b)[0] for b in BINS}
        _check(src, masks, ds._load(c, s, e), "+", None, e - s, stats, scales=(0.0, 2.5))
    print("dataset: whole %.3e, partial ratio %.3f over %d partly covered elements" % (stats["whole"], stats["ratio"], stats["n_part"]))
    assert stats["n_part"] > 20


def test_one_absent_player_is_the_fine_scan_bit_for_bit():
    raw = _raw(12345, 3)
    base = _binned(raw, "-", None)
    for marks, (lo, hi), start in (((1, 4), (0, 7), 95), (ALL, (3, 4), 0), ((0,), (5, 40), 100), ((2,), (0, 3), 200)):
        for s in SCALES:
            a, _, ka = fo.fine_rows(base, scale=s, width=hi - lo, start=start + lo, n_windows=1, mark_sets=[marks], lengths=[12345], flip=[True])
            b, _, kb, _ = fw.fine_window_rows(base, [(marks, (lo, hi))], [[True], [False]], start=start, lengths=[12345], flip=[True], scale=s)
            for bs in BINS:
                assert torch.equal(a[bs], b[bs]), (marks, lo, hi, start, s, bs)
                assert torch.equal(ka[bs][0, 1] != 0, (kb[bs][0, 1] != 0).any(-1))


def test_overlapping_absent_players_change_an_element_once():
    raw = _raw(7300, 5)
    base = _binned(raw, "+", None)
    two = [((1, 4), (0, 30)), ((1, 2), (10, 50))]
    one = [((1, 4), (0, 30)), ((1, 2), (10, 50)), ((1,), (0, 50)), ((4,), (0, 30)), ((2,), (10, 50))]
    a, _, _, _ = fw.fine_window_rows(base, two, [[False, False]], scale=0.5)
    b, _, _, _ = fw.fine_window_rows(base, one, [[True, True, False, False, False]], scale=0.5)
    assert all(torch.equal(a[bs], b[bs]) for bs in BINS)


def test_fine_window_players():
    marks, lo, hi, names = at.fine_window_players("windows", 7, 2, 10)
    assert marks.dtype == np.uint32 and lo.dtype == hi.dtype == np.int32
    assert marks.tolist() == [127] * 10 and lo.tolist() == list(range(0, 20, 2)) and hi.tolist() == list(range(2, 22, 2))
    assert names[0] == "fine[0:2]" and names[9] == "fine[18:20]"
    marks, lo, hi, names = at.fine_window_players("cells", 7, 2, 10)
    assert len(marks) == 70 and marks[:8].tolist() == [1, 2, 4, 8, 16, 32, 64, 1] and lo[:8].tolist() == [0] * 7 + [2] and hi[69] == 20
    assert names[8] == "mark1@fine[2:4]" and len(set(names)) == 70
    marks, lo, hi, names = at.fine_window_players([((0, 1), (3, 9)), ([6], (0, 2 ** 31 - 1))], 7)
    assert marks.tolist() == [3, 64] and lo.tolist() == [3, 0] and hi.tolist() == [9, 2 ** 31 - 1] and names[0] == "marks(0,1)@fine[3:9]"
    assert len(at.fine_window_players("windows", 7, 1, 128)[0]) == 128
    for bad, msg in ((("windows", 7, 1, 129), "129 players"), (("cells", 7, 1, 19), "133 players"), (("stretches", 7, 1, 4), "choose from"),
                     (("windows", 7, 0, 4), "width = 0"), (("windows", 7, 1, 0), "n_windows = 0"), (([((7,), (0, 1))], 7), "mark"),
                     (([((), (0, 1))], 7), "empty"), (([((0,), (3, 3))], 7), "window [3, 3)"), (([((0,), (-1, 3))], 7), "window [-1, 3)"),
                     (([((0,), (0, 1))] * 129, 7), "129 players"), (([(0, 1)], 7), "pairs")):
        with pytest.raises(ValueError, match="fine_window_players") as e:
            at.fine_window_players(*bad)
        assert msg in str(e.value), (bad, str(e.value))


def test_oracle_logits_equal_the_golden(tmp_path):
    """The reference's own dataset and models on raw files edited inside fine windows (tests/golden/make_fine_window_goldens.py) against
    the rule + orc.forward on the unedited dataset: the project's 1e-4."""
    from oracle import chromoformer_oracle as orc
    from tests import donor_oracle as do
    from tests.helpers import GOLDEN
    g = np.load(os.path.join(GOLDEN, "fine_window.npz"))
    ds = so.scan_dataset(str(tmp_path / "a"), w_prom=int(g["w_prom"]))
    genes = [str(x) for x in g["genes"]]
    base = so.dataset_batch(ds, genes)
    donor = so.dataset_batch(do.donor_dataset(ds.npy_dir, str(tmp_path / "d"), int(g["donor_seed"]), w_prom=int(g["w_prom"])), genes)
    flips = [ds.genes[x]["tss"][2] != "+" for x in genes]
    n_cases = len(g["scales"])
    assert n_cases == 6 and bool(g["donor"].any())
    for head, regression in (("clf", False), ("reg", True)):
        P = orc.init_params(None, 42, regression)
        for k in range(n_cases):
            players, present, region, start = golden_case(g, k)
            assert k != 1 or sum(not p for p in present) >= 2
            lg, _, kinds, _ = fw.oracle_fine_window(P, base, players, [present], region=region, start=start, lengths=g["lengths"][k].tolist(),
                                                    flip=flips if region == 0 else None, scale=float(g["scales"][k]),
                                                    donor=donor if g["donor"][k] else None)
            d = (lg[:, 0] - torch.from_numpy(g[head][k])).abs().max().item()
            print(head, "case", k, "oracle vs reference %.2e" % d)
            assert d < 1e-4, (head, k, d)


def golden_case(g, k):
    """Case k of tests/golden/fine_window.npz -> (players, present, region, start [B])."""
    rows = [r for r in g["players"].tolist() if r[0] == k]
    players = [(tuple(f for f in range(F) if r[1] >> f & 1), (r[2], r[3])) for r in rows]
    return players, [bool(r[4]) for r in rows], int(g["regions"][k]), g["starts"][k].tolist()


def test_abi_symbols_struct_and_null_handle():
    hdr = open(os.path.join(ROOT, "include", "chromoformer_hip.h")).read()
    for name in ("cf_mark_fine_coalitions", "cf_mark_fine_shapley", "cf_mark_fine_shapley_sampled"):
        assert re.search(r"int %s\(cf_handle\* h, const cf_batch\* batch, const cf_mark_fine_opts\* opts," % name, hdr) and name in _lib.SYMBOLS
    o = _lib.cf_mark_fine_opts
    # int region, n_players; 6 pointers; float scale (+ pad); three pointer arrays
    assert C.sizeof(o) == 8 + 6 * 8 + 8 + 3 * 8 * _lib.MAX_RES
    assert [o.region.offset, o.n_players.offset, o.player_marks.offset, o.player_lo.offset, o.player_hi.offset, o.start.offset, o.lengths.offset,
            o.flip.offset, o.scale.offset, o.donor_promoter_feats.offset] == [0, 4, 8, 16, 24, 32, 40, 48, 56, 64]
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct cf_mark_fine_opts \{(.*?)\} cf_mark_fine_opts;", hdr, re.S).group(1), flags=re.S)
    assert re.findall(r"(\w+)(?:\[CF_MAX_RES\])?[;,]", body) == [n for n, _ in o._fields_]
    assert C.sizeof(_lib.cf_mark_window_opts) == 104 and C.sizeof(_lib.cf_scan_fine_opts) == 88      # the existing structs keep their sizes
    L = _lib.lib()
    assert L.cf_abi_version() == 1
    assert L.cf_mark_fine_coalitions(None, None, None, None, 0, None, None) != 0
    assert L.cf_last_error() == b"cf_mark_fine_coalitions: null handle"
    assert L.cf_mark_fine_shapley(None, None, None, None, None, None) != 0
    assert L.cf_last_error() == b"cf_mark_fine_shapley: null handle"
    assert L.cf_mark_fine_shapley_sampled(None, None, None, None, 1, None, None, None, None) != 0
    assert L.cf_last_error() == b"cf_mark_fine_shapley_sampled: null handle"
