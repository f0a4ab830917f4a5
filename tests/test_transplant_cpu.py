"""pCRE transplant screen, what runs without a GPU: the oracle's rule against the dataset built from edited metadata and against the
reference's golden logits; the library builders; freq / slot broadcasting and the Python-side refusals; the binding; CLI misuse."""
import ctypes as C
import os

import numpy as np
import pandas as pd
import pytest
import torch

from chromoformer_amd import _lib, predict
from chromoformer_amd import transplant as tp
from chromoformer_amd.data import ChromoformerDataset
from oracle import chromoformer_oracle as orc
from tests import scan_oracle as so
from tests import transplant_oracle as to
from tests.helpers import GOLDEN
from tests.transplant_cases import choose_cases, edited_meta, oracle_candidate

TOL = 1e-4
BINS = (2000, 500, 100)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """-> (dataset at w_prom = 39000, its metadata table, the golden cases): built once, shared, never written."""
    ds = so.scan_dataset(str(tmp_path_factory.mktemp("transplant")), w_prom=39000)
    return ds, pd.read_csv(os.path.join(ds.npy_dir, "meta.csv")), choose_cases(ds)


def _item(ds, table, gid):
    d = ChromoformerDataset(table, ds.npy_dir, [gid], w_prom=ds.w_prom)
    return torch.utils.data.default_collate([d[0]])


def test_golden_cases_are_the_ones_chosen_here(data):
    ds, table, cases = data
    z = np.load(os.path.join(GOLDEN, "transplant.npz"))
    assert int(z["w_prom"]) == 39000 and [str(s) for s in z["names"]] == [c[0] for c in cases]
    assert [str(s) for s in z["genes"]] == [c[1] for c in cases] and z["slots"].tolist() == [c[2] for c in cases]
    got = list(zip((str(s) for s in z["cand_chrom"]), z["cand_start"].tolist(), z["cand_end"].tolist()))
    assert got == [c[3] for c in cases] and z["freq"].tolist() == [c[4] for c in cases] and z["regression"].tolist() == [c[5] for c in cases]
    # what the cases are about: replace / append by partner count, a '-' strand gene, an 1,800-sample candidate
    n_part = {c[0]: len(ds.genes[c[1]]["pcres"]) for c in cases}
    slot = {c[0]: c[2] for c in cases}
    assert slot["replace"] < n_part["replace"] and n_part["append2"] == 2 == slot["append2"] and n_part["append0"] == 0 == slot["append0"]
    assert ds.genes[cases[3][1]]["tss"][2] == "-" and cases[4][3][2] - cases[4][3][1] == 1800 and z["clf"].shape == (5, 2, 2) and z["reg"].shape == (1, 2, 1)


def test_oracle_edit_is_the_dataset_item_of_the_edited_metadata_and_reproduces_the_golden(data):
    ds, table, cases = data
    z = np.load(os.path.join(GOLDEN, "transplant.npz"))
    at = {False: 0, True: 0}
    for name, gid, slot, cand, f, regression in cases:
        base, edit = _item(ds, table, gid), _item(ds, edited_meta(table, gid, slot, cand, f), gid)
        feats, cols = oracle_candidate(ds, cand)
        mine = to.transplant(base, 0, feats, cols, f, slot)
        for k in to.KEYS:
            pairs = [(mine[k][b], edit[k][b]) for b in edit[k]] if isinstance(edit[k], dict) else [(mine[k], edit[k])]
            assert all(a.dtype == b.dtype and torch.equal(a, b) for a, b in pairs), (name, k)
        if slot == len(ds.genes[gid]["pcres"]):
            assert to.append_slot(base, 0) == slot, name
        P = orc.init_params(None, 42, regression)
        with torch.no_grad():
            lg = torch.cat([orc.forward(P, base), orc.forward(P, mine)])
        gold = torch.from_numpy(z["reg" if regression else "clf"][at[regression]])
        at[regression] += 1
        d = (lg - gold).abs().max().item()
        print("%s: oracle vs golden %.2e (bound %.0e); effect %.2e" % (name, d, TOL, (gold[1] - gold[0]).abs().max().item()))
        assert d < TOL, (name, d)
        assert not torch.equal(gold[0], gold[1]), name
    assert torch.equal(to.transplant(base, 0, feats, cols, f, -1)["interaction_freq"], base["interaction_freq"])


def test_library_from_regions_is_the_datasets_own_binning(data):
    ds, table, cases = data
    gid = cases[3][1]                                      # a gene with partners
    parts = ds.genes[gid]["pcres"]
    lib = tp.library_from_regions(ds, [tuple(p) + ("enh%d" % i,) for i, p in enumerate(parts)] + [tuple(cases[4][3])])
    assert len(lib) == len(parts) + 1 and lib.names[:2] == ["enh0", "enh1"] and lib.names[-1] == "%s:%d-%d" % cases[4][3]
    assert lib.coords[0] == tuple(parts[0])
    reg = ds.regions(gid)
    for b in BINS:
        L = 40000 // b
        assert lib.feats[b].shape == (len(lib), L, 7) and lib.feats[b].dtype == torch.float32
        assert lib.mask_rows[b].shape == (len(lib), L) and lib.mask_rows[b].dtype == torch.uint8
        for i, (x, lo, n) in enumerate(reg[b][3]):
            assert torch.equal(lib.feats[b][i], x.t())
            row = torch.ones(L, dtype=torch.uint8)
            row[lo:lo + n] = 0
            assert torch.equal(lib.mask_rows[b][i], row)
    assert int((lib.mask_rows[2000][-1] == 0).sum()) == 1 and int((lib.mask_rows[100][-1] == 0).sum()) == 18      # 1,800 samples
    item = _item(ds, table, gid)                           # ... and equal to what the dataset puts in the slot, mask row included
    for b in BINS:
        L = 40000 // b
        assert torch.equal(item["pcre_feats"][b][0, :len(parts)], lib.feats[b][:len(parts)])
        assert torch.equal(item["pcre_pad_masks"][b][0, :len(parts), 0, L // 2].to(torch.uint8), lib.mask_rows[b][:len(parts)])
    with pytest.raises(ValueError, match="w_max"):
        tp.library_from_regions(ds, [("chr1", 0, 40001)])
    with pytest.raises(ValueError, match="at least 1"):
        tp.library_from_regions(ds, [])
    with pytest.raises(ValueError, match="chrom, start, end"):
        tp.library_from_regions(ds, [("chr1", 5)])


def test_library_from_batch_gathers_the_right_rows():
    batch = orc.synthetic_batch(3, seed=13, regime="realistic")
    pairs = [(2, 0), (0, 1), (2, 0), (1, 7)]
    lib = tp.library_from_batch(batch, pairs)
    assert len(lib) == 4 and lib.names == ["gene2:slot0", "gene0:slot1", "gene2:slot0", "gene1:slot7"] and lib.coords is None
    compact = dict(batch)
    compact["pcre_pad_masks"] = {b: batch["pcre_pad_masks"][b][:, :, 0, (40000 // b) // 2].to(torch.uint8) for b in BINS}
    lib2 = tp.library_from_batch(compact, pairs)
    for b in BINS:
        L = 40000 // b
        for c, (g, s) in enumerate(pairs):
            assert torch.equal(lib.feats[b][c], batch["pcre_feats"][b][g, s])
            assert torch.equal(lib.mask_rows[b][c], batch["pcre_pad_masks"][b][g, s, 0, L // 2].to(torch.uint8))
        assert torch.equal(lib2.feats[b], lib.feats[b]) and torch.equal(lib2.mask_rows[b], lib.mask_rows[b])
    sub = lib.select([3, 0])
    assert sub.names == ["gene1:slot7", "gene2:slot0"] and torch.equal(sub.feats[500][1], lib.feats[500][0])
    with pytest.raises(ValueError, match="outside"):
        tp.library_from_batch(batch, [(3, 0)])
    with pytest.raises(ValueError, match="outside"):
        tp.library_from_batch(batch, [(0, 8)])
    with pytest.raises(ValueError, match="at least 1"):
        tp.library_from_batch(batch, [])
    with pytest.raises(ValueError, match="names"):
        tp.Library(lib.feats, lib.mask_rows, names=["a"])
    with pytest.raises(ValueError, match="same bin sizes"):
        tp.Library(lib.feats, {2000: lib.mask_rows[2000]})


def test_freq_and_slot_broadcasting_and_refusals():
    B, Cn = 3, 4
    assert torch.equal(tp.broadcast_freq(2.5, B, Cn), torch.full((B, Cn, 1), 2.5))
    q = tp.broadcast_freq([1.0, 5.0], B, Cn)
    assert q.shape == (B, Cn, 2) and q.is_contiguous() and q.dtype == torch.float32 and bool((q == torch.tensor([1.0, 5.0])).all())
    cq = torch.arange(8.0).reshape(Cn, 2)
    assert torch.equal(tp.broadcast_freq(cq, B, Cn), cq[None].expand(B, Cn, 2))
    bcq = torch.arange(24.0).reshape(B, Cn, 2)
    assert torch.equal(tp.broadcast_freq(bcq, B, Cn), bcq)
    for bad, msg in ((torch.zeros(3, 2), "rows"), (torch.zeros(2, Cn, 2), "B = 3"), (torch.zeros(1, 1, 1, 1), "scalar"), ([1.0, float("nan")], "finite"),
                     (torch.zeros(0), "Q >= 1")):
        with pytest.raises(ValueError, match=msg):
            tp.broadcast_freq(bad, B, Cn)
    assert tp.slot_argument("append", B, 8) == (-1, None) and tp.slot_argument(5, B, 8) == (5, None)
    all_, per = tp.slot_argument([2, -1, 7], B, 8)
    assert per.dtype == torch.int32 and per.tolist() == [2, -1, 7]
    for bad, msg in (("prepend", "append"), (8, "outside"), (-1, "outside"), ([0, 1], "one per gene"), ([0, 1, 8], "-1, i_max"), ([0, 1, -2], "-1, i_max"),
                     ([0.0, 1.0, 2.0], "one per gene")):
        with pytest.raises(ValueError, match=msg):
            tp.slot_argument(bad, B, 8)

    class NoDevice:      # what pcre_transplant reads of a model before it asks for the device
        binsizes, n_bins, n_feats, i_max = [2000, 500, 100], [20, 80, 400], 7, 8

    lib = tp.library_from_batch(orc.synthetic_batch(1, seed=3, regime="realistic"), [(0, 0)])
    with pytest.raises(ValueError, match="Library"):
        tp.pcre_transplant(NoDevice(), None, library=None)
    NoDevice.n_bins = [20, 80, 200]
    with pytest.raises(ValueError, match=r"feats\[100\]"):
        tp.pcre_transplant(NoDevice(), None, library=lib)
    NoDevice.binsizes = [2000, 500]
    with pytest.raises(ValueError, match="bin sizes"):
        tp.pcre_transplant(NoDevice(), None, library=lib)


def test_binding_symbol_arguments_and_struct():
    res, args = _lib.SYMBOLS["cf_pcre_transplant"]
    assert res is C.c_int and len(args) == 5 and args[1] == C.POINTER(_lib.cf_batch) and args[2] == C.POINTER(_lib.cf_transplant_opts)
    fields = [(n, t) for n, t in _lib.cf_transplant_opts._fields_]
    assert [n for n, _ in fields] == ["n_cand", "n_freq", "lib_feats", "lib_mask", "freq", "slot", "slot_all", "slot_out"]
    assert fields[2][1] is C.c_void_p * _lib.MAX_RES and fields[3][1] is C.c_void_p * _lib.MAX_RES and fields[6][1] is C.c_int
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "chromoformer_hip.h")).read()
    assert "int cf_pcre_transplant(cf_handle* h, const cf_batch* batch, const cf_transplant_opts* opts, float* logits, void* stream);" in header
    assert "#define CF_ABI_VERSION 1\n" in header and "} cf_transplant_opts;" in header


def test_cli_misuse_exits_2(tmp_path, capsys):
    bed = tmp_path / "c.bed"
    bed.write_text("# candidates\nchr1\t100\t2000\tfirst\nchr2 5 900\n")
    assert tp.read_bed(str(bed)) == [("chr1", 100, 2000, "first"), ("chr2", 5, 900)]
    bad = tmp_path / "bad.bed"
    bad.write_text("chr1\tx\t2000\n")
    empty = tmp_path / "empty.bed"
    empty.write_text("# nothing\n")
    base = ["-m", "m.csv", "-d", "npy", "-o", str(tmp_path / "p.csv")]
    out = str(tmp_path / "t.npz")
    cases = [(["--transplant-bed", str(bed)], "--transplant-bed needs --transplant-out"),
             (["--transplant-out", out], "--transplant-out needs --transplant-bed"),
             (["--transplant-freq", "1,5"], "need --transplant-out"),
             (["--transplant-slot", "3"], "need --transplant-out"),
             (["--transplant-bed", str(bed), "--transplant-out", out, "--transplant-freq", "1,x"], "--transplant-freq"),
             (["--transplant-bed", str(bed), "--transplant-out", out, "--transplant-freq", "1,inf"], "--transplant-freq"),
             (["--transplant-bed", str(bed), "--transplant-out", out, "--transplant-slot", "8"], "--transplant-slot"),
             (["--transplant-bed", str(bed), "--transplant-out", out, "--transplant-slot", "last"], "--transplant-slot"),
             (["--transplant-bed", str(bad), "--transplant-out", out], "chrom start end"),
             (["--transplant-bed", str(empty), "--transplant-out", out], "no region"),
             (["--transplant-bed", str(tmp_path / "missing.bed"), "--transplant-out", out], "--transplant-bed")]
    for extra, msg in cases:
        with pytest.raises(SystemExit) as e:
            predict.main(base + extra)
        assert e.value.code == 2 and msg in capsys.readouterr().err, extra
    assert not os.path.exists(out)
    a = predict.build_parser().parse_args(base + ["--transplant-bed", str(bed), "--transplant-out", out, "--transplant-freq", "1,5,10", "--transplant-slot", "append"])
    assert (a.transplant_bed, a.transplant_out, a.transplant_freq, a.transplant_slot) == (str(bed), out, "1,5,10", "append")
    assert predict.build_parser().parse_args(base).transplant_out is None
