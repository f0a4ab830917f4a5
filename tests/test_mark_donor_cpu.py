"""Histone-mark coalitions against a donor cell type, host side (no GPU): the C ABI declares, exports and mirrors the three entry points
and their options struct; the methods and the CLI options are offered; the oracle reproduces the reference's logits on raw files
whose rows were replaced by the donor's (golden); selecting binned features equals binning the replaced raw rows, bit for bit;
attribution.same_regions accepts the pair and refuses other regions and another geometry by name."""
import copy
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from chromoformer_amd import _lib
from chromoformer_amd.attribution import mark_players, same_regions
from oracle import chromoformer_oracle as orc
from tests import donor_oracle as do
from tests import mark_oracle as mo
from tests import scan_oracle as so
from tests.helpers import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINS = (2000, 500, 100)
GENES = ["ENSGSYN00001", "ENSGSYN00000", "ENSGSYN00002"]
TOL = 1e-4      # the project's logit bound
OVERLAP = [((0, 1), (0, 1)), ((1, 2), (0, 2))]
NAMES = ("cf_mark_donor_coalitions", "cf_mark_donor_shapley", "cf_mark_donor_epistasis")


def test_the_entry_points_are_declared_bound_and_offered():
    hdr = open(os.path.join(ROOT, "include", "chromoformer_hip.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert ("int cf_mark_donor_coalitions(cf_handle* h, const cf_batch* batch, const cf_mark_donor_opts* opts, const uint32_t* keep, int n_coal, "
            "float* logits, void* stream);") in flat
    assert "int cf_mark_donor_shapley(cf_handle* h, const cf_batch* batch, const cf_mark_donor_opts* opts, float* phi, float* logits_all, void* stream);" in flat
    assert "int cf_mark_donor_epistasis(cf_handle* h, const cf_batch* batch, const cf_mark_donor_opts* opts, float* eps, float* logits_pairs, void* stream);" in flat
    assert set(NAMES) <= set(_lib.SYMBOLS)
    assert "#define CF_ABI_VERSION 1" in hdr
    # int n_players; (pad) const unsigned*; const unsigned*; const float* [3]; const float* [3]
    o = _lib.cf_mark_donor_opts
    assert C.sizeof(o) == 72
    assert [o.n_players.offset, o.player_marks.offset, o.player_regions.offset, o.donor_promoter_feats.offset, o.donor_pcre_feats.offset] == [0, 8, 16, 24, 48]
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct cf_mark_donor_opts \{(.*?)\} cf_mark_donor_opts;", hdr, re.S).group(1), flags=re.S)
    assert re.findall(r"(\w+)(?:\[CF_MAX_RES\])?;", body) == [n for n, _ in o._fields_]
    assert C.sizeof(_lib.cf_mark_opts) == 32      # the scale family's struct is left as it is
    for name in NAMES:
        res, args = _lib.SYMBOLS[name]
        assert res is C.c_int and args[1] == C.POINTER(_lib.cf_batch) and args[2] == C.POINTER(o), name
    L = _lib.lib()
    for name in NAMES:
        assert hasattr(L, name), name
    assert L.cf_mark_donor_coalitions(None, None, None, None, 0, None, None) != 0
    assert L.cf_last_error() == b"cf_mark_donor_coalitions: null handle"
    assert L.cf_mark_donor_shapley(None, None, None, None, None, None) != 0 and L.cf_last_error() == b"cf_mark_donor_shapley: null handle"
    assert L.cf_mark_donor_epistasis(None, None, None, None, None, None) != 0 and L.cf_last_error() == b"cf_mark_donor_epistasis: null handle"
    from chromoformer_amd import ChromoformerRegressor
    from chromoformer_amd.net import Chromoformer
    for name in ("mark_donor_coalitions", "mark_donor_shapley", "mark_donor_epistasis", "mark_donor_shapley_dataset"):
        assert getattr(Chromoformer, name) is getattr(ChromoformerRegressor, name)
    out = subprocess.run([sys.executable, "-m", "chromoformer_amd.predict", "--help"], cwd=ROOT, capture_output=True, text=True,
                         check=True).stdout
    for opt in ("--donor-npy-dir", "--donor-meta", "--donor-store", "--mark-donor-shapley-out", "--mark-donor-epistasis-out", "--mark-players"):
        assert opt in out, opt


def test_a_donor_output_without_the_donor_signals_is_a_parser_error(tmp_path):
    from chromoformer_amd import predict
    for flag in ("--mark-donor-shapley-out", "--mark-donor-epistasis-out"):
        with pytest.raises(SystemExit) as e:
            predict.main(["-m", str(tmp_path / "meta.csv"), "-d", str(tmp_path), "-o", str(tmp_path / "p.csv"), flag, str(tmp_path / "out")])
        assert e.value.code == 2
    with pytest.raises(SystemExit) as e:      # ... and donor signals nobody reads
        predict.main(["-m", str(tmp_path / "meta.csv"), "-d", str(tmp_path), "-o", str(tmp_path / "p.csv"), "--donor-npy-dir", str(tmp_path)])
    assert e.value.code == 2


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """-> (dataset, donor dataset, the three genes' batch, the donor's batch): built once, shared, never written."""
    ds = so.scan_dataset(str(tmp_path_factory.mktemp("marks")), w_prom=39000)
    dn = do.donor_dataset(ds.npy_dir, str(tmp_path_factory.mktemp("donor")), do.DONOR_SEED, w_prom=39000)
    return ds, dn, so.dataset_batch(ds, GENES), so.dataset_batch(dn, GENES)


def test_the_donor_dataset_is_another_cell_type_over_the_same_regions(data):
    ds, dn, batch, donor = data
    names = sorted(n for n in os.listdir(ds.npy_dir) if n.endswith(".npy"))
    assert names == sorted(n for n in os.listdir(dn.npy_dir) if n.endswith(".npy")) and len(names) > 20
    for n in names[:12]:
        a, d = np.load(os.path.join(ds.npy_dir, n)), np.load(os.path.join(dn.npy_dir, n))
        assert a.shape == d.shape and d.dtype == np.float16 and (d >= 0).all() and all((a[f] != d[f]).any() for f in range(7)), n
    again = np.load(os.path.join(dn.npy_dir, names[0])).copy()      # deterministic
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        do.donor_dataset(ds.npy_dir, tmp, do.DONOR_SEED)
        assert np.array_equal(np.load(os.path.join(tmp, names[0])), again)
    for key in ("promoter_pad_masks", "pcre_pad_masks", "interaction_masks"):
        assert all(torch.equal(batch[key][b], donor[key][b]) for b in BINS)
    assert all(not torch.equal(batch["promoter_feats"][b], donor["promoter_feats"][b]) for b in BINS)


def test_selecting_binned_features_equals_binning_the_replaced_raw_rows(data):
    """donor_rows (a copy of the donor's binned elements) against the from-raw oracle (the absent marks' rows of every raw region
    replaced by the donor's, binned by the dataset's own code): bit for bit at every resolution, on a '-' strand promoter narrowed
    to 39000 and a 1,800-sample pCRE -- binning works per mark."""
    ds, dn, batch, donor = data
    assert ds.w_prom == 39000 and ds.genes[GENES[0]]["tss"][2] == "-"
    c, s, e = ds.genes[GENES[1]]["pcres"][0]
    assert e - s == 1800 and not ds.genes[GENES[2]]["pcres"]
    cases = [("marks", 0x7F & ~0x12), ("marks", 0x00), ("compartments", 0x3FFF & ~(1 << 1) & ~(1 << 11)), ("regions", 0x1FF & ~0b11), (OVERLAP, 0b00)]
    for spec, word in cases:
        marks, regions, _ = mark_players(spec, 7, 8)
        gone = mo.gone_words(marks, regions, word, 9)
        assert any(gone)
        ref = do.batch_from_replaced_regions(ds, dn.npy_dir, GENES, gone)
        got = do.donor_rows(batch, donor, (marks, regions), [word])
        for b in BINS:
            for key in ("promoter_feats", "pcre_feats", "promoter_pad_masks", "pcre_pad_masks", "interaction_masks"):
                assert torch.equal(got[key][b], ref[key][b]), (spec, hex(word), b, key)
            for f in range(7):      # an absent mark carries the donor's bits, a present one the gene's
                src = donor if gone[0] >> f & 1 else batch
                assert torch.equal(got["promoter_feats"][b][..., f], src["promoter_feats"][b][..., f])
                for j in range(8):
                    src = donor if gone[1 + j] >> f & 1 else batch
                    assert torch.equal(got["pcre_feats"][b][:, j, :, f], src["pcre_feats"][b][:, j, :, f])
        assert torch.equal(got["interaction_freq"], ref["interaction_freq"]) and torch.equal(got["interaction_freq"], batch["interaction_freq"])
    # the full word is the gene's own batch; with the seven marks as players word 0 is the donor's features under the gene's masks
    marks, regions, _ = mark_players("marks", 7, 8)
    got = do.donor_rows(batch, donor, (marks, regions), [0x7F, 0x00])
    for b in BINS:
        assert torch.equal(got["promoter_feats"][b][0::2], batch["promoter_feats"][b]) and torch.equal(got["pcre_feats"][b][1::2], donor["pcre_feats"][b])


def test_the_select_passes_nan_payloads_negative_zero_and_inf(data):
    ds, dn, batch, donor = data
    odd = copy.deepcopy(donor)
    bits = torch.tensor([0x7FC12345, 0x80000000, 0x7F800000, 0xFF800000 - (1 << 32), 0x7F812345], dtype=torch.int64).to(torch.int32)
    t = odd["promoter_feats"][2000]
    t.view(torch.int32).reshape(-1)[:5] = bits
    marks, regions, _ = mark_players("marks", 7, 8)
    got = do.donor_rows(batch, odd, (marks, regions), [0x00])
    assert torch.equal(got["promoter_feats"][2000].view(torch.int32), t.view(torch.int32))


def test_oracle_logits_equal_the_golden(data):
    """The reference's own dataset and model on raw files with the donor's rows (tests/golden/make_mark_donor_goldens.py) against the
    select + orc.forward on the two datasets' batches."""
    ds, dn, batch, donor = data
    g = np.load(os.path.join(GOLDEN, "mark_donor.npz"))
    assert [str(x) for x in g["genes"]] == GENES and int(g["w_prom"]) == 39000 and int(g["donor_seed"]) == do.DONOR_SEED and len(g["words"]) == 6
    assert os.path.getsize(os.path.join(GOLDEN, "mark_donor.npz")) < 16384
    for head, regression in (("clf", False), ("reg", True)):
        P = orc.init_params(None, 42, regression)
        assert g[head].shape == (6, 3, 1 if regression else 2) and g[head].dtype == np.float32
        for k in range(len(g["words"])):
            n = int(g["n_players"][k])
            players = (g["player_marks"][k][:n], g["player_regions"][k][:n])
            lg = do.oracle_donor_coalitions(P, batch, donor, players, [int(g["words"][k]), (1 << n) - 1])
            d = (lg[:, 0] - torch.from_numpy(g[head][k])).abs().max().item()
            d0 = (lg[:, 1] - torch.from_numpy(g["base." + head])).abs().max().item()
            print(head, "case", k, "oracle vs reference %.2e, unperturbed %.2e" % (d, d0))
            assert d < TOL and d0 < TOL, (head, k, d, d0)
            assert (g[head][k] != g["base." + head]).any()


def test_same_regions_accepts_the_pair_and_refuses_by_name(data, tmp_path):
    import pandas as pd

    from chromoformer_amd.data import ChromoformerDataset
    ds, dn, batch, donor = data
    assert same_regions(ds, dn) == ds.target_genes and same_regions(ds, dn, GENES) == GENES
    # one pCRE dropped from one gene of the donor's metadata
    table = pd.read_csv(os.path.join(dn.npy_dir, "meta.csv"))
    row = table.index[table.gene_id == GENES[0]][0]
    assert len(table.loc[row, "neighbors"].split(";")) > 1
    table.loc[row, "neighbors"] = ";".join(table.loc[row, "neighbors"].split(";")[1:])
    table.loc[row, "scores"] = ";".join(str(table.loc[row, "scores"]).split(";")[1:])
    short = ChromoformerDataset(table, dn.npy_dir, table.gene_id.tolist(), w_prom=39000)
    with pytest.raises(ValueError, match=r"same_regions: 1 gene\(s\).*%s \(pcres\)" % GENES[0]):
        same_regions(ds, short)
    assert same_regions(ds, short, GENES[1:]) == GENES[1:]      # the other genes agree
    # another strand, another TSS: up to five genes are listed
    moved = pd.read_csv(os.path.join(dn.npy_dir, "meta.csv"))
    moved["start"] = moved["start"] + 100
    far = ChromoformerDataset(moved, dn.npy_dir, moved.gene_id.tolist(), w_prom=39000)
    with pytest.raises(ValueError, match=r"same_regions: 20 gene\(s\)") as e:
        same_regions(ds, far)
    assert str(e.value).count("(tss)") == 5 and str(e.value).endswith("...")
    # another geometry, by name
    narrow = ChromoformerDataset(os.path.join(dn.npy_dir, "meta.csv"), dn.npy_dir, dn.target_genes, w_prom=38000)
    with pytest.raises(ValueError, match="same_regions: .*w_prom 39000 != 38000"):
        same_regions(ds, narrow)
    other = ChromoformerDataset(os.path.join(dn.npy_dir, "meta.csv"), dn.npy_dir, dn.target_genes, i_max=4, binsizes=[2000, 500], w_prom=39000)
    with pytest.raises(ValueError, match="binsizes.*i_max 8 != 4"):
        same_regions(ds, other)
    with pytest.raises(ValueError, match="not in both"):
        same_regions(ds, dn, ["ENSGSYN99999"])
