"""Raw-signal saliency, host side: the job record and symbol of cf_bin_regions_multi_backward, the closed form of the binning
backward (tests/raw_grad_oracle.py) against fp64 autograd through ChromoformerDataset.regions on a synthetic dataset (both strands,
a gene without partners, partial last bins, w_prom 40000 and 10000), the predict options and the error for missing raw signals."""
import ctypes as C
import os

import numpy as np
import pandas as pd
import pytest
import torch

from tests.raw_grad_oracle import closed_form, make_small_dataset
from tests.synth_data import make_dataset


def test_grad_job_record_matches_the_c_struct():
    from chromoformer_amd.data import BIN_GRAD_JOB
    assert BIN_GRAD_JOB.itemsize == 72
    assert BIN_GRAD_JOB.fields["dfeat"][1] == 32 and BIN_GRAD_JOB.fields["draw"][1] == 56 and BIN_GRAD_JOB.fields["ld_out"][1] == 64


def test_symbol_is_declared_and_exported():
    from chromoformer_amd import _lib
    assert "cf_bin_regions_multi_backward" in _lib.SYMBOLS
    res, args = _lib.SYMBOLS["cf_bin_regions_multi_backward"]
    assert res is C.c_int and len(args) == 9
    fn = _lib.lib().cf_bin_regions_multi_backward
    assert len(fn.argtypes) == 9
    assert _lib.lib().cf_abi_version() == 1


@pytest.mark.parametrize("w_prom", [40000, 10000])
def test_closed_form_equals_fp64_autograd_through_the_dataset(tmp_path, w_prom):
    from chromoformer_amd.data import ChromoformerDataset, load_raw_regions, raw_window
    meta, _ = make_small_dataset(str(tmp_path / "npy"))
    table = pd.read_csv(meta)
    genes = table.gene_id.tolist()
    assert set(table.strand) == {"+", "-"} and bool(table.neighbors.isna().any()), "both strands and a gene without partners"
    ds = ChromoformerDataset(meta, str(tmp_path / "npy"), genes, w_prom=w_prom)
    leaves = {}

    def load(chrom, start, end):      # fp64 leaves instead of the fp16 arrays
        key = (chrom, start, end)
        if key not in leaves:
            a = np.load("%s/%s:%d-%d.npy" % (ds.npy_dir, chrom, start, end))
            leaves[key] = torch.from_numpy(a.astype(np.float64)).requires_grad_(True)
        return leaves[key]

    ds._load = load
    rng = np.random.default_rng(11)
    n_bins = [ds.w_max // b for b in ds.binsizes]
    partial = 0
    for gene in genes:
        g = ds.genes[gene]
        chrom, tss, strand = g["tss"]
        regs = ds.regions(gene, dtype=torch.float64)
        S = len(g["pcres"])
        Dp = [rng.standard_normal((L, 7)) for L in n_bins]                       # including the pad rows
        Dc = [[rng.standard_normal((L, 7)) for L in n_bins] for _ in range(S)]
        loss = 0
        for r, b in enumerate(ds.binsizes):
            p, _, _, pcs = regs[b]
            assert p.dtype == torch.float64
            loss = loss + (p * torch.from_numpy(Dp[r]).t()).sum()
            for s, (x, _, _) in enumerate(pcs):
                loss = loss + (x * torch.from_numpy(Dc[s][r]).t()).sum()
        loss.backward()
        files = [(chrom, tss - 20000, tss + 20000)] + list(g["pcres"])
        for (s, flip, a), key in zip(load_raw_regions(ChromoformerDataset(meta, ds.npy_dir, genes, w_prom=w_prom), gene), files):
            c0, nc = raw_window(ds, s, a.shape[1])
            partial += any(nc % b for b in ds.binsizes)
            ref = leaves[key].grad.numpy()
            got = closed_form(a, c0, nc, flip, ds.binsizes, n_bins, Dp if s < 0 else Dc[s])
            assert flip == (s < 0 and strand == "-")
            assert np.abs(got - ref[:, c0:c0 + nc]).max() <= 1e-12 * np.abs(ref).max(), (gene, s)
            outside = np.ones(ref.shape[1], bool)
            outside[c0:c0 + nc] = False
            assert not ref[:, outside].any()
    assert partial, "the dataset must hold partial last bins"


def test_predict_parser_accepts_the_raw_saliency_options():
    from chromoformer_amd import predict
    a = predict.build_parser().parse_args(["-m", "m.csv", "-d", "npy", "-o", "out.csv", "--raw-saliency-dir", "sal", "--raw-saliency-target", "0",
                                           "--raw-saliency-times-input"])
    assert a.raw_saliency_dir == "sal" and a.raw_saliency_target == 0 and a.raw_saliency_times_input is True
    b = predict.build_parser().parse_args(["-m", "m.csv", "-d", "npy", "-o", "out.csv"])
    assert b.raw_saliency_dir is None and b.raw_saliency_target is None and b.raw_saliency_times_input is False


def test_packed_store_without_raw_signals_is_refused_by_name(tmp_path):
    from chromoformer_amd import pack, predict
    d = str(tmp_path / "npy")
    meta = make_dataset(d, n_genes=3, seed=5)
    out = os.path.join(d, pack.DEFAULT_NAME)
    pack.pack(meta, d, out, device=None)
    names = sorted(f for f in os.listdir(d) if f.endswith(".npy"))
    for f in names:
        os.remove(os.path.join(d, f))
    first = pd.read_csv(meta).iloc[0]
    missing = "%s:%d-%d.npy" % (first.chrom, first.start - 20000, first.start + 20000)
    with pytest.raises(FileNotFoundError, match="raw signals are required") as e:
        predict.predict(meta, d, store_path=out, raw_saliency_dir=str(tmp_path / "sal"))
    assert missing in str(e.value)
    assert not os.path.exists(str(tmp_path / "sal"))
