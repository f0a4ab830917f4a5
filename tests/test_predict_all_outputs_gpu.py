"""predict.predict with all 36 outputs requested at once against three runs that request disjoint thirds: the same predictions and the
same files, array by array and bit for bit.  An output depends neither on which others were requested nor on the order of the
writers, and the datasets built on first use and the donor store are shared correctly.  Three synthetic genes, bsz = 2 (two batches,
the second ragged), seed-42 classifier weights, every option at the smallest value it allows."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SLOT_AND_EXACT = {"attention_dir": "att", "embeddings_out": "emb.npy", "pcre_ablation_out": "abl.npy", "pcre_shapley_out": "pcre_phi.npz",
                  "pcre_epistasis_out": "pcre_eps.npy", "pcre_interactions_out": "pcre_int.npy", "pcre_dividends_out": "pcre_div.npz",
                  "mark_shapley_out": "mark_phi.npz", "mark_epistasis_out": "mark_eps.npy", "mark_interactions_out": "mark_int.npy",
                  "mark_dividends_out": "mark_div.npz", "ig_dir": "ig", "scan_out": "scan.npz", "contact_shapley_out": "contact_phi.npz",
                  "contact_interactions_out": "contact_int.npy", "contact_dividends_out": "contact_div.npz"}
DONOR = {"mark_donor_shapley_out": "donor_phi.npz", "mark_donor_epistasis_out": "donor_eps.npy", "mark_donor_interactions_out": "donor_int.npy",
         "mark_donor_dividends_out": "donor_div.npz", "mark_donor_sampled_shapley_out": "donor_sampled.npz",
         "mark_donor_sampled_interactions_out": "donor_pairs.npz", "mark_donor_backselect_out": "donor_backselect.npz",
         "contact_donor_shapley_out": "contact_donor.npz", "window_donor_shapley_out": "window_donor.npz",
         "fine_window_donor_shapley_out": "fine_window_donor.npz", "raw_donor_ig_dir": "raw_donor_ig"}
REST = {"raw_ig_dir": "raw_ig", "raw_saliency_dir": "raw_saliency", "fine_scan_out": "fine_scan.npz", "mark_sampled_shapley_out": "sampled.npz",
        "mark_sampled_interactions_out": "pairs.npz", "mark_backselect_out": "backselect.npz", "window_shapley_out": "window.npz",
        "fine_window_shapley_out": "fine_window.npz", "transplant_out": "transplant.npz"}
THIRDS = (SLOT_AND_EXACT, DONOR, REST)
OPTIONS = dict(ig_steps=2, mark_perms=2, window_perms=2, fine_window_perms=2, mark_sampled_players="marks", mark_backselect_players="marks",
               mark_focal=1, scan_width=10, fine_scan_width=100, window_width=10, fine_window_width=10, fine_window_zoom=1,
               transplant_freq=[2.0])      # (2 scan windows, 4 fine scan windows, 2 window players and 2 fine ones, 1 focal player, 1 candidate)


def make_data(root):
    """The three genes, the donor cell type over the same regions, the weights and one transplant candidate -> predict()'s common arguments."""
    from chromoformer_amd.data import ChromoformerDataset
    from oracle import chromoformer_oracle as orc
    from tests import donor_oracle as do
    from tests.synth_data import make_dataset
    npy, dnpy, ck, bed = os.path.join(root, "npy"), os.path.join(root, "donor"), os.path.join(root, "w.pt"), os.path.join(root, "cand.bed")
    meta = make_dataset(npy, n_genes=3, seed=11)
    do.donor_dataset(npy, dnpy, do.DONOR_SEED, w_prom=40000)
    torch.save({"net": orc.init_params(seed=42)}, ck)
    import pandas as pd
    ds = ChromoformerDataset(meta, npy, pd.read_csv(meta).gene_id.tolist())
    partner = next(r for g in ds.target_genes for r in ds.genes[g]["pcres"])
    with open(bed, "w") as fh:
        fh.write("\t".join(str(x) for x in partner) + "\n")
    return dict(meta_path=meta, npy_dir=npy, weights=ck, bsz=2, donor_npy_dir=dnpy, transplant_bed=bed)


def run(data, outs, out_dir):
    """One predict.predict call that writes `outs` (argument -> name under out_dir) -> the predictions."""
    from chromoformer_amd import predict
    os.makedirs(out_dir)
    kw = dict(data, **OPTIONS)
    if not set(outs) & set(DONOR):
        del kw["donor_npy_dir"]
    if "transplant_out" not in outs:
        del kw["transplant_bed"], kw["transplant_freq"]
    return predict.predict(**kw, **{arg: os.path.join(out_dir, name) for arg, name in outs.items()})[1]


def arrays(path):
    """Every array below `path` (a file or a directory of .npy / .npz files) by name; an .npz archive by member."""
    if os.path.isdir(path):
        return {os.path.join(name, k): a for name in sorted(os.listdir(path)) for k, a in arrays(os.path.join(path, name)).items()}
    loaded = np.load(path)
    return {"": loaded} if isinstance(loaded, np.ndarray) else {k: loaded[k] for k in loaded.files}


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_every_output_is_the_same_alone_and_with_all_others(tmp_path):
    assert sum(len(t) for t in THIRDS) == 36 and len({**SLOT_AND_EXACT, **DONOR, **REST}) == 36
    data = make_data(str(tmp_path))
    every = str(tmp_path / "all")
    pred = run(data, {**SLOT_AND_EXACT, **DONOR, **REST}, every)
    assert pred.shape == (3,) and pred.dtype == np.float32
    for k, third in enumerate(THIRDS):
        part = str(tmp_path / ("third%d" % k))
        assert same_bits(run(data, third, part), pred), k
        for name in third.values():
            got, want = arrays(os.path.join(every, name)), arrays(os.path.join(part, name))
            assert got and sorted(got) == sorted(want), name
            for key in got:
                assert same_bits(got[key], want[key]), (name, key)
