"""Integrated gradients in raw-signal space, the parts that need no GPU:

  * the identity the device path rests on, in fp64 on the small dataset (both strands, partial last bins, a gene without partners):
    the per-bin coeff = (1 + m) C of the tensor-level oracle pushed through the closed form of the binning backward with
    times_input equals integrated gradients computed directly from the raw signal (autograd to the raw leaf per node, never a bin
    mean); per resolution the tracks sum, bin by bin, to attr = m C; and the tracks sum to the same total as attr, so their distance
    to F(x) - F(0) is the tensor-level delta;
  * the CLI's parser takes --raw-ig-dir; path="signal" refuses a feature baseline before it touches the device."""
import numpy as np
import pandas as pd
import pytest
import torch

from chromoformer_amd.attribution import ig_quadrature64
from oracle import chromoformer_oracle as orc
from tests.raw_grad_oracle import closed_form, make_small_dataset
from tests.raw_ig_oracle import batch_from_raw, oracle_ig_from_raw, oracle_ig_signal


def test_bin_mean_identity_in_fp64(tmp_path):
    from chromoformer_amd.data import ChromoformerDataset, load_raw_regions, raw_window
    meta, orphan = make_small_dataset(str(tmp_path / "npy"))
    ids = pd.read_csv(meta).gene_id.tolist()
    ds = ChromoformerDataset(meta, str(tmp_path / "npy"), ids)
    assert {ds.genes[g]["tss"][2] for g in ids} == {"+", "-"} and not ds.genes[orphan]["pcres"]
    P = orc.init_params(seed=7)
    t, dt = 1, torch.float64
    a, w = ig_quadrature64("gausslegendre", 4)
    tracks, lx, lb = oracle_ig_from_raw(ds, P, ids, a, w, t, dt)
    with torch.no_grad():
        batch, _ = batch_from_raw(ds, ids, dt)
    attr, coeff, lx2, lb2, delta = oracle_ig_signal(P, batch, a, w, t, dtype=dt)
    assert torch.equal(lx, lx2) and torch.equal(lb, lb2)
    n_bins = [ds.w_max // b for b in ds.binsizes]
    partial = 0
    for i, g in enumerate(ids):
        total = 0.0
        for s, flip, x in load_raw_regions(ds, g):
            c0, nc = raw_window(ds, s, x.shape[1])
            pick = (lambda d, b: d["promoter_feats"][b][i, 0]) if s < 0 else (lambda d, b: d["pcre_feats"][b][i, s])
            dfeat = [pick(coeff, b).numpy() for b in ds.binsizes]
            got = closed_form(x, c0, nc, flip, ds.binsizes, n_bins, dfeat, times_input=True)
            ref = tracks[g, s].numpy()
            assert np.abs(ref[:, :c0]).max(initial=0) == 0 and np.abs(ref[:, c0 + nc:]).max(initial=0) == 0
            ref = ref[:, c0:c0 + nc]
            assert np.linalg.norm(got - ref) <= 1e-9 * np.linalg.norm(ref), (g, s)
            total += got.sum()
            for r, (b, L) in enumerate(zip(ds.binsizes, n_bins)):        # one resolution at a time: bin sums of the track = attr
                one = [d if k == r else np.zeros_like(d) for k, d in enumerate(dfeat)]
                tr = closed_form(x, c0, nc, flip, ds.binsizes, n_bins, one, times_input=True)
                n = min(-(-nc // b), L)
                left = -(-(L - n) // 2)
                at = pick(attr, b).numpy()
                seen = np.zeros(L, dtype=bool)
                for k in range(n):
                    p = L - 1 - (left + k) if flip else left + k
                    seen[p] = True
                    assert np.allclose(tr[:, k * b:(k + 1) * b].sum(1), at[p], rtol=1e-9, atol=1e-13 * np.abs(at).max()), (g, s, b, k)
                assert np.all(at[~seen] == 0)                              # padded bins: m = 0
                partial += nc % b != 0
        gap = float(lx[i, t] - lb[i, t])
        assert abs((total - gap) - float(delta[i])) <= 1e-9 * abs(gap) + 1e-12, (g, total - gap, float(delta[i]))
    assert partial > 0


def test_cli_parser_accepts_raw_ig_dir():
    from chromoformer_amd import predict
    args = predict.build_parser().parse_args(["-m", "m.csv", "-d", "npy", "-o", "p.csv", "--raw-ig-dir", "ig", "--ig-steps", "8"])
    assert args.raw_ig_dir == "ig" and args.ig_steps == 8
    assert predict.build_parser().parse_args(["-m", "m.csv", "-d", "npy", "-o", "p.csv"]).raw_ig_dir is None


def test_signal_path_refuses_a_feature_baseline_before_the_device():
    from chromoformer_amd import ChromoformerClassifier
    cfg = orc._cfg(None)
    model = ChromoformerClassifier(cfg["n_feats"], cfg["d_emb"], cfg["d_head"], cfg["embed"], cfg["pairwise_interaction"], cfg["regulation"],
                                   binsizes=cfg["binsizes"], seed=1, i_max=cfg["i_max"], w_max=cfg["w_max"], max_batch=2)      # (never .cuda())
    batch = orc.synthetic_batch(2, seed=1, regime="realistic")
    args = [batch[k] for k in ("promoter_feats", "promoter_pad_masks", "pcre_feats", "pcre_pad_masks", "interaction_masks", "interaction_freq")]
    base = {"pcre_feats": {b: torch.zeros_like(v[:1]) for b, v in batch["pcre_feats"].items()}}
    with pytest.raises(ValueError, match="zero signal"):
        model.integrated_gradients(*args, n_steps=2, baselines=base, path="signal")
    with pytest.raises(ValueError, match="needs promoter_feats or pcre_feats"):
        model.integrated_gradients(*args, n_steps=2, inputs=("interaction_freq",), path="signal")
    with pytest.raises(ValueError, match="path"):
        model.integrated_gradients(*args, n_steps=2, path="curved")
