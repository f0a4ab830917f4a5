"""In-silico pCRE deletion (cf_pcre_ablation, ChromoformerBase.pcre_ablation): logits [B, i_max + 2, n_out] with nothing deleted,
each pCRE slot deleted (its interaction-mask row and column set) and the promoter alone.

  * the reference's logits on the default configuration, classifier and regressor (tests/golden/pcre_ablation.npz);
  * bit-identity with model(...) on the explicitly masked batches, since every variant runs the per-gene kernels of an inference
    forward; dummy slots give the baseline;
  * bsz 64 in the realistic regime against the oracle (tests/ablation_oracle.py), bit-identical whatever the chunking, call after call;
  * the other accepted shapes: layer-by-layer Regulation, i_max = 16, d_emb = 64, embed.n_layers = 2, d_head = 64, the regressor;
  * the C ABI: launches = the trunk once + 1 + chunks x (1 + Regulation + head), refusals by name;
  * no side effects on training or attention maps, a pending backward of an earlier forward refused;
  * `predict.py --pcre-ablation-out`."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import chromoformer_oracle as orc
from tests.ablation_oracle import oracle_ablation, variant_masks
from tests.helpers import GOLDEN, load_npz_batch

pytestmark = pytest.mark.gpu
TOL = 1e-4
ARGS = ("promoter_feats", "promoter_pad_masks", "pcre_feats", "pcre_pad_masks", "interaction_masks", "interaction_freq")


def _args(batch):
    return [batch[k] for k in ARGS]


def _model(cfg=None, B=8, regression=False, seed=42):
    from chromoformer_amd import ChromoformerClassifier, ChromoformerRegressor
    c = orc._cfg(cfg)
    Model = ChromoformerRegressor if regression else ChromoformerClassifier
    return Model(c["n_feats"], c["d_emb"], c["d_head"], c["embed"], c["pairwise_interaction"], c["regulation"], binsizes=c["binsizes"],
                 seed=seed, i_max=c["i_max"], w_max=c["w_max"], max_batch=B).cuda(0)


def _dummies(batch):
    """[B, S]: slots whose interaction-mask column is masked for the promoter row at every resolution (dataset dummies)."""
    return torch.stack([m[:, 0, 0, 1:] for m in batch["interaction_masks"].values()]).all(0)


@pytest.mark.parametrize("regression", [False, True], ids=["classifier", "regressor"])
def test_default_config_matches_the_reference(regression):
    z = np.load(os.path.join(GOLDEN, "pcre_ablation.npz"))
    head = "reg" if regression else "clf"
    model = _model(regression=regression)
    for tag, batch in (("demo", load_npz_batch("demo_subset.npz")[0]), ("real", orc.synthetic_batch(8, seed=31, regime="realistic"))):
        got = model.pcre_ablation(*_args(batch)).cpu()
        ref = torch.from_numpy(z["%s.%s.masked" % (tag, head)])
        assert got.shape == ref.shape
        assert (got - ref).abs().max().item() < TOL, (tag, (got - ref).abs().max().item())


def test_bit_identical_to_the_forward_on_masked_batches():
    batch = orc.synthetic_batch(8, seed=31, regime="realistic")
    model = _model(B=8)
    S = model.i_max
    got = model.pcre_ablation(*_args(batch)).cpu()
    assert not got.requires_grad and got.shape == (8, S + 2, 2)
    with torch.no_grad():
        for v in range(S + 2):
            ref = model(*_args(variant_masks(batch, v, S))).cpu()
            assert torch.equal(got[:, v], ref), v
    dummy = _dummies(batch)
    assert bool(dummy.any()) and not bool(dummy.all())
    for j in range(S):
        assert torch.equal(got[dummy[:, j], 1 + j], got[dummy[:, j], 0]), j
        assert not torch.equal(got[~dummy[:, j], 1 + j], got[~dummy[:, j], 0]) or not bool((~dummy[:, j]).any()), j


def test_bsz64_realistic_against_the_oracle_and_chunking_invariant():
    batch = orc.synthetic_batch(64, seed=77, regime="realistic")
    ref = oracle_ablation(orc.init_params(None, 42, False), batch)
    runs = {}
    for cap in (64, 640, 96):      # 10 chunks, one chunk, 640 = 6 x 96 + 64
        model = _model(B=cap)
        a = model.pcre_ablation(*_args(batch)).cpu()
        b = model.pcre_ablation(*_args(batch)).cpu()
        assert torch.equal(a, b), cap                                # call after call
        runs[cap] = a
    assert (runs[64] - ref).abs().max().item() < TOL
    assert torch.equal(runs[64], runs[640]) and torch.equal(runs[64], runs[96])
    model = _model(B=64)
    one = model.pcre_ablation(*_args({k: ({r: t[5:6] for r, t in v.items()} if isinstance(v, dict) else v[5:6])
                                      for k, v in batch.items()})).cpu()
    assert one.shape == (1, 10, 2) and torch.equal(one[0], runs[64][5])      # B = 1


def test_variants_straddling_chunks_equal_the_forward_on_hand_set_masks():
    """The smallest shape at which a gene's variants straddle chunks: i_max = 2 (V = 4), B = 2, max_batch = 3 -- chunks of 3, 3 and
    2 rows, gene 0 ending and gene 1 beginning inside the second.  Every column is model(...) on the batch with the variant's rows
    and columns of interaction_masks set here, by hand, bit for bit; and one chunk (max_batch = 8) gives the same bits."""
    cfg = orc._cfg(dict(i_max=2))
    batch = orc.synthetic_batch(2, cfg=cfg, seed=13, regime="realistic")
    P = orc.init_params(cfg, 3, False)
    runs = {}
    for cap in (3, 8):
        model = _model(cfg, B=cap, seed=3)
        model.load_state_dict(P)
        runs[cap] = model.pcre_ablation(*_args(batch))
        assert runs[cap].shape == (2, 4, 2)
        gone = {0: [], 1: [1], 2: [2], 3: [1, 2]}      # variant -> the interaction-mask rows and columns it sets
        with torch.no_grad():
            for v, tokens in gone.items():
                masks = {r: m.clone() for r, m in batch["interaction_masks"].items()}
                for m in masks.values():
                    for t in tokens:
                        m[:, 0, t, :] = True
                        m[:, 0, :, t] = True
                ref = model(*_args(dict(batch, interaction_masks=masks)))
                assert torch.equal(runs[cap][:, v], ref), (cap, v)
    assert not torch.equal(runs[3][:, 0], runs[3][:, 3])      # (the promoter alone is another prediction: the masks are read)
    assert torch.equal(runs[3], runs[8])


REG_4x128 = dict(n_layers=6, n_heads=4, d_model=128, d_ff=256)
SHAPES = {
    "reg_4x128": (dict(regulation=REG_4x128), False),
    "i_max16": (dict(i_max=16), False),
    "d_emb_64": (dict(d_emb=64, embed=dict(n_layers=1, n_heads=2, d_model=64, d_ff=128),
                      pairwise_interaction=dict(n_layers=2, n_heads=2, d_model=64, d_ff=256), regulation=REG_4x128), False),
    "embed_2_layers": (dict(embed=dict(n_layers=2, n_heads=2, d_model=128, d_ff=128)), False),
    "d_head_64": (dict(d_head=64), False),
    "regressor": (None, True),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_other_shapes_against_the_oracle(name):
    over, regression = SHAPES[name]
    cfg = orc._cfg(over)
    batch = orc.synthetic_batch(5, cfg=cfg, seed=13, regime="realistic")
    P = orc.init_params(cfg, 3, regression)
    model = _model(cfg, B=16, regression=regression, seed=3)      # (several chunks: 5 x (i_max + 2) gene-variants)
    model.load_state_dict(P)
    got = model.pcre_ablation(*_args(batch)).cpu()
    ref = oracle_ablation(P, batch, cfg)
    assert got.shape == ref.shape
    assert (got - ref).abs().max().item() < TOL, (got - ref).abs().max().item()
    with torch.no_grad():
        assert torch.equal(got[:, 0], model(*_args(batch)).cpu())


@pytest.mark.parametrize("name,n_reg_head", [("default", 2), ("i_max16", 3 * 6 + 1)])
def test_launch_contract_at_the_c_abi(name, n_reg_head):
    """launches = n_trunk + 1 + chunks x (1 + n_reg_head), with n_trunk + n_reg_head those of cf_forward(save = 0): one chunk gives
    the inference forward's count + 2, each further chunk 1 + n_reg_head (no trunk launch)."""
    from chromoformer_amd import _lib
    cfg = orc._cfg(None if name == "default" else dict(i_max=16))
    B, V = 6, cfg["i_max"] + 2
    batch = orc.synthetic_batch(B, cfg=cfg, seed=23, regime="realistic")
    counts = {}
    for chunks in (1, 3):
        cap = B * V if chunks == 1 else (B * V + 2) // 3
        assert -(-B * V // cap) == chunks
        model = _model(cfg, B=cap)
        with torch.no_grad():
            model(*_args(batch))
        n_inf = model.launch_counts()[0]
        out = model.pcre_ablation(*_args(batch))
        counts[chunks] = model.launch_counts()[0]
        assert counts[chunks] == n_inf + 2 + (chunks - 1) * (1 + n_reg_head), (chunks, n_inf, counts[chunks])
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all())
    assert counts[3] - counts[1] == 2 * (1 + n_reg_head)
    # refusals by name, before anything is launched
    L = _lib.lib()
    small = _model(cfg, B=4)
    packed = model.pack_batch(batch)      # B = 6 > small's max_batch
    st = torch.cuda.current_stream().cuda_stream
    out = torch.empty(B, V, 2, device="cuda")
    assert L.cf_pcre_ablation(small._handle, C.byref(packed[0]), out.data_ptr(), st) != 0
    assert b"max_batch" in L.cf_last_error() and b"cf_pcre_ablation" in L.cf_last_error()
    assert L.cf_pcre_ablation(None, C.byref(packed[0]), out.data_ptr(), st) != 0 and b"null handle" in L.cf_last_error()
    assert L.cf_pcre_ablation(model._handle, None, out.data_ptr(), st) != 0 and b"null batch" in L.cf_last_error()
    # the packed forms (pack_batch, engine.Slot) give the same result as the six tensors
    from chromoformer_amd.engine import Slot
    ref = model.pcre_ablation(*_args(batch)).cpu()
    slot = Slot(model, B).fill(model, batch)
    for p in (packed, slot):
        assert torch.equal(model.pcre_ablation(p).cpu(), ref)


def test_no_side_effects_on_training_and_a_stale_backward_is_refused():
    from chromoformer_amd.engine import Trainer
    batches = [orc.synthetic_batch(8, seed=41 + i, regime="realistic") for i in range(3)]

    def run(interpose):
        model = _model(B=8)
        tr = Trainer(model, lr=1e-3)
        slots = [tr.stage(b) for b in batches[:2]]
        tr.step(slots[0])
        if interpose:
            torch.cuda.synchronize()
            model.pcre_ablation(*_args(batches[2]))
            torch.cuda.synchronize()
        tr.step(slots[1])
        torch.cuda.synchronize()
        sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        sd["<exp_avg>"], sd["<exp_avg_sq>"] = model._mflat.cpu().clone(), model._vflat.cpu().clone()
        return sd

    ref, got = run(False), run(True)
    assert all(torch.equal(ref[k], got[k]) for k in ref)

    model = _model(B=8)
    b = batches[0]
    with torch.enable_grad():
        out = model(*_args(b))
        model.pcre_ablation(*_args(batches[1]))
        with pytest.raises(RuntimeError, match="pcre_ablation"):
            out[:, 1].sum().backward()
        model(*_args(b))[:, 1].sum().backward()      # a fresh forward trains as before
    assert float(model._gflat.abs().sum()) > 0

    lg0, maps0 = model.attention_maps(*_args(b))
    lg0, maps0 = lg0.cpu(), {k: {r: t.cpu() for r, t in v.items()} if isinstance(v, dict) else v.cpu() for k, v in maps0.items()}
    model.pcre_ablation(*_args(batches[2]))
    lg1, maps1 = model.attention_maps(*_args(b))
    assert torch.equal(lg0, lg1.cpu())
    for k, v in maps0.items():
        if isinstance(v, dict):
            assert all(torch.equal(t, maps1[k][r].cpu()) for r, t in v.items()), k
        else:
            assert torch.equal(v, maps1[k].cpu()), k


def test_predict_writes_the_ablation(tmp_path):
    import pandas as pd

    from chromoformer_amd import ChromoformerClassifier, predict
    from chromoformer_amd.data import ChromoformerDataset
    from tests.synth_data import make_dataset
    meta = make_dataset(str(tmp_path / "npy"), n_genes=20, seed=11)
    P = orc.init_params(seed=7)
    ck = str(tmp_path / "w.pt")
    torch.save({"net": P}, ck)
    out = str(tmp_path / "abl.npy")
    _, pred = predict.predict(meta, str(tmp_path / "npy"), ck, pcre_ablation_out=out)
    abl = np.load(out)
    assert abl.shape == (20, 10) and abl.dtype == np.float32
    assert np.array_equal(abl[:, 0], pred)                      # column 0 is the prediction, bit for bit
    out2 = str(tmp_path / "abl2.npy")
    assert predict.main(["-m", meta, "-d", str(tmp_path / "npy"), "-w", ck, "-o", str(tmp_path / "p.csv"), "--pcre-ablation-out", out2]) == 0
    assert np.array_equal(np.load(out2), abl)
    assert np.array_equal(pd.read_csv(str(tmp_path / "p.csv"))["prediction"].to_numpy().astype(np.float32), abl[:, 0])
    ds = ChromoformerDataset(meta, str(tmp_path / "npy"), pd.read_csv(meta).gene_id.tolist())
    batch = torch.utils.data.default_collate([ds[i] for i in range(len(ds))])
    model = ChromoformerClassifier(seed=123, max_batch=32).cuda(0)
    model.load_state_dict(P)
    ref = torch.sigmoid(model.pcre_ablation(*_args(batch)).cpu())[..., 1].numpy()
    assert np.abs(abl - ref).max() <= 1e-6
    assert np.isfinite(abl).all() and (np.abs(abl[:, 1:] - abl[:, :1]).max(0) > 0).any()
