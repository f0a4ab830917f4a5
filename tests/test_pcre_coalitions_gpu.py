"""pCRE coalition forwards, exact Shapley values and pair epistasis (cf_pcre_coalitions / cf_pcre_shapley / cf_pcre_epistasis and the
ChromoformerBase methods of the same names): row (b, m) is the inference forward of gene b with the interaction-mask row and column
of every pCRE slot whose bit of the word m is clear set.

  * the reference's logits of all 256 coalitions on the default configuration (tests/golden/pcre_coalitions.npz), phi against the
    float64 Shapley values of those logits;
  * bit-identity with model(...) on the explicitly masked batches and with pcre_ablation; dummy-bit twins;
  * small shapes against the live oracle (tests/coalition_oracle.py), whatever the chunking, call after call; null players exactly 0;
    phi within the fp32 rounding bound of its own coalition logits; the efficiency gap;
  * the other accepted shapes; i_max = 16;
  * the C ABI: launches, refusals by name, the handle-owned row buffer, the packed forms;
  * no side effects on training or attention maps, a pending backward of an earlier forward refused;
  * epistasis bit-equal to its definition on pcre_coalitions, symmetric, leave-one-out on the diagonal;
  * `predict.py --pcre-shapley-out / --pcre-epistasis-out`."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import chromoformer_oracle as orc
from tests.coalition_oracle import coalition_masks, epistasis_fp32, oracle_coalitions, shapley_fp64
from tests.helpers import GOLDEN, load_npz_batch

pytestmark = pytest.mark.gpu
TOL = 1e-4      # the project's logit bound
U = 2.0 ** -24
ARGS = ("promoter_feats", "promoter_pad_masks", "pcre_feats", "pcre_pad_masks", "interaction_masks", "interaction_freq")
REG_4x128 = dict(n_layers=6, n_heads=4, d_model=128, d_ff=256)


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


def _gamma(S):
    """n u / (1 - n u), n = 2^(S - 1) + 3: one subtraction, the weight's rounding, one product and the additions of a slot's sum."""
    n = 2 ** (S - 1) + 3
    return n * U / (1 - n * U)


def _check_phi(phi, info, S):
    """phi against shapley_fp64 of the returned coalition logits, elementwise within the fp32 rounding bound (any summation order);
    info["delta"] within S times that bound plus 4 u max|v|."""
    v = info["coalitions"].cpu().numpy()
    phi64, scale = shapley_fp64(v)
    bound = _gamma(S) * scale
    err = np.abs(phi.cpu().numpy().astype(np.float64) - phi64)
    print("phi: max err %.3e, max bound %.3e, max err / bound %.3f" % (err.max(), bound.max(), (err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all(), (err.max(), bound.max())
    dbound = S * bound.max(1) + 4 * U * np.abs(v).max(1)
    delta = np.abs(info["delta"].cpu().numpy())
    print("delta: max %.3e, max bound %.3e" % (delta.max(), dbound.max()))
    assert delta.shape == dbound.shape and (delta <= dbound).all(), (delta.max(), dbound.max())
    assert torch.equal(info["logits"], info["coalitions"][:, -1]) and torch.equal(info["promoter_only"], info["coalitions"][:, 0])


@pytest.mark.parametrize("regression", [False, True], ids=["classifier", "regressor"])
def test_default_config_matches_the_reference(regression):
    ref = np.load(os.path.join(GOLDEN, "pcre_coalitions.npz"))["demo.%s" % ("reg" if regression else "clf")]
    batch = load_npz_batch("demo_subset.npz")[0]
    model = _model(B=256, regression=regression)
    phi, info = model.pcre_shapley(*_args(batch), return_coalitions=True)
    got = info["coalitions"].cpu().numpy()
    assert got.shape == ref.shape and phi.shape == (6, 8, ref.shape[-1]) and not phi.requires_grad
    d = np.abs(got - ref).max()
    print("coalition logits vs the reference: %.3e" % d)
    assert d < TOL
    phi64, _ = shapley_fp64(ref)
    dp = np.abs(phi.cpu().numpy() - phi64).max()
    print("phi vs shapley_fp64(reference): %.3e" % dp)
    assert dp < 2e-4      # a slot's weights sum to 1 and each difference carries two logit errors
    for b, n in enumerate((0, 1, 5, 8, 8, 3)):      # the demo genes' pCRE counts: dummies are null players
        assert bool((phi[b, n:] == 0).all()) and bool((phi[b, :n] != 0).all()), b


def test_bit_identical_to_the_forward_on_masked_batches_and_to_the_ablation():
    batch = orc.synthetic_batch(8, seed=31, regime="realistic")
    model = _model(B=8)
    S, N = model.i_max, 255
    dummy = _dummies(batch)
    jd = next(j for j in range(S) if bool(dummy[:, j].any()) and not bool(dummy[:, j].all()))      # a slot that is a dummy in some genes
    rng = np.random.RandomState(3)
    base = [int(w) | 1 << jd for w in rng.randint(0, 256, 3)]
    words = [N, 0, N & ~(1 << 0), N & ~(1 << 5)] + base + [w & ~(1 << jd) for w in base] + [int(w) for w in rng.randint(0, 256, 2)]
    got = model.pcre_coalitions(*_args(batch), keep=words).cpu()
    assert not got.requires_grad and got.shape == (8, len(words), 2)
    with torch.no_grad():
        for c, m in enumerate(words):
            ref = model(*_args(coalition_masks(batch, m, S))).cpu()
            assert torch.equal(got[:, c], ref), (c, hex(m))
    abl = model.pcre_ablation(*_args(batch)).cpu()
    assert torch.equal(got[:, 0], abl[:, 0]) and torch.equal(got[:, 1], abl[:, S + 1])
    assert torch.equal(got[:, 2], abl[:, 1 + 0]) and torch.equal(got[:, 3], abl[:, 1 + 5])
    for k in range(3):      # twins that differ in bit jd only: equal where slot jd is a dummy
        a, b = got[:, 4 + k], got[:, 7 + k]
        assert torch.equal(a[dummy[:, jd]], b[dummy[:, jd]]), k
    assert any(not torch.equal(got[~dummy[:, jd], 4 + k], got[~dummy[:, jd], 7 + k]) for k in range(3))
    # the bool form of keep
    bits = torch.tensor([[bool(m >> j & 1) for j in range(S)] for m in words])
    assert torch.equal(model.pcre_coalitions(*_args(batch), keep=bits).cpu(), got)
    with pytest.raises(ValueError, match="pcre_coalitions"):
        model.pcre_coalitions(*_args(batch), keep=[256])


@pytest.fixture(scope="module")
def small():
    """i_max = 3, 5 genes with [0, 0, 0, 2, 3] dummy slots, and all 8 coalition rows by the oracle (40 gene-forwards, computed once)."""
    cfg = orc._cfg(dict(i_max=3))
    batch = orc.synthetic_batch(5, cfg=cfg, seed=13, regime="realistic")
    P = orc.init_params(cfg, 3, False)
    return cfg, batch, P, oracle_coalitions(P, batch, range(8), cfg)


def test_small_shapes_against_the_oracle_chunking_invariant(small):
    cfg, batch, P, ref = small
    dummy = _dummies(batch)
    assert dummy.sum(1).tolist() == [0, 0, 0, 2, 3]
    runs = {}
    for cap in (7, 64, 5):      # 40 rows: chunks straddle genes (7), one chunk (64), five rows a chunk; max_batch >= B = 5
        model = _model(cfg, B=cap, seed=3)
        model.load_state_dict(P)
        phi, info = model.pcre_shapley(*_args(batch), return_coalitions=True)
        phi2, info2 = model.pcre_shapley(*_args(batch), return_coalitions=True)
        assert torch.equal(phi, phi2) and torch.equal(info["coalitions"], info2["coalitions"]), cap      # call after call
        runs[cap] = (phi.cpu(), info["coalitions"].cpu())
        if cap == 7:
            d = (info["coalitions"].cpu() - ref).abs().max().item()
            print("i_max 3: coalition logits vs the oracle %.3e" % d)
            assert d < TOL
            _check_phi(phi, info, 3)
            assert bool((phi.cpu()[dummy] == 0).all()) and bool((phi.cpu()[~dummy] != 0).all())
            rows = info["coalitions"].cpu()[4]      # the gene with no pCRE: every row equal
            assert all(torch.equal(rows[m], rows[0]) for m in range(8))
            assert torch.equal(model.pcre_coalitions(*_args(batch), keep=range(8)), info["coalitions"])
    for cap in (64, 5):
        assert torch.equal(runs[7][0], runs[cap][0]) and torch.equal(runs[7][1], runs[cap][1]), cap


def test_max_batch_4_and_i_max_2(small):
    """max_batch 4 holds a batch of at most 4 genes: genes 1..4 of the batch above (rows bit-equal to the 5-gene runs), 32 rows in
    8 chunks; and i_max = 2, B = 3 (12 oracle gene-forwards)."""
    cfg, batch, P, ref = small
    sub = {k: ({r: t[1:5] for r, t in v.items()} if isinstance(v, dict) else v[1:5]) for k, v in batch.items()}
    model = _model(cfg, B=4, seed=3)
    model.load_state_dict(P)
    phi, info = model.pcre_shapley(*_args(sub), return_coalitions=True)
    assert (info["coalitions"].cpu() - ref[1:5]).abs().max().item() < TOL
    wide = _model(cfg, B=64, seed=3)
    wide.load_state_dict(P)
    phi_w, info_w = wide.pcre_shapley(*_args(batch), return_coalitions=True)
    assert torch.equal(info["coalitions"], info_w["coalitions"][1:5]) and torch.equal(phi, phi_w[1:5])
    _check_phi(phi, info, 3)

    cfg2 = orc._cfg(dict(i_max=2))
    b2 = orc.synthetic_batch(3, cfg=cfg2, seed=13, regime="realistic")
    P2 = orc.init_params(cfg2, 3, False)
    m2 = _model(cfg2, B=4, seed=3)
    m2.load_state_dict(P2)
    phi, info = m2.pcre_shapley(*_args(b2), return_coalitions=True)
    assert phi.shape == (3, 2, 2) and info["coalitions"].shape == (3, 4, 2)
    assert (info["coalitions"].cpu() - oracle_coalitions(P2, b2, range(4), cfg2)).abs().max().item() < TOL
    _check_phi(phi, info, 2)
    d2 = _dummies(b2)
    assert bool((phi.cpu()[d2] == 0).all()) and bool((phi.cpu()[~d2] != 0).all())


SHAPES = {
    "reg_4x128": (dict(i_max=3, regulation=REG_4x128), False),
    "embed_2_layers": (dict(i_max=3, embed=dict(n_layers=2, n_heads=2, d_model=128, d_ff=128)), False),
    "d_emb_64": (dict(i_max=3, d_emb=64, embed=dict(n_layers=1, n_heads=2, d_model=64, d_ff=128),
                      pairwise_interaction=dict(n_layers=2, n_heads=2, d_model=64, d_ff=256), regulation=REG_4x128), False),
    "regressor": (dict(i_max=3), True),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_other_shapes_against_the_oracle(name):
    over, regression = SHAPES[name]
    cfg = orc._cfg(over)
    batch = orc.synthetic_batch(5, cfg=cfg, seed=13, regime="realistic")
    P = orc.init_params(cfg, 3, regression)
    model = _model(cfg, B=16, regression=regression, seed=3)      # (three chunks: 40 rows)
    model.load_state_dict(P)
    phi, info = model.pcre_shapley(*_args(batch), return_coalitions=True)
    ref = oracle_coalitions(P, batch, range(8), cfg)
    assert info["coalitions"].shape == ref.shape
    d = (info["coalitions"].cpu() - ref).abs().max().item()
    print("%s: coalition logits vs the oracle %.3e" % (name, d))
    assert d < TOL
    _check_phi(phi, info, 3)
    with torch.no_grad():
        assert torch.equal(info["logits"], model(*_args(batch)))


def test_i_max_16():
    cfg = orc._cfg(dict(i_max=16))
    batch = orc.synthetic_batch(2, cfg=cfg, seed=13, regime="realistic")
    P = orc.init_params(cfg, 3, False)
    model = _model(cfg, B=256, seed=3)
    model.load_state_dict(P)
    words = [0xFFFF, 0x00FF, 0xFF00, 0x8001, 0x5A5A, 0x0100]      # bits 8..15 in use
    got = model.pcre_coalitions(*_args(batch), keep=words).cpu()
    d = (got - oracle_coalitions(P, batch, words, cfg)).abs().max().item()
    print("i_max 16: coalition logits vs the oracle %.3e" % d)
    assert d < TOL
    one = {k: ({r: t[:1] for r, t in v.items()} if isinstance(v, dict) else v[:1]) for k, v in batch.items()}
    phi, info = model.pcre_shapley(*_args(one), return_coalitions=True)      # 65,536 rows in 256 chunks
    assert phi.shape == (1, 16, 2) and info["coalitions"].shape == (1, 65536, 2)
    assert bool(torch.isfinite(phi).all()) and bool(torch.isfinite(info["coalitions"]).all())
    # (off the fused trunk the gene-batched attention kernel's regions per workgroup follow B: B = 1 and B = 2 agree to rounding only)
    assert (info["coalitions"][0, words].cpu() - got[0]).abs().max().item() < TOL
    _check_phi(phi, info, 16)
    dummy = _dummies(one)
    assert bool((phi.cpu()[dummy] == 0).all())


@pytest.mark.parametrize("name,n_reg_head", [("default", 2), ("i_max16", 3 * 6 + 1)])
def test_launch_contract_and_refusals_at_the_c_abi(name, n_reg_head):
    """fwd = n_trunk + 1 + chunks x (1 + n_reg_head), with n_trunk + n_reg_head those of cf_forward(save = 0): one chunk gives the
    inference forward's count + 2, each further chunk 1 + n_reg_head; Shapley and epistasis add their reducer."""
    from chromoformer_amd import _lib
    cfg = orc._cfg(None if name == "default" else dict(i_max=16))
    S = cfg["i_max"]
    B, n_coal = 6, 10
    rng = np.random.RandomState(1)
    words = [int(w) for w in rng.randint(0, 1 << S, n_coal)]
    batch = orc.synthetic_batch(B, cfg=cfg, seed=23, regime="realistic")
    counts = {}
    for chunks in (1, 3):
        cap = B * n_coal if chunks == 1 else (B * n_coal + 2) // 3
        assert -(-B * n_coal // cap) == chunks
        model = _model(cfg, B=cap)
        with torch.no_grad():
            model(*_args(batch))
        n_inf = model.launch_counts()[0]
        out = model.pcre_coalitions(*_args(batch), keep=words)
        counts[chunks] = model.launch_counts()[0]
        assert counts[chunks] == n_inf + 2 + (chunks - 1) * (1 + n_reg_head), (chunks, n_inf, counts[chunks])
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all())
        R = 1 + S + S * (S - 1) // 2
        eps, _ = model.pcre_epistasis(*_args(batch))
        assert model.launch_counts()[0] == n_inf + 2 + (-(-B * R // cap) - 1) * (1 + n_reg_head) + 1
        if name == "default":
            model.pcre_shapley(*_args(batch))
            assert model.launch_counts()[0] == n_inf + 2 + (-(-B * 256 // cap) - 1) * (1 + n_reg_head) + 1
    assert counts[3] - counts[1] == 2 * (1 + n_reg_head)
    # refusals by name, before anything is launched
    L = _lib.lib()
    small = _model(cfg, B=4)
    packed = model.pack_batch(batch)      # B = 6 > small's max_batch
    bs = C.byref(packed[0])
    st = torch.cuda.current_stream().cuda_stream
    out = torch.empty(B, n_coal, 2, device="cuda")
    keep = np.array(words, dtype=np.uint32)
    kp = keep.ctypes.data
    n0 = model.launch_counts()[0]

    def refused(rc, *needles):
        err = L.cf_last_error()
        assert rc != 0 and all(n in err for n in needles), err

    refused(L.cf_pcre_coalitions(small._handle, bs, kp, n_coal, out.data_ptr(), st), b"cf_pcre_coalitions", b"max_batch")
    refused(L.cf_pcre_coalitions(None, bs, kp, n_coal, out.data_ptr(), st), b"cf_pcre_coalitions", b"null handle")
    refused(L.cf_pcre_coalitions(model._handle, None, kp, n_coal, out.data_ptr(), st), b"cf_pcre_coalitions", b"null batch")
    refused(L.cf_pcre_coalitions(model._handle, bs, kp, n_coal, None, st), b"cf_pcre_coalitions", b"null logits")
    refused(L.cf_pcre_coalitions(model._handle, bs, kp, 0, out.data_ptr(), st), b"cf_pcre_coalitions", b"n_coal")
    refused(L.cf_pcre_coalitions(model._handle, bs, None, n_coal, out.data_ptr(), st), b"cf_pcre_coalitions", b"null keep")
    bad = keep.copy()
    bad[7] = 1 << S
    refused(L.cf_pcre_coalitions(model._handle, bs, bad.ctypes.data, n_coal, out.data_ptr(), st), b"cf_pcre_coalitions", b"keep[7]", b"i_max")
    for fn, nm in ((L.cf_pcre_shapley, b"cf_pcre_shapley"), (L.cf_pcre_epistasis, b"cf_pcre_epistasis")):
        refused(fn(small._handle, bs, out.data_ptr(), None, st), nm, b"max_batch")
        refused(fn(None, bs, out.data_ptr(), None, st), nm, b"null handle")
        refused(fn(model._handle, None, out.data_ptr(), None, st), nm, b"null batch")
        refused(fn(model._handle, bs, None, None, st), nm, b"null")
    assert model.launch_counts()[0] == n0      # nothing was launched
    # the packed forms (pack_batch, engine.Slot) give the same result as the six tensors
    from chromoformer_amd.engine import Slot
    ref = model.pcre_coalitions(*_args(batch), keep=words).cpu()
    eps_ref = model.pcre_epistasis(*_args(batch))[0].cpu()
    slot = Slot(model, B).fill(model, batch)
    for p in (packed, slot):
        assert torch.equal(model.pcre_coalitions(p, keep=words).cpu(), ref)
        assert torch.equal(model.pcre_epistasis(p)[0].cpu(), eps_ref)
    # without a caller's row buffer the rows go to a handle-owned one: the same values
    eps2 = torch.empty_like(eps_ref, device="cuda")
    assert L.cf_pcre_epistasis(model._handle, bs, eps2.data_ptr(), None, st) == 0, L.cf_last_error()
    assert torch.equal(eps2.cpu(), eps_ref)
    if name == "default":
        phi_ref = model.pcre_shapley(packed)[0]
        phi2 = torch.empty_like(phi_ref)
        assert L.cf_pcre_shapley(model._handle, bs, phi2.data_ptr(), None, st) == 0, L.cf_last_error()
        assert torch.equal(phi2, phi_ref)


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
            model.pcre_shapley(*_args(batches[2]))
            model.pcre_epistasis(*_args(batches[2]))
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
        for method, kw in (("pcre_shapley", {}), ("pcre_epistasis", {}), ("pcre_coalitions", dict(keep=[255, 0]))):
            out = model(*_args(b))
            getattr(model, method)(*_args(batches[1]), **kw)
            with pytest.raises(RuntimeError, match=method):
                out[:, 1].sum().backward()
        model(*_args(b))[:, 1].sum().backward()      # a fresh forward trains as before
    assert float(model._gflat.abs().sum()) > 0

    lg0, maps0 = model.attention_maps(*_args(b))
    lg0, maps0 = lg0.cpu(), {k: {r: t.cpu() for r, t in v.items()} if isinstance(v, dict) else v.cpu() for k, v in maps0.items()}
    model.pcre_shapley(*_args(batches[2]))
    lg1, maps1 = model.attention_maps(*_args(b))
    assert torch.equal(lg0, lg1.cpu())
    for k, v in maps0.items():
        if isinstance(v, dict):
            assert all(torch.equal(t, maps1[k][r].cpu()) for r, t in v.items()), k
        else:
            assert torch.equal(v, maps1[k].cpu()), k


def test_epistasis_is_its_definition_on_the_pair_deletion_rows():
    from chromoformer_amd.attribution import coalition_table
    batch = orc.synthetic_batch(8, seed=31, regime="realistic")
    model = _model(B=8)
    S = model.i_max
    eps, info = model.pcre_epistasis(*_args(batch))
    assert eps.shape == (8, S, S, 2) and not eps.requires_grad
    rows = model.pcre_coalitions(*_args(batch), keep=coalition_table("pairs", S)).cpu()
    eps = eps.cpu()
    assert torch.equal(eps, torch.from_numpy(epistasis_fp32(rows.numpy())))
    assert torch.equal(eps, eps.transpose(1, 2))
    abl = model.pcre_ablation(*_args(batch)).cpu()
    for i in range(S):
        assert torch.equal(eps[:, i, i], abl[:, 0] - abl[:, 1 + i]), i
    assert torch.equal(info["logits"].cpu(), abl[:, 0]) and torch.equal(info["single"].cpu(), abl[:, 1:1 + S])
    dummy = _dummies(batch)
    assert bool(dummy.any())
    for b in range(8):
        for j in range(S):
            if dummy[b, j]:
                assert bool((eps[b, j] == 0).all()) and bool((eps[b, :, j] == 0).all()), (b, j)
    live = ~dummy
    assert bool((eps[live[:, :, None] & live[:, None, :]] != 0).any())


def test_predict_writes_shapley_values_and_epistasis(tmp_path):
    import pandas as pd

    from chromoformer_amd import ChromoformerClassifier, predict
    from chromoformer_amd.data import ChromoformerDataset
    from tests.synth_data import make_dataset
    meta = make_dataset(str(tmp_path / "npy"), n_genes=20, seed=11)
    P = orc.init_params(seed=7)
    ck = str(tmp_path / "w.pt")
    torch.save({"net": P}, ck)
    out, eout = str(tmp_path / "shap.npz"), str(tmp_path / "eps.npy")
    _, pred = predict.predict(meta, str(tmp_path / "npy"), ck, pcre_shapley_out=out, pcre_epistasis_out=eout)
    z = np.load(out)
    assert sorted(z.files) == ["logits", "n_pcres", "phi", "promoter_only"]
    assert z["phi"].shape == (20, 8) and z["phi"].dtype == np.float32 and z["logits"].shape == (20,) and z["logits"].dtype == np.float32
    assert z["promoter_only"].shape == (20,) and z["n_pcres"].shape == (20,)
    eps = np.load(eout)
    assert eps.shape == (20, 8, 8) and eps.dtype == np.float32 and np.array_equal(eps, eps.transpose(0, 2, 1))
    out2, eout2 = str(tmp_path / "shap2.npz"), str(tmp_path / "eps2.npy")
    assert predict.main(["-m", meta, "-d", str(tmp_path / "npy"), "-w", ck, "-o", str(tmp_path / "p.csv"), "--pcre-shapley-out", out2,
                         "--pcre-epistasis-out", eout2]) == 0
    assert all(np.array_equal(np.load(out2)[k], z[k]) for k in z.files) and np.array_equal(np.load(eout2), eps)
    ds = ChromoformerDataset(meta, str(tmp_path / "npy"), pd.read_csv(meta).gene_id.tolist())
    batch = torch.utils.data.default_collate([ds[i] for i in range(len(ds))])
    model = ChromoformerClassifier(seed=123, max_batch=32).cuda(0)
    model.load_state_dict(P)
    with torch.no_grad():
        plain = model(*_args(batch)).cpu()
    # the plain run's logits: the written column is logit 1, whose sigmoid is the prediction (one float32 rounding of the sigmoid apart)
    assert np.abs(z["logits"] - plain[:, 1].numpy()).max() <= 1e-6
    assert np.abs(torch.sigmoid(torch.from_numpy(z["logits"])).numpy() - pred).max() <= 2.0 ** -23
    phi, info = model.pcre_shapley(*_args(batch))
    assert np.abs(z["phi"] - phi.cpu()[..., 1].numpy()).max() <= 1e-6
    assert np.abs(z["promoter_only"] - info["promoter_only"].cpu()[:, 1].numpy()).max() <= 1e-6
    # (an entry sums four logits, each held to 1e-6 between the store's inputs, binned on the GPU, and the dataset's)
    assert np.abs(eps - model.pcre_epistasis(*_args(batch))[0].cpu()[..., 1].numpy()).max() <= 4e-6
    dummy = _dummies(batch)
    assert np.array_equal(z["n_pcres"], (~dummy).sum(1).numpy()) and (z["phi"][dummy.numpy()] == 0).all()
