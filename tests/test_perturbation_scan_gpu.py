"""In-silico perturbation scan on the GPU (cf_perturbation_scan, model.perturbation_scan, attribution.perturbation_scan,
predict --scan-out):

  * feats_out against the scaled raw signal binned by the dataset's own code; logits against the CPU oracle and the reference's golden;
  * row (b, v) is the plain forward on the batch with feats_out[:, v] substituted, bit for bit; dead windows, an empty mark set and a
    dummy slot are the baseline; s = 0 over the whole region is the forward with the region's real rows zeroed;
  * the same bits whatever max_batch is, call after call, for the packed forms; other model shapes; the launch contract and every
    refusal by name; no side effects on training; the dataset generator and the CLI.

Three genes of the 20-gene synthetic dataset read at w_prom = 39000: a '-' strand gene whose promoter is stored mirrored with the short
last coarse bin first and whose first pCRE has 12,201 samples, a '+' strand gene with an 1,800-sample pCRE, a gene without partners.
V = 161 at the default eight mark sets: at max_batch = 4 the three genes run in 121 chunks, genes straddling them."""
import ctypes as C
import os

import numpy as np
import pandas as pd
import pytest
import torch

from chromoformer_amd import _lib
from oracle import chromoformer_oracle as orc
from tests import scan_oracle as so
from tests.helpers import GOLDEN
from tests.test_input_grads_gpu import _model

pytestmark = pytest.mark.gpu
BINS = (2000, 500, 100)
GENES = ["ENSGSYN00001", "ENSGSYN00000", "ENSGSYN00002"]
ALL = tuple(range(7))
W = 20
TOL = 1e-4


def _args(batch):
    return tuple(batch[k] for k in so.KEYS)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """-> (dataset, the three genes' batch, their promoter flips): built once, shared, never written."""
    ds = so.scan_dataset(str(tmp_path_factory.mktemp("scan")), w_prom=39000)
    return ds, so.dataset_batch(ds, GENES), [ds.genes[g]["tss"][2] != "+" for g in GENES]


@pytest.fixture(scope="module")
def small():
    """The seed-42 classifier (the golden's weights) at max_batch = 4."""
    return _model(None, False, orc.init_params(None, 42, False), 4)


def _sub(batch, key, b, value):
    """The batch with one feature tensor replaced."""
    out = dict(batch)
    out[key] = dict(batch[key])
    out[key][b] = value
    return out


def _with_region(batch, region, feats, v):
    """The batch with the scanned region's features replaced by feats[b][:, v] (feats on any device)."""
    out = batch
    for b in BINS:
        f = feats[b][:, v].cpu()
        if region == 0:
            out = _sub(out, "promoter_feats", b, f[:, None])
        else:
            t = batch["pcre_feats"][b].clone()
            t[:, region - 1] = f
            out = _sub(out, "pcre_feats", b, t)
    return out


def test_features_against_the_scaled_raw_signal(data, small):
    """feats_out against the from-raw oracle (the window's raw samples scaled, binned by the dataset's own code in fp32), promoter and
    pCRE slot 0, s = 2.5.  Bound: 4 x what the torch fp32 evaluation of the rule reaches against the same oracle on these inputs.
    That evaluation reaches 2.384e-07 (one ulp of a feature in [2, 4); measured on the CPU over all 20 windows of both regions, mark
    sets (1, 4) and all seven), so the bound is 9.537e-07."""
    ds, batch, flips = data
    # preconditions: a '-' strand promoter narrowed to 39000 and a pCRE whose length is a multiple of neither 2,000 nor 500
    assert ds.w_prom == 39000 and ds.genes[GENES[0]]["tss"][2] == "-"
    c, s, e = ds.genes[GENES[0]]["pcres"][0]
    assert (e - s) % 2000 and (e - s) % 500 and not ds.genes[GENES[2]]["pcres"]
    sets = [(1, 4), ALL]
    host32 = 2.384185791015625e-07
    bound = 4 * host32
    for region in (0, 1):
        fl = flips if region == 0 else None
        lg, feats = small.perturbation_scan(*_args(batch), region=region, scale=2.5, mark_sets=sets, flip=fl, return_feats=True)
        feats = {b: t.cpu() for b, t in feats.items()}
        f32, _ = so.scan_rows(batch, region=region, scale=2.5, mark_sets=sets, flip=fl)
        worst = worst32 = 0.0
        for k, g in [(0, g) for g in range(W)] + [(1, 0), (1, 6), (1, 19)]:
            ref = so.batch_from_scaled_raw(ds, GENES, region, g, 1, sets[k], 2.5)
            for b in BINS:
                r = ref["promoter_feats"][b][:, 0] if region == 0 else ref["pcre_feats"][b][:, 0]
                v = 1 + k * W + g
                worst = max(worst, (feats[b][:, v] - r).abs().max().item())
                worst32 = max(worst32, (f32[b][:, v] - r).abs().max().item())
        print("region %d: |feats_out - from raw| %.3e, torch fp32 rule %.3e, bound %.3e" % (region, worst, worst32, bound))
        assert worst <= bound, (region, worst, worst32)
        for b in BINS:      # rows nobody covers, and v = 0, are the gene's own bits
            src = batch["promoter_feats"][b][:, 0] if region == 0 else batch["pcre_feats"][b][:, 0]
            assert torch.equal(feats[b][:, 0], src)
            assert bool(((feats[b] != src[:, None]) <= (f32[b] != src[:, None])).all())      # (a covered zero stays a zero in both)


@pytest.mark.parametrize("regression", [False, True], ids=["classifier", "regressor"])
def test_logits_against_the_oracle_and_the_golden(data, regression):
    ds, batch, flips = data
    P = orc.init_params(None, 42, regression)
    model = _model(None, regression, P, 4)
    z = np.load(os.path.join(GOLDEN, "perturbation_scan.npz"))
    assert [str(g) for g in z["genes"]] == GENES and int(z["w_prom"]) == 39000
    for k, (region, g, width, scale) in enumerate(z["cases"].tolist()):
        region, g, width = int(region), int(g), int(width)
        marks = tuple(np.flatnonzero(z["marks"][k]).tolist())
        fl = flips if region == 0 else None
        got = model.perturbation_scan(*_args(batch), region=region, scale=scale, width=width, mark_sets=[marks], flip=fl).cpu()
        assert got.shape == (3, 1 + W, 1 if regression else 2)
        gold = torch.from_numpy(z["reg" if regression else "clf"][k])
        d_gold = (got[:, [0, 1 + g]] - gold).abs().max().item()
        vs = [0, 1, 1 + g, W]
        ora, _ = so.oracle_scan(P, batch, region=region, scale=scale, width=width, mark_sets=[marks], flip=fl, variants=vs)
        d_ora = (got[:, vs] - ora).abs().max().item()
        print("case", k, "vs golden %.2e, vs oracle %.2e" % (d_gold, d_ora))
        assert d_gold < TOL and d_ora < TOL, (k, d_gold, d_ora)


def test_rows_are_the_plain_forward_bit_for_bit(data, small):
    ds, batch, flips = data
    for region in (0, 1):
        fl = flips if region == 0 else None
        lg, feats = small.perturbation_scan(*_args(batch), region=region, scale=2.5, flip=fl, return_feats=True)
        lg = lg.cpu()
        assert lg.shape == (3, 161, 2)
        k = 7      # all marks together; windows: first, middle, the 12,201-sample pCRE's last real one, the last (dead for every pCRE)
        for v in (0, 1 + k * W, 1 + k * W + 3, 1 + k * W + 6, 1 + k * W + 19, 1 + 2 * W + 19):
            with torch.no_grad():
                ref = small(*_args(_with_region(batch, region, feats, v))).cpu()
            assert torch.equal(lg[:, v], ref), (region, v)
        if region == 1:
            assert torch.equal(lg[:, 1 + k * W + 19], lg[:, 0])


def test_dead_windows_empty_sets_and_dummy_slots_are_the_baseline(data, small):
    ds, batch, flips = data
    with torch.no_grad():
        base = small(*_args(batch)).cpu()
    sets = [ALL, (), (3,)]
    lg = small.perturbation_scan(*_args(batch), region=1, scale=0.0, mark_sets=sets).cpu().reshape(3, -1, 2)
    assert torch.equal(lg[:, 0], base)
    scan = lg[:, 1:].reshape(3, len(sets), W, 2)
    n_c = [7, 1, 0]      # 12,201 and 1,800 samples; no pCRE at all
    for i in range(3):
        assert bool((scan[i, :, n_c[i]:] == base[i]).all()), i              # windows past the region's real bins
        assert bool((scan[i, 1] == base[i]).all()), i                        # the empty set
        if n_c[i]:
            assert bool((scan[i, 0, :n_c[i]] != base[i]).any(-1).all()), i  # ... while every real window of a real set moves the logits
    last = small.perturbation_scan(*_args(batch), region=8, scale=0.0).cpu()      # slot 7: a dummy for the gene without partners
    assert torch.equal(last[2], base[2:3].expand(161, 2)) and not torch.equal(last[0], base[0:1].expand(161, 2))
    prom = small.perturbation_scan(*_args(batch), region=0, scale=0.0, mark_sets=[()], flip=flips).cpu()
    assert torch.equal(prom, base[:, None].expand(3, 1 + W, 2))


def test_whole_region_deletion_is_the_forward_on_zeroed_rows(data, small):
    ds, batch, flips = data
    for region in (0, 1):
        lg = small.perturbation_scan(*_args(batch), region=region, scale=0.0, width=W, mark_sets=[ALL],
                                     flip=flips if region == 0 else None).cpu()
        zeroed = batch
        for b in BINS:
            L = 40000 // b
            key, mk, lead = ("promoter_feats", "promoter_pad_masks", 3) if region == 0 else ("pcre_feats", "pcre_pad_masks", 24)
            t = batch[key][b].clone()
            rows = so.centre_row(batch[mk][b], lead, L).reshape(3, -1, L)[:, region - 1 if region else 0]
            for i in range(3):
                q, n = so.extent(rows[i])
                t[i, region - 1 if region else 0, q:q + n] = 0
            zeroed = _sub(zeroed, key, b, t)
        with torch.no_grad():
            ref = small(*_args(zeroed)).cpu()
        assert torch.equal(lg[:, 1], ref), region
        assert not torch.equal(lg[:2, 1], lg[:2, 0])


def test_same_bits_for_every_max_batch_call_after_call_and_packed_forms(data, small):
    from chromoformer_amd.engine import Slot
    ds, batch, flips = data
    P = orc.init_params(None, 42, False)
    kw = dict(region=0, scale=0.5, width=2, flip=flips, return_feats=True)
    ref, ref_f = small.perturbation_scan(*_args(batch), **kw)
    ref, ref_f = ref.cpu(), {b: t.cpu() for b, t in ref_f.items()}
    again, _ = small.perturbation_scan(*_args(batch), **kw)
    assert torch.equal(again.cpu(), ref)
    for cap in (7, 64):
        model = _model(None, False, P, cap)
        got, got_f = model.perturbation_scan(*_args(batch), **kw)
        assert torch.equal(got.cpu(), ref), cap
        assert all(torch.equal(got_f[b].cpu(), ref_f[b]) for b in BINS), cap
    packed = small.pack_batch(batch)
    slot = Slot(small, 3).fill(small, batch)
    for p in (packed, slot):
        got, got_f = small.perturbation_scan(p, **kw)
        assert torch.equal(got.cpu(), ref)
        assert all(torch.equal(got_f[b].cpu(), ref_f[b]) for b in BINS)
    pc = small.perturbation_scan(*_args(batch), region=1, scale=2.0)
    assert torch.equal(_model(None, False, P, 64).perturbation_scan(*_args(batch), region=1, scale=2.0).cpu(), pc.cpu())


REG_4x128 = dict(n_layers=6, n_heads=4, d_model=128, d_ff=256)
SHAPES = {
    "i_max16": (dict(i_max=16), False),
    "d_emb_64": (dict(d_emb=64, embed=dict(n_layers=1, n_heads=2, d_model=64, d_ff=128),
                      pairwise_interaction=dict(n_layers=2, n_heads=2, d_model=64, d_ff=256), regulation=REG_4x128), False),
    "embed_2_layers": (dict(embed=dict(n_layers=2, n_heads=2, d_model=128, d_ff=128)), False),
    "reg_layer_by_layer": (dict(regulation=REG_4x128), False),
    "regressor": (None, True),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_other_shapes_against_the_oracle(name):
    over, regression = SHAPES[name]
    cfg = orc._cfg(over)
    batch = orc.synthetic_batch(2, cfg=cfg, seed=13, regime="realistic")
    P = orc.init_params(cfg, 3, regression)
    model = _model(cfg, regression, P, 5)
    for region, fl in ((0, [True, False]), (2, None)):
        got = model.perturbation_scan(*_args(batch), region=region, scale=0.0, width=2, mark_sets=[(0, 6), ALL], flip=fl).cpu()
        vs = [0, 1, 1 + 9, 1 + W + 4, 2 * W]
        ora, _ = so.oracle_scan(P, batch, cfg, region=region, scale=0.0, width=2, mark_sets=[(0, 6), ALL], flip=fl, variants=vs)
        d = (got[:, vs] - ora).abs().max().item()
        print(name, "region", region, "vs oracle %.2e" % d)
        assert got.shape == (2, 1 + 2 * W, 1 if regression else 2) and d < TOL, (name, region, d)
        with torch.no_grad():
            assert torch.equal(got[:, 0], model(*_args(batch)).cpu())


def test_launch_contract_and_refusals(data):
    ds, batch, flips = data
    P = orc.init_params(None, 42, False)
    L = _lib.lib()
    for cap, chunks in ((64, 2), (7, 9)):                                  # B * V = 3 * 21 = 63 rows with one mark set ... and a second call
        model = _model(None, False, P, cap)
        with torch.no_grad():
            model(*_args(batch))
        n_fwd = model.launch_counts()[0]
        sets = [ALL] if cap == 7 else [ALL, (0,)]                          # 63 rows in 9 chunks of 7; 123 rows in 2 chunks of 64
        model.perturbation_scan(*_args(batch), region=0, mark_sets=sets)
        assert -(-3 * (1 + len(sets) * W) // cap) == chunks
        assert model.launch_counts()[0] == chunks * (1 + n_fwd), (cap, model.launch_counts()[0], n_fwd)
    model = _model(None, False, P, 4)
    bs, keep = model.pack_batch(batch)
    st = torch.cuda.current_stream().cuda_stream
    out = torch.full((3, 1 + W, 2), float("nan"), device="cuda")
    one = (C.c_uint * 1)(0x7f)
    f0 = model.launch_counts()[0]

    def call(h=model._handle, b=bs, lg=out, no_opts=False, **kw):
        o = _lib.cf_scan_opts()
        o.region, o.width, o.n_sets, o.scale = 0, 1, 1, 0.0
        o.mark_sets = C.cast(one, C.c_void_p)
        for k, v in kw.items():
            setattr(o, k, v)
        return L.cf_perturbation_scan(h, C.byref(b) if b is not None else None, None if no_opts else C.byref(o),
                                      lg.data_ptr() if lg is not None else None, st)

    big = _lib.cf_batch.from_buffer_copy(bs)
    big.B = 5
    bit7 = (C.c_uint * 2)(0x01, 0x80)
    cases = [(dict(h=None), b"null handle"), (dict(b=None), b"null batch"), (dict(no_opts=True), b"null opts"), (dict(lg=None), b"null logits"),
             (dict(mark_sets=None), b"null mark_sets"), (dict(b=big), b"max_batch"), (dict(region=-1), b"region"), (dict(region=9), b"region"),
             (dict(width=0), b"width"), (dict(n_sets=0), b"n_sets"), (dict(scale=-0.5), b"scale"), (dict(scale=float("inf")), b"scale"),
             (dict(scale=float("nan")), b"scale"), (dict(n_sets=2, mark_sets=C.cast(bit7, C.c_void_p)), b"n_feats")]
    for kw, msg in cases:
        assert call(**kw) != 0, kw
        err = L.cf_last_error()
        assert msg in err and b"cf_perturbation_scan" in err, (kw, err)
    # a bin count that is no multiple of the smallest (a feats_out index >= n_res cannot be formed: cf_create takes exactly CF_MAX_RES = 3
    # resolutions, so the check in the entry point is unreachable today)
    cfg = orc._cfg(dict(binsizes=[2000, 800, 100], w_max=40000))
    odd = _model(cfg, False, orc.init_params(cfg, 3, False), 4)
    ob, okeep = odd.pack_batch(orc.synthetic_batch(2, cfg=cfg, seed=13, regime="realistic"))
    assert call(h=odd._handle, b=ob) != 0 and b"multiple" in L.cf_last_error() and b"cf_perturbation_scan" in L.cf_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and model.launch_counts()[0] == f0      # nothing was launched
    # armed riders (a training step in flight): refused; the handle is not used again
    assert L.cf_rider_arm(model._handle, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, 0, 8) == 0, L.cf_last_error()
    assert call() != 0 and b"riders" in L.cf_last_error() and b"cf_perturbation_scan" in L.cf_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    with pytest.raises(ValueError, match="mark_sets"):      # (raised by the method before it calls the library)
        model.perturbation_scan((bs, keep), mark_sets=[(7,)])
    del keep, okeep


def test_no_side_effects_on_training_and_a_stale_backward_is_refused():
    from chromoformer_amd.engine import Trainer
    batches = [orc.synthetic_batch(8, seed=41 + i, regime="realistic") for i in range(3)]
    P = orc.init_params(None, 42, False)

    def run(interpose):
        model = _model(None, False, P, 8)
        tr = Trainer(model, lr=1e-3)
        slots = [tr.stage(b) for b in batches[:2]]
        tr.step(slots[0])
        torch.cuda.synchronize()
        snap = [t.clone() for t in (model._flat, model._gflat, model._mflat, model._vflat)]
        if interpose:
            model.perturbation_scan(*_args(batches[2]), region=0, mark_sets=[ALL])
            model.perturbation_scan(*_args(batches[2]), region=3, scale=2.0, mark_sets=[(1,)], return_feats=True)
            torch.cuda.synchronize()
            for a, b in zip(snap, (model._flat, model._gflat, model._mflat, model._vflat)):
                assert torch.equal(a, b)
        tr.step(slots[1])
        torch.cuda.synchronize()
        sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        sd["<exp_avg>"], sd["<exp_avg_sq>"] = model._mflat.cpu().clone(), model._vflat.cpu().clone()
        return sd

    ref, got = run(False), run(True)
    assert all(torch.equal(ref[k], got[k]) for k in ref)
    model = _model(None, False, P, 8)
    b = batches[0]
    with torch.enable_grad():
        out = model(*_args(b))
        lg = model.perturbation_scan(*_args(batches[1]), mark_sets=[ALL])
        assert not lg.requires_grad
        with pytest.raises(RuntimeError, match="perturbation_scan"):
            out[:, 1].sum().backward()
        model(*_args(b))[:, 1].sum().backward()      # a fresh forward trains as before
    # the C ABI itself refuses a backward without a new saving forward
    bs, keep = model.pack_batch(b)
    st = torch.cuda.current_stream().cuda_stream
    lgt = torch.empty(8, 2, device="cuda")
    _lib.check(_lib.lib().cf_forward(model._handle, C.byref(bs), lgt.data_ptr(), 1, st), "cf_forward")
    model.perturbation_scan((bs, keep), mark_sets=[ALL])
    dl = torch.zeros(8, 2, device="cuda")
    assert _lib.lib().cf_backward_from(model._handle, C.byref(bs), dl.data_ptr(), st) != 0
    assert b"must follow cf_forward" in _lib.lib().cf_last_error()
    lg0, maps0 = model.attention_maps(*_args(b))
    model.perturbation_scan(*_args(batches[2]), mark_sets=[ALL])
    lg1, maps1 = model.attention_maps(*_args(b))
    assert torch.equal(lg0, lg1)
    for k, v in maps0.items():
        if isinstance(v, dict):
            assert all(torch.equal(t, maps1[k][r]) for r, t in v.items()), k
        else:
            assert torch.equal(v, maps1[k]), k


def test_dataset_generator_and_cli(tmp_path):
    from chromoformer_amd import ChromoformerClassifier, predict
    from chromoformer_amd.data import ChromoformerDataset
    from tests.synth_data import make_dataset
    npy = str(tmp_path / "npy")
    meta = make_dataset(npy, n_genes=20, seed=11)
    table = pd.read_csv(meta)
    P = orc.init_params(seed=7)
    ck = str(tmp_path / "w.pt")
    torch.save({"net": P}, ck)
    out = str(tmp_path / "scan.npz")
    assert predict.main(["-m", meta, "-d", npy, "-w", ck, "-o", str(tmp_path / "p.csv"), "--scan-out", out, "--scan-regions", "all"]) == 0
    z = np.load(out)
    assert sorted(z.files) == ["gene_ids", "mark_sets", "pcres", "prediction", "promoter"]
    assert list(z["gene_ids"]) == table.gene_id.tolist() and z["mark_sets"].shape == (8, 7) and z["mark_sets"][7].all()
    assert z["prediction"].dtype == np.float32 and z["promoter"].shape == (20, 8, W) and z["pcres"].shape == (20, 8, 8, W)
    assert np.array_equal(pd.read_csv(str(tmp_path / "p.csv"))["prediction"].to_numpy().astype(np.float32), z["prediction"])
    assert np.isfinite(z["promoter"]).all()                                   # w_prom = 40000: every promoter window is real
    ds = ChromoformerDataset(meta, npy, table.gene_id.tolist())
    for i, gid in enumerate(ds.target_genes):                                 # NaN exactly where a window holds no real bin
        for s in range(8):
            pc = ds.genes[gid]["pcres"]
            n_win = -(-(pc[s][2] - pc[s][1]) // 2000) if s < len(pc) else 0
            assert np.isfinite(z["pcres"][i, s, :, :n_win]).all() and np.isnan(z["pcres"][i, s, :, n_win:]).all(), (gid, s)
    model = ChromoformerClassifier(seed=123, max_batch=32).cuda(0)
    model.load_state_dict(P)
    batch = torch.utils.data.default_collate([ds[i] for i in range(len(ds))])
    flips = [ds.genes[g]["tss"][2] != "+" for g in ds.target_genes]
    ref = torch.sigmoid(model.perturbation_scan(*_args(batch), region=0, flip=flips).cpu())[..., 1].numpy()
    assert np.abs(z["promoter"] - ref[:, 1:].reshape(20, 8, W)).max() <= 1e-6
    assert np.abs(z["prediction"] - ref[:, 0]).max() <= 1e-6
    # the generator: shapes, coordinates, finite values, the same numbers
    genes = ds.target_genes[:5]
    res = list(model.perturbation_scan_dataset(ds, genes=genes, regions="all", bsz=3))
    assert [d["gene_id"] for d in res] == genes
    for i, d in enumerate(res):
        g = ds.genes[d["gene_id"]]
        chrom, tss, _ = g["tss"]
        assert sorted(d) == ["gene_id", "logits", "mark_sets", "regions", "scan", "windows"]
        assert d["regions"] == [(chrom, tss - 20000, tss + 20000)] + [tuple(p) for p in g["pcres"]]
        assert len(d["windows"]) == len(d["scan"]) == len(d["regions"]) and len(d["mark_sets"]) == 8
        assert d["logits"].shape == (2,) and d["logits"].dtype == np.float32
        for (c, s, e), w, sc in zip(d["regions"], d["windows"], d["scan"]):
            n_win = -(-(e - s) // 2000)
            assert w.dtype == np.int64 and w.shape == (n_win, 2) and w[0, 0] == s and w[-1, 1] == e
            assert sc.dtype == np.float32 and sc.shape == (8, n_win, 2) and np.isfinite(sc).all()
        sig = 1 / (1 + np.exp(-d["scan"][0][..., 1].astype(np.float64)))
        assert np.abs(sig - z["promoter"][i]).max() <= 1e-6
