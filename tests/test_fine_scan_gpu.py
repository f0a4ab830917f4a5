"""Fine-resolution perturbation scan on the GPU (cf_perturbation_scan_fine, model.perturbation_scan_fine):

  * feats_out against the CPU oracle (tests/fine_scan_oracle.py) within the bounds of tests/test_fine_scan_cpu.py; logits against the
    oracle, classifier and regressor;
  * row (b, v) is the plain forward on the batch with feats_out[:, v] substituted, bit for bit; a window that is a union of whole coarse
    bins is cf_perturbation_scan's row, bit for bit; windows past the real bins, an empty mark set and a dummy slot are the baseline;
  * per-gene starts; the same bits whatever max_batch is, call after call, for the packed forms; another nested shape and the
    all-rows Embedding; the launch contract and every refusal by its message; no side effects on training.

The three genes of tests/test_perturbation_scan_gpu.py (w_prom = 39000: 390 finest bins, the '-' strand promoter stored mirrored with
its ten-child coarse bin first; pCREs of 12,201 and 1,800 samples, a gene without partners), a few dozen rows per gene."""
import ctypes as C

import numpy as np
import pytest
import torch

from chromoformer_amd import _lib
from oracle import chromoformer_oracle as orc
from tests import fine_scan_oracle as fo
from tests import scan_oracle as so
from tests.test_fine_scan_cpu import PART_C, WHOLE_TOL
from tests.test_input_grads_gpu import _model

pytestmark = pytest.mark.gpu
BINS = (2000, 500, 100)
GENES = ["ENSGSYN00001", "ENSGSYN00000", "ENSGSYN00002"]
ALL = tuple(range(7))
TOL = 1e-4
#: (region, per-gene start, per-gene length): the promoter's tail and both strands, the 12,201-sample pCRE's one-sample last bin
ZOOMS = {0: ([371, 0, 17], [39000] * 3), 1: ([104, 0, 3], [12201, 1800, 0])}
KW = dict(width=7, stride=3, n_windows=7)


def _args(batch):
    return tuple(batch[k] for k in so.KEYS)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """-> (dataset, the three genes' batch, their promoter flips): built once, shared, never written."""
    ds = so.scan_dataset(str(tmp_path_factory.mktemp("fine")), w_prom=39000)
    c, s, e = ds.genes[GENES[0]]["pcres"][0]
    assert e - s == 12201 and ds.genes[GENES[0]]["tss"][2] == "-" and not ds.genes[GENES[2]]["pcres"]
    c, s, e = ds.genes[GENES[1]]["pcres"][0]
    assert e - s == 1800
    return ds, so.dataset_batch(ds, GENES), [ds.genes[g]["tss"][2] != "+" for g in GENES]


@pytest.fixture(scope="module")
def small():
    """The seed-42 classifier at max_batch = 4."""
    return _model(None, False, orc.init_params(None, 42, False), 4)


def _sub(batch, key, b, value):
    out = dict(batch)
    out[key] = dict(batch[key])
    out[key][b] = value
    return out


def _with_region(batch, region, feats, v, bins=BINS):
    """The batch with the scanned region's features replaced by feats[b][:, v] (feats on any device)."""
    out = batch
    for b in bins:
        f = feats[b][:, v].cpu()
        if region == 0:
            out = _sub(out, "promoter_feats", b, f[:, None])
        else:
            t = batch["pcre_feats"][b].clone()
            t[:, region - 1] = f
            out = _sub(out, "pcre_feats", b, t)
    return out


def _src(batch, region, b):
    return batch["promoter_feats"][b][:, 0] if region == 0 else batch["pcre_feats"][b][:, region - 1]


@pytest.mark.parametrize("scale", [0.0, 2.5])
def test_features_against_the_cpu_oracle(data, small, scale):
    ds, batch, flips = data
    sets = [(1, 4), ALL]
    for region, (start, lengths) in ZOOMS.items():
        fl = flips if region == 0 else None
        lg, feats = small.perturbation_scan_fine(*_args(batch), region=region, scale=scale, start=start, lengths=lengths, mark_sets=sets, flip=fl,
                                                 return_feats=True, **KW)
        ref, _, kinds = fo.fine_rows(batch, region=region, scale=scale, start=start, lengths=lengths, mark_sets=sets, flip=fl, **KW)
        assert lg.shape == (3, 15, 2) and int(sum((kinds[b] == fo.PART).sum() for b in BINS)) > 20
        worst = ratio = 0.0
        for b in BINS:
            got = feats[b].cpu()
            assert not torch.isnan(got).any()
            src = _src(batch, region, b)[:, None].expand_as(got)
            assert torch.equal(got[:, 0], src[:, 0])
            assert bool(((got != src) <= (kinds[b] != fo.NONE)[..., None]).all())      # rows nobody covers keep their bits
            err = (got.double() - ref[b].double()).abs()
            part = (kinds[b] == fo.PART)[..., None].expand_as(err)
            fac = fo.partial_bound_factor(src, ref[b], kinds[b])
            worst = max(worst, err[~part].max().item())
            if part.any():
                ratio = max(ratio, (err[part] / (2.0 ** -24 * fac[part])).max().item())
            assert bool((err <= torch.where(part, PART_C * 2.0 ** -24 * fac, torch.full_like(fac, WHOLE_TOL))).all()), (region, b)
        print("region %d s %g: wholly covered %.3e (bound %.1e), partly covered ratio %.3f (bound %.2f)" % (region, scale, worst, WHOLE_TOL, ratio, PART_C))
    # lengths = None: every real finest bin is full
    start, lengths = ZOOMS[1]
    a, fa = small.perturbation_scan_fine(*_args(batch), region=1, scale=scale, start=start, mark_sets=sets, return_feats=True, **KW)
    b_, fb = small.perturbation_scan_fine(*_args(batch), region=1, scale=scale, start=start, lengths=[12300, 1800, -5], mark_sets=sets, return_feats=True, **KW)
    assert torch.equal(a, b_) and all(torch.equal(fa[b], fb[b]) for b in BINS)


@pytest.mark.parametrize("regression", [False, True], ids=["classifier", "regressor"])
def test_logits_against_the_oracle(data, regression):
    ds, batch, flips = data
    P = orc.init_params(None, 42, regression)
    model = _model(None, regression, P, 4)
    for region, (start, lengths) in ZOOMS.items():
        fl = flips if region == 0 else None
        kw = dict(region=region, scale=0.0, start=start, lengths=lengths, mark_sets=[ALL, (2, 5)], flip=fl, **KW)
        got = model.perturbation_scan_fine(*_args(batch), **kw).cpu()
        vs = [0, 1, 3, 7, 8, 14]
        ora, _, _ = fo.oracle_fine(P, batch, variants=vs, **kw)
        d = (got[:, vs] - ora).abs().max().item()
        print("region", region, "vs oracle %.2e" % d)
        assert got.shape == (3, 15, 1 if regression else 2) and d < TOL, (region, d)
        assert not torch.equal(got[:2, 1], got[:2, 0])


@pytest.mark.parametrize("regression", [False, True], ids=["classifier", "regressor"])
def test_logits_against_the_golden(data, regression):
    """The reference's dataset and seed-42 models on raw files scaled inside fine windows (tests/golden/make_fine_scan_goldens.py)."""
    import os

    from tests.helpers import GOLDEN
    ds, batch, flips = data
    model = _model(None, regression, orc.init_params(None, 42, regression), 4)
    z = np.load(os.path.join(GOLDEN, "fine_scan.npz"))
    assert [str(g) for g in z["genes"]] == GENES and int(z["w_prom"]) == 39000 and len(z["cases"]) == 6
    for k, (region, lo, hi, scale) in enumerate(z["cases"].tolist()):
        region, lo, hi = int(region), int(lo), int(hi)
        marks = tuple(np.flatnonzero(z["marks"][k]).tolist())
        got = model.perturbation_scan_fine(*_args(batch), region=region, scale=scale, width=hi - lo, start=lo, n_windows=1, mark_sets=[marks],
                                           lengths=z["lengths"][k].tolist(), flip=flips if region == 0 else None).cpu()
        gold = torch.from_numpy(z["reg" if regression else "clf"][k])
        d = (got - gold).abs().max().item()
        print("case", k, "vs golden %.2e" % d)
        assert got.shape == gold.shape and d < TOL, (k, d)


def test_rows_are_the_plain_forward_bit_for_bit(data, small):
    ds, batch, flips = data
    for region, (start, lengths) in ZOOMS.items():
        fl = flips if region == 0 else None
        lg, feats = small.perturbation_scan_fine(*_args(batch), region=region, scale=0.5, start=start, lengths=lengths, flip=fl, return_feats=True,
                                                 width=7, stride=3, n_windows=3)
        lg = lg.cpu()
        assert lg.shape == (3, 25, 2)
        for v in (0, 1, 3, 22, 23, 24):
            with torch.no_grad():
                ref = small(*_args(_with_region(batch, region, feats, v))).cpu()
            assert torch.equal(lg[:, v], ref), (region, v)


@pytest.mark.parametrize("w", [1, 3])
def test_whole_coarse_bins_are_the_coarse_scan_bit_for_bit(data, small, w):
    ds, batch, flips = data
    sets = [ALL, (3,)]
    n_win = -(-20 // w)
    for region, fl in ((0, flips), (0, None), (1, None), (1, [False, True, True])):
        coarse, cfeats = small.perturbation_scan(*_args(batch), region=region, scale=2.5, width=w, mark_sets=sets, flip=fl, return_feats=True)
        fine, ffeats = small.perturbation_scan_fine(*_args(batch), region=region, scale=2.5, width=20 * w, stride=20 * w, mark_sets=sets, flip=fl,
                                                    return_feats=True)
        assert fine.shape == (3, 1 + 2 * n_win, 2)
        pick = [0] + [1 + k * 20 + g * w for k in range(2) for g in range(n_win)]
        assert torch.equal(fine, coarse[:, pick]), (region, fl)
        assert all(torch.equal(ffeats[b], cfeats[b][:, pick]) for b in BINS), (region, fl)


def test_dead_windows_empty_sets_and_dummy_slots_are_the_baseline(data, small):
    ds, batch, flips = data
    with torch.no_grad():
        base = small(*_args(batch)).cpu()
    sets = [ALL, (), (3,)]
    # pCRE slot 0 has 123 / 18 / 0 real finest bins: windows of width 5 from bin 110 at stride 10
    lg = small.perturbation_scan_fine(*_args(batch), region=1, scale=0.0, width=5, stride=10, start=110, n_windows=4, mark_sets=sets).cpu()
    assert torch.equal(lg[:, 0], base)
    scan = lg[:, 1:].reshape(3, 3, 4, 2)
    live = [2, 0, 0]
    for i in range(3):
        assert bool((scan[i, :, live[i]:] == base[i]).all()), i
        assert bool((scan[i, 1] == base[i]).all()), i
        if live[i]:
            assert bool((scan[i, 0, :live[i]] != base[i]).any(-1).all()), i
    last = small.perturbation_scan_fine(*_args(batch), region=8, scale=0.0, width=40, n_windows=3).cpu()
    assert torch.equal(last[2], base[2:3].expand(25, 2))      # slot 7: a dummy for the gene without partners
    prom = small.perturbation_scan_fine(*_args(batch), region=0, scale=0.0, width=3, start=[390, 400, 2 ** 31 - 1], n_windows=5, stride=2 ** 30,
                                        mark_sets=[ALL], flip=flips).cpu()
    assert torch.equal(prom, base[:, None].expand(3, 6, 2))      # past the 390 real bins, and past the int range


def test_per_gene_start_is_the_scalar_start_of_each_gene(data, small):
    ds, batch, flips = data
    start = [371, 0, 17]
    kw = dict(region=0, scale=0.0, flip=flips, mark_sets=[ALL, (1,)], return_feats=True, **KW)
    got, gf = small.perturbation_scan_fine(*_args(batch), start=start, **kw)
    for i, s in enumerate(start):
        one, of = small.perturbation_scan_fine(*_args(batch), start=s, **kw)
        assert torch.equal(got[i], one[i]), i
        assert all(torch.equal(gf[b][i], of[b][i]) for b in BINS), i
    assert not torch.equal(got[0], small.perturbation_scan_fine(*_args(batch), start=0, **kw)[0][0])


def test_same_bits_for_every_max_batch_call_after_call_and_packed_forms(data, small):
    from chromoformer_amd.engine import Slot
    ds, batch, flips = data
    P = orc.init_params(None, 42, False)
    start, lengths = ZOOMS[0]
    kw = dict(region=0, scale=0.5, start=start, lengths=lengths, flip=flips, mark_sets=[ALL, (0, 6)], return_feats=True, **KW)
    ref, ref_f = small.perturbation_scan_fine(*_args(batch), **kw)
    ref, ref_f = ref.cpu(), {b: t.cpu() for b, t in ref_f.items()}
    again, _ = small.perturbation_scan_fine(*_args(batch), **kw)
    assert torch.equal(again.cpu(), ref)
    for cap in (7, 64):
        model = _model(None, False, P, cap)
        got, got_f = model.perturbation_scan_fine(*_args(batch), **kw)
        assert torch.equal(got.cpu(), ref), cap
        assert all(torch.equal(got_f[b].cpu(), ref_f[b]) for b in BINS), cap
    packed = small.pack_batch(batch)
    slot = Slot(small, 3).fill(small, batch)
    for p in (packed, slot):
        got, got_f = small.perturbation_scan_fine(p, **kw)
        assert torch.equal(got.cpu(), ref)
        assert all(torch.equal(got_f[b].cpu(), ref_f[b]) for b in BINS)
    start, lengths = ZOOMS[1]
    kw = dict(region=1, scale=2.0, start=start, lengths=lengths, **KW)
    pc = small.perturbation_scan_fine(*_args(batch), **kw)
    assert torch.equal(_model(None, False, P, 64).perturbation_scan_fine(*_args(batch), **kw).cpu(), pc.cpu())


SHAPES = {
    "bins_2000_1000_500": dict(binsizes=[2000, 1000, 500], w_max=40000),
    "embed_2_layers": dict(embed=dict(n_layers=2, n_heads=2, d_model=128, d_ff=128)),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_other_shapes_against_the_oracle(name):
    """s = 2.5: the features of orc.synthetic_batch are drawn per resolution, not binned from one signal, and only s >= 1 keeps
    1 + m' > 0 on them."""
    cfg = orc._cfg(SHAPES[name])
    bins = tuple(cfg["binsizes"])
    R = max(bins) // min(bins)
    batch = orc.synthetic_batch(2, cfg=cfg, seed=13, regime="realistic")
    P = orc.init_params(cfg, 3, False)
    model = _model(cfg, False, P, 5)
    for region, fl in ((0, [True, False]), (2, None)):
        kw = dict(region=region, scale=2.5, width=R + 1, stride=R - 1, start=[1, R], n_windows=6, mark_sets=[(0, 6), ALL], flip=fl)
        got, feats = model.perturbation_scan_fine(*_args(batch), return_feats=True, **kw)
        got = got.cpu()
        vs = [0, 1, 2, 6, 7, 12]
        ora, ofeats, kinds = fo.oracle_fine(P, batch, cfg, variants=vs, **kw)
        d = (got[:, vs] - ora).abs().max().item()
        df = max((feats[b].cpu()[:, vs] - ofeats[b]).abs().max().item() for b in bins)
        print(name, "region", region, "vs oracle %.2e, features %.2e" % (d, df))
        assert got.shape == (2, 13, 2) and d < TOL and df < 1e-6, (name, region, d, df)
        assert any((kinds[b] == fo.PART).any() for b in bins)
        with torch.no_grad():
            assert torch.equal(got[:, 0], model(*_args(batch)).cpu())
        v = 8
        with torch.no_grad():
            assert torch.equal(got[:, v], model(*_args(_with_region(batch, region, feats, v, bins))).cpu())


def test_launch_contract_and_refusals(data):
    ds, batch, flips = data
    P = orc.init_params(None, 42, False)
    L = _lib.lib()
    for cap, chunks in ((64, 2), (7, 5)):                                  # B * V = 3 * (1 + 3 * 9) = 84 rows; 3 * 11 = 33 rows
        model = _model(None, False, P, cap)
        with torch.no_grad():
            model(*_args(batch))
        n_fwd = model.launch_counts()[0]
        sets, nw = ([ALL, (0,), (1,)], 9) if cap == 64 else ([ALL], 10)
        model.perturbation_scan_fine(*_args(batch), region=0, mark_sets=sets, n_windows=nw, lengths=[39000] * 3)
        assert -(-3 * (1 + len(sets) * nw) // cap) == chunks
        assert model.launch_counts()[0] == chunks * (1 + n_fwd), (cap, model.launch_counts()[0], n_fwd)
    model = _model(None, False, P, 4)
    bs, keep = model.pack_batch(batch)
    st = torch.cuda.current_stream().cuda_stream
    out = torch.full((3, 3, 2), float("nan"), device="cuda")
    one = (C.c_uint * 1)(0x7f)
    f0 = model.launch_counts()[0]

    def ints(*v):
        return C.cast((C.c_int * len(v))(*v), C.c_void_p)

    def call(h=model._handle, b=bs, lg=out, no_opts=False, **kw):
        o = _lib.cf_scan_fine_opts()
        o.region, o.n_sets, o.scale, o.width, o.stride, o.n_windows = 0, 1, 0.0, 1, 1, 2
        o.mark_sets = C.cast(one, C.c_void_p)
        for k, v in kw.items():
            setattr(o, k, v)
        return L.cf_perturbation_scan_fine(h, C.byref(b) if b is not None else None, None if no_opts else C.byref(o),
                                           lg.data_ptr() if lg is not None else None, st)

    big = _lib.cf_batch.from_buffer_copy(bs)
    big.B = 5
    bit7 = (C.c_uint * 2)(0x01, 0x80)
    cases = [(dict(h=None), b"null handle"), (dict(b=None), b"null batch"), (dict(no_opts=True), b"null opts"), (dict(lg=None), b"null logits"),
             (dict(mark_sets=None), b"null mark_sets"), (dict(b=big), b"max_batch"), (dict(region=-1), b"region"), (dict(region=9), b"region"),
             (dict(width=0), b"width"), (dict(stride=0), b"stride"), (dict(n_windows=0), b"n_windows"), (dict(n_sets=0), b"n_sets"),
             (dict(scale=-0.5), b"scale"), (dict(scale=float("inf")), b"scale"), (dict(scale=float("nan")), b"scale"),
             (dict(n_sets=2, mark_sets=C.cast(bit7, C.c_void_p)), b"n_feats"), (dict(start=ints(0, -1, 0)), b"start[1]"),
             (dict(lengths=ints(39000, 38900, 39000)), b"lengths[1]"), (dict(lengths=ints(39001, 39000, 39000)), b"lengths[0]"),
             (dict(region=1, lengths=ints(12201, 1700, 0)), b"lengths[1]"), (dict(lengths=ints(39000, 39000, 0)), b"lengths[2]")]
    for kw, msg in cases:
        assert call(**kw) != 0, kw
        err = L.cf_last_error()
        assert msg in err and b"cf_perturbation_scan_fine" in err, (kw, err)
    # bin counts that do not nest (20 / 50 / 400)
    cfg = orc._cfg(dict(binsizes=[2000, 800, 100], w_max=40000))
    odd = _model(cfg, False, orc.init_params(cfg, 3, False), 4)
    ob, okeep = odd.pack_batch(orc.synthetic_batch(2, cfg=cfg, seed=13, regime="realistic"))
    assert call(h=odd._handle, b=ob) != 0 and b"multiple" in L.cf_last_error() and b"cf_perturbation_scan_fine" in L.cf_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and model.launch_counts()[0] == f0      # nothing was launched
    assert call(lengths=ints(39000, 39000, 38901), region=0) == 0, L.cf_last_error()      # (38900, 39000] is accepted
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any())
    out.fill_(float("nan"))
    # armed riders (a training step in flight): refused; the handle is not used again
    assert L.cf_rider_arm(model._handle, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, 0, 8) == 0, L.cf_last_error()
    assert call() != 0 and b"riders" in L.cf_last_error() and b"cf_perturbation_scan_fine" in L.cf_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    for kw, match in ((dict(mark_sets=[(7,)]), "mark_sets"), (dict(start=[0, 1]), "start"), (dict(lengths=[1]), "lengths"), (dict(flip=[True]), "flip")):
        with pytest.raises(ValueError, match=match):      # (raised by the method before it calls the library)
            model.perturbation_scan_fine((bs, keep), **kw)
    del keep


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
            model.perturbation_scan_fine(*_args(batches[2]), region=0, scale=2.0, width=7, stride=3, n_windows=2, mark_sets=[ALL])
            model.perturbation_scan_fine(*_args(batches[2]), region=3, scale=2.0, width=30, n_windows=2, mark_sets=[(1,)], return_feats=True)
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
        lg = model.perturbation_scan_fine(*_args(batches[1]), scale=2.0, n_windows=1, mark_sets=[ALL])
        assert not lg.requires_grad
        with pytest.raises(RuntimeError, match="perturbation_scan_fine"):
            out[:, 1].sum().backward()
        model(*_args(b))[:, 1].sum().backward()      # a fresh forward trains as before
    # the C ABI itself refuses a backward without a new saving forward
    bs, keep = model.pack_batch(b)
    st = torch.cuda.current_stream().cuda_stream
    lgt = torch.empty(8, 2, device="cuda")
    _lib.check(_lib.lib().cf_forward(model._handle, C.byref(bs), lgt.data_ptr(), 1, st), "cf_forward")
    model.perturbation_scan_fine((bs, keep), scale=2.0, n_windows=1, mark_sets=[ALL])
    dl = torch.zeros(8, 2, device="cuda")
    assert _lib.lib().cf_backward_from(model._handle, C.byref(bs), dl.data_ptr(), st) != 0
    assert b"must follow cf_forward" in _lib.lib().cf_last_error()


def test_dataset_walker_with_zoom_and_cli(tmp_path):
    import pandas as pd

    from chromoformer_amd import ChromoformerClassifier, predict
    from chromoformer_amd.data import ChromoformerDataset
    from tests.synth_data import make_dataset
    npy = str(tmp_path / "npy")
    meta = make_dataset(npy, n_genes=20, seed=11)
    table = pd.read_csv(meta)
    P = orc.init_params(seed=7)
    ds = ChromoformerDataset(meta, npy, table.gene_id.tolist())
    model = ChromoformerClassifier(seed=123, max_batch=32).cuda(0)
    model.load_state_dict(P)
    genes = ds.target_genes[:5]
    batch = torch.utils.data.default_collate([ds[i] for i in range(5)])
    flips = [ds.genes[g]["tss"][2] != "+" for g in genes]
    # zoom = 1: the coarse scan, then ten windows of two finest bins inside each gene's most important coarse window
    coarse = model.perturbation_scan(*_args(batch), region=0, flip=flips).cpu().numpy()
    res = list(model.perturbation_scan_fine_dataset(ds, genes=genes, zoom=1, width=2, bsz=3))
    assert [d["gene_id"] for d in res] == genes
    top = []
    for i, d in enumerate(res):
        chrom, tss, _ = ds.genes[d["gene_id"]]["tss"]
        assert sorted(d) == ["coarse_scan", "coarse_windows", "gene_id", "logits", "mark_sets", "region", "scan", "windows", "zoom"]
        assert d["region"] == (chrom, tss - 20000, tss + 20000) and len(d["mark_sets"]) == 8
        assert d["coarse_scan"].shape == (8, 20, 2) and np.abs(d["coarse_scan"] - coarse[i, 1:].reshape(8, 20, 2)).max() <= 1e-6
        assert d["coarse_windows"][3] == (chrom, tss - 20000 + 6000, tss - 20000 + 8000)
        moved = np.abs(d["coarse_scan"][..., 1] - d["logits"][1]).max(axis=0)
        g = int(d["zoom"][0])
        assert d["zoom"].shape == (1,) and moved[g] == moved.max()
        top.append(g)
        assert d["windows"] == [(chrom, tss - 20000 + 2000 * g + 200 * k, tss - 20000 + 2000 * g + 200 * k + 200) for k in range(10)]
        assert d["scan"].dtype == np.float32 and d["scan"].shape == (8, 10, 2) and np.isfinite(d["scan"]).all()
    ref = model.perturbation_scan_fine(*_args(batch), region=0, width=2, start=[20 * g for g in top], n_windows=10, flip=flips).cpu().numpy()
    for i, d in enumerate(res):
        assert np.abs(d["scan"] - ref[i, 1:].reshape(8, 10, 2)).max() <= 1e-6 and np.abs(d["logits"] - ref[i, 0]).max() <= 1e-6
    # a pCRE slot, the whole region: a gene without the slot yields no window; the last window is clipped to the pCRE's end
    res = list(model.perturbation_scan_fine_dataset(ds, genes=genes, region="promoter", width=25, mark_sets=[ALL], bsz=5))
    res1 = list(model.perturbation_scan_fine_dataset(ds, genes=ds.target_genes, region=1, width=25, mark_sets=[ALL]))
    assert all(len(d["windows"]) == 16 for d in res)
    for d in res1:
        pc = ds.genes[d["gene_id"]]["pcres"]
        if len(pc) < 2:
            assert d["region"] is None and d["windows"] == [] and d["scan"].shape == (1, 0, 2)
        else:
            c, s, e = pc[1]
            assert d["region"] == (c, s, e) and len(d["windows"]) == -(-(e - s) // 2500) == d["scan"].shape[1]
            assert d["windows"][0][1] == s and d["windows"][-1][2] == e and np.isfinite(d["scan"]).all()
    assert any(d["region"] is None for d in res1) and any(d["region"] for d in res1)
    # the CLI
    ck = str(tmp_path / "w.pt")
    torch.save({"net": P}, ck)
    out = str(tmp_path / "fine.npz")
    base = ["-m", meta, "-d", npy, "-w", ck, "-o", str(tmp_path / "p.csv")]
    assert predict.main(base + ["--fine-scan-out", out, "--fine-scan-width", "5", "--fine-scan-zoom", "1"]) == 0
    z = np.load(out)
    assert sorted(z.files) == ["chroms", "coarse", "coarse_windows", "gene_ids", "mark_sets", "prediction", "scan", "windows", "zoom"]
    assert list(z["gene_ids"]) == table.gene_id.tolist() and z["mark_sets"].shape == (8, 7) and z["mark_sets"][7].all()
    assert z["scan"].shape == (20, 8, 4) and z["windows"].shape == (20, 4, 2) and z["coarse"].shape == (20, 8, 20) and z["zoom"].shape == (20, 1)
    assert np.isfinite(z["scan"]).all() and np.isfinite(z["coarse"]).all()
    assert np.array_equal(z["windows"][:, 0, 0], z["coarse_windows"][np.arange(20), z["zoom"][:, 0], 0])
    assert np.abs(pd.read_csv(str(tmp_path / "p.csv"))["prediction"].to_numpy().astype(np.float32) - z["prediction"]).max() <= 1e-6
    sig = 1 / (1 + np.exp(-res[0]["logits"][1].astype(np.float64)))
    assert abs(sig - z["prediction"][0]) <= 1e-6
    for argv in (["--fine-scan-width", "2"], ["--fine-scan-out", out, "--fine-scan-width", "0"], ["--fine-scan-out", out, "--fine-scan-region", "9"],
                 ["--fine-scan-out", out, "--fine-scan-scale", "-1"], ["--fine-scan-out", out, "--fine-scan-zoom", "0"]):
        with pytest.raises(SystemExit) as e:
            predict.main(base + argv)
        assert e.value.code == 2, argv
