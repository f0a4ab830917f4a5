"""Perturbation scan of several regions per call on the GPU (cf_perturbation_scan_regions, model.perturbation_scan_regions, the
dataset generator and predict --scan-out --scan-regions all on top of it).  The contract: block q of the call carries, bit for bit,
what cf_perturbation_scan writes for that region -- although the variants of a pCRE slot run slot-packed, i_max of them per trunk pass.

  * blocks against model.perturbation_scan per region, bit for bit; against the CPU oracle at the project's logits bound;
  * other model shapes (the stand-alone kernels, k_attc2, the all-rows Embedding, Regulation layer by layer);
  * the same bits whatever max_batch is, call after call, for the packed forms, and with CF_SCAN_PACK=0;
  * the launch contract of the header: a pCRE region issues P = ceil(B U / max_batch) trunk passes, not C = ceil(B V / max_batch);
  * every refusal by name with nothing launched; no side effects on training; the dataset generator and the CLI.

The three genes of tests/test_perturbation_scan_gpu.py at w_prom = 39000: a mirrored promoter, a 12,201-sample pCRE, an 1,800-sample
pCRE, a gene without partners whose slots are all dummies."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest
import torch

from chromoformer_amd import _lib
from oracle import chromoformer_oracle as orc
from tests import scan_oracle as so
from tests.test_input_grads_gpu import _model
from tests.test_perturbation_scan_gpu import ALL, GENES, SHAPES, TOL, W

pytestmark = pytest.mark.gpu
S = 8


def _args(batch):
    return tuple(batch[k] for k in so.KEYS)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """-> (the three genes' batch, their promoter flips): built once, shared, never written."""
    ds = so.scan_dataset(str(tmp_path_factory.mktemp("scan_regions")), w_prom=39000)
    assert ds.genes[GENES[0]]["tss"][2] == "-" and not ds.genes[GENES[2]]["pcres"]
    return so.dataset_batch(ds, GENES), [ds.genes[g]["tss"][2] != "+" for g in GENES]


@pytest.fixture(scope="module")
def small():
    """The seed-42 classifier at max_batch = 4."""
    return _model(None, False, orc.init_params(None, 42, False), 4)


def _per_region(model, args, regions, flip, **kw):
    """The blocks assembled from one model.perturbation_scan per region (flips for the promoter alone)."""
    return torch.stack([model.perturbation_scan(*args, region=r, flip=flip if r == 0 else None, **kw) for r in regions])


@pytest.mark.parametrize("sets", [[(1, 4), ALL], [ALL]], ids=["two_sets_full_pseudo_genes", "one_set_half_full_last"])
@pytest.mark.parametrize("scale,width", [(0.0, 1), (2.0, 1), (0.0, 2), (2.0, 2)])
def test_blocks_equal_the_per_region_call_bit_for_bit(data, small, sets, scale, width):
    """max_batch = 4.  Two sets: 40 variants per gene, 5 full pseudo-genes each, 15 pseudo rows in chunks of 4 that straddle genes.
    One set: 20 variants, the third pseudo-gene of every gene half full."""
    batch, flips = data
    kw = dict(scale=scale, width=width, mark_sets=sets)
    got, regions = small.perturbation_scan_regions(*_args(batch), regions="all", flip=flips, **kw)
    V = 1 + len(sets) * W
    assert regions == list(range(S + 1)) and got.shape == (S + 1, 3, V, 2)
    ref = _per_region(small, _args(batch), regions, flips, **kw)
    for q in regions:
        assert torch.equal(got[q], ref[q]), (q, (got[q] - ref[q]).abs().max().item())
    got = got.cpu()
    with torch.no_grad():
        base = small(*_args(batch)).cpu()
    assert torch.equal(got[:, :, 0], base[None].expand(S + 1, 3, 2))                     # row 0 of every block: the unperturbed gene
    assert torch.equal(got[1:, 2], base[2].expand(S, V, 2))                              # the gene whose slots are all dummies
    v_all = 1 + (len(sets) - 1) * W                                                      # all marks over window 0
    assert not torch.equal(got[1, 0, v_all], base[0]) and not torch.equal(got[1, 1, v_all], base[1])      # ... while real windows move the logits
    unflipped = small.perturbation_scan(*_args(batch), region=0, **kw).cpu()
    assert not torch.equal(got[0, 0], unflipped[0])                                      # the promoter block did take the flips


@pytest.mark.parametrize("regression", [False, True], ids=["classifier", "regressor"])
def test_blocks_against_the_oracle(data, regression):
    batch, flips = data
    P = orc.init_params(None, 42, regression)
    model = _model(None, regression, P, 4)
    sets = [ALL]
    regions = [0, 1, 2]
    got, named = model.perturbation_scan_regions(*_args(batch), regions=regions, scale=0.0, mark_sets=sets, flip=flips)
    assert named == regions and got.shape == (3, 3, 1 + W, 1 if regression else 2)
    vs = [0, 1, 1 + 3, 1 + 6, W]
    for q, region in enumerate(regions):
        ora, _ = so.oracle_scan(P, batch, region=region, scale=0.0, width=1, mark_sets=sets, flip=flips if region == 0 else None, variants=vs)
        d = (got[q].cpu()[:, vs] - ora).abs().max().item()
        print("region %d vs oracle %.2e" % (region, d))
        assert d < TOL, (region, d)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_other_shapes_bit_for_bit_and_against_the_oracle(name):
    """max_batch = 5, two genes, 40 variants per gene.  At i_max16 the 40 variants fill 2.5 pseudo-genes of 16 slots and k_attc2 runs."""
    over, regression = SHAPES[name]
    cfg = orc._cfg(over)
    batch = orc.synthetic_batch(2, cfg=cfg, seed=13, regime="realistic")
    P = orc.init_params(cfg, 3, regression)
    model = _model(cfg, regression, P, 5)
    kw = dict(scale=0.0, width=2, mark_sets=[(0, 6), ALL])
    fl = [True, False]
    got, regions = model.perturbation_scan_regions(*_args(batch), regions="all", flip=fl, **kw)
    assert regions == list(range(cfg["i_max"] + 1)) and got.shape == (len(regions), 2, 1 + 2 * W, 1 if regression else 2)
    ref = _per_region(model, _args(batch), regions, fl, **kw)
    for q in regions:
        assert torch.equal(got[q], ref[q]), (name, q, (got[q] - ref[q]).abs().max().item())
    vs = [0, 1, 1 + 9, 1 + W + 4, 2 * W]
    for region in (0, 2):
        ora, _ = so.oracle_scan(P, batch, cfg, region=region, variants=vs, flip=fl if region == 0 else None, **kw)
        d = (got[region].cpu()[:, vs] - ora).abs().max().item()
        print(name, "region", region, "vs oracle %.2e" % d)
        assert d < TOL, (name, region, d)


def test_same_bits_for_every_max_batch_call_after_call_packed_forms_and_unpacked_path(data, small, monkeypatch):
    from chromoformer_amd.engine import Slot
    batch, flips = data
    P = orc.init_params(None, 42, False)
    kw = dict(regions="all", scale=0.5, width=2, mark_sets=[(1, 4), (), ALL], flip=flips)
    ref, _ = small.perturbation_scan_regions(*_args(batch), **kw)
    ref = ref.cpu()
    again, _ = small.perturbation_scan_regions(*_args(batch), **kw)
    assert torch.equal(again.cpu(), ref)
    assert torch.equal(ref[:, :, 1 + W:1 + 2 * W], ref[:, :, :1].expand(S + 1, 3, W, 2))      # the empty set: the baseline
    for cap in (7, 64):
        got, _ = _model(None, False, P, cap).perturbation_scan_regions(*_args(batch), **kw)
        assert torch.equal(got.cpu(), ref), cap
    for p in (small.pack_batch(batch), Slot(small, 3).fill(small, batch)):
        got, _ = small.perturbation_scan_regions(p, **kw)
        assert torch.equal(got.cpu(), ref)
    monkeypatch.setenv("CF_SCAN_PACK", "0")      # (read at cf_create)
    unpacked = _model(None, False, P, 4)
    monkeypatch.delenv("CF_SCAN_PACK")
    got, _ = unpacked.perturbation_scan_regions(*_args(batch), **kw)
    assert torch.equal(got.cpu(), ref)
    few, named = small.perturbation_scan_regions(*_args(batch), regions=[5, 1], scale=0.5, width=2, mark_sets=[(1, 4), (), ALL])
    assert named == [1, 5] and torch.equal(few.cpu(), ref[[1, 5]])
    pcres, named = small.perturbation_scan_regions(*_args(batch), regions="pcres", scale=0.5, width=2, mark_sets=[(1, 4), (), ALL])
    assert named == list(range(1, S + 1)) and torch.equal(pcres.cpu(), ref[1:])


@pytest.mark.parametrize("cap", [64, 7])
def test_launch_contract(data, cap, monkeypatch):
    """B = 3, one mark set: V = 21, U = ceil(20 / 8) = 3.  cap 64: C = P = 1; cap 7: C = 9, P = 2 -- a pCRE region issues P trunk passes."""
    batch, flips = data
    P_ = orc.init_params(None, 42, False)
    B, V, U, n_reg_head = 3, 1 + W, -(-W // S), 2
    Cn, Pn = -(-B * V // cap), -(-B * U // cap)
    assert (Cn, Pn) == {64: (1, 1), 7: (9, 2)}[cap]
    model = _model(None, False, P_, cap)
    with torch.no_grad():
        model(*_args(batch))
    n_fwd = model.launch_counts()[0]
    n_trunk = n_fwd - n_reg_head
    for regions in ([0], [3], list(range(S + 1))):
        n_p, n_c = int(0 in regions), len([r for r in regions if r])
        model.perturbation_scan_regions(*_args(batch), regions=regions, mark_sets=[ALL], flip=flips)
        want = n_p * Cn * (1 + n_fwd) + (n_c > 0) * (n_trunk + 1) + n_c * (Pn * (n_trunk + 2) + Cn * (1 + n_reg_head))
        assert model.launch_counts()[0] == want, (cap, regions, model.launch_counts()[0], want, n_fwd)
    monkeypatch.setenv("CF_SCAN_PACK", "0")      # (read at cf_create)
    unpacked = _model(None, False, P_, cap)
    monkeypatch.delenv("CF_SCAN_PACK")
    for regions in ([0], [3], list(range(S + 1))):
        unpacked.perturbation_scan_regions(*_args(batch), regions=regions, mark_sets=[ALL], flip=flips)
        assert unpacked.launch_counts()[0] == len(regions) * Cn * (1 + n_fwd), (cap, regions)


def test_refusals_by_name_with_nothing_launched(data):
    batch, flips = data
    P = orc.init_params(None, 42, False)
    L = _lib.lib()
    model = _model(None, False, P, 4)
    bs, keep = model.pack_batch(batch)
    st = torch.cuda.current_stream().cuda_stream
    out = torch.full((S + 1, 3, 1 + W, 2), float("nan"), device="cuda")
    one = (C.c_uint * 1)(0x7f)
    with torch.no_grad():
        model(*_args(batch))
    f0 = model.launch_counts()[0]

    def call(h=model._handle, b=bs, lg=out, no_opts=False, **kw):
        o = _lib.cf_scan_regions_opts()
        o.regions, o.width, o.n_sets, o.scale = 0x1ff, 1, 1, 0.0
        o.mark_sets = C.cast(one, C.c_void_p)
        for k, v in kw.items():
            setattr(o, k, v)
        return L.cf_perturbation_scan_regions(h, C.byref(b) if b is not None else None, None if no_opts else C.byref(o),
                                              lg.data_ptr() if lg is not None else None, st)

    big = _lib.cf_batch.from_buffer_copy(bs)
    big.B = 5
    bit7 = (C.c_uint * 2)(0x01, 0x80)
    cases = [(dict(h=None), b"null handle"), (dict(b=None), b"null batch"), (dict(no_opts=True), b"null opts"), (dict(lg=None), b"null logits"),
             (dict(mark_sets=None), b"null mark_sets"), (dict(b=big), b"max_batch"), (dict(regions=0), b"regions = 0"),
             (dict(regions=1 << 9), b"i_max"), (dict(regions=0x3ff), b"i_max"), (dict(regions=1 << 31), b"i_max"),
             (dict(width=0), b"width"), (dict(n_sets=0), b"n_sets"), (dict(scale=-0.5), b"scale"), (dict(scale=float("inf")), b"scale"),
             (dict(scale=float("nan")), b"scale"), (dict(n_sets=2, mark_sets=C.cast(bit7, C.c_void_p)), b"n_feats")]
    for kw, msg in cases:
        assert call(**kw) != 0, kw
        err = L.cf_last_error()
        assert msg in err and b"cf_perturbation_scan_regions" in err, (kw, err)
    cfg = orc._cfg(dict(binsizes=[2000, 800, 100], w_max=40000))      # a bin count that is no multiple of the smallest
    odd = _model(cfg, False, orc.init_params(cfg, 3, False), 4)
    ob, okeep = odd.pack_batch(orc.synthetic_batch(2, cfg=cfg, seed=13, regime="realistic"))
    assert call(h=odd._handle, b=ob) != 0 and b"multiple" in L.cf_last_error() and b"cf_perturbation_scan_regions" in L.cf_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and model.launch_counts()[0] == f0      # nothing was launched
    # armed riders (a training step in flight): refused; the handle is not used again
    assert L.cf_rider_arm(model._handle, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, 0, 8) == 0, L.cf_last_error()
    assert call() != 0 and b"riders" in L.cf_last_error() and b"cf_perturbation_scan_regions" in L.cf_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and model.launch_counts()[0] == f0
    fresh = _model(None, False, P, 4)
    for bad in ("some", [], [9], [-1]):      # (raised by the method before it calls the library)
        with pytest.raises(ValueError, match="regions"):
            fresh.perturbation_scan_regions(*_args(batch), regions=bad)
    with pytest.raises(ValueError, match="mark_sets"):
        fresh.perturbation_scan_regions(*_args(batch), mark_sets=[(7,)])
    with pytest.raises(ValueError, match="flip"):
        fresh.perturbation_scan_regions(*_args(batch), flip=[True])
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
            model.perturbation_scan_regions(*_args(batches[2]), regions="all", mark_sets=[ALL])
            model.perturbation_scan_regions(*_args(batches[2]), regions=[3], scale=2.0, mark_sets=[(1,)])
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
        lg, _ = model.perturbation_scan_regions(*_args(batches[1]), regions=[0, 2], mark_sets=[ALL])
        assert not lg.requires_grad
        with pytest.raises(RuntimeError, match="perturbation_scan_regions"):
            out[:, 1].sum().backward()
        model(*_args(b))[:, 1].sum().backward()      # a fresh forward trains as before
    # the C ABI itself refuses a backward without a new saving forward, after the packed path and after the promoter path
    bs, keep = model.pack_batch(b)
    st = torch.cuda.current_stream().cuda_stream
    lgt = torch.empty(8, 2, device="cuda")
    dl = torch.zeros(8, 2, device="cuda")
    for regions in ([2], [0]):
        _lib.check(_lib.lib().cf_forward(model._handle, C.byref(bs), lgt.data_ptr(), 1, st), "cf_forward")
        model.perturbation_scan_regions((bs, keep), regions=regions, mark_sets=[ALL])
        assert _lib.lib().cf_backward_from(model._handle, C.byref(bs), dl.data_ptr(), st) != 0
        assert b"must follow cf_forward" in _lib.lib().cf_last_error()


def _spy(monkeypatch, model_cls, calls):
    """model.perturbation_scan_regions checked, call by call and on the very inputs of the call, against one perturbation_scan per
    region; `calls` collects (regions, the blocks assembled from the per-region calls)."""
    real = model_cls.perturbation_scan_regions

    def checked(self, *args, regions="all", scale=0.0, width=1, mark_sets=None, flip=None):
        got, named = real(self, *args, regions=regions, scale=scale, width=width, mark_sets=mark_sets, flip=flip)
        ref = _per_region(self, args, named, flip, scale=scale, width=width, mark_sets=mark_sets)
        assert torch.equal(got, ref), named
        calls.append((named, ref.cpu()))
        return got, named

    monkeypatch.setattr(model_cls, "perturbation_scan_regions", checked)


def test_dataset_generator_and_cli_equal_the_per_region_assembly(tmp_path, monkeypatch):
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
    calls = []
    _spy(monkeypatch, ChromoformerClassifier, calls)
    assert predict.main(["-m", meta, "-d", npy, "-w", ck, "-o", str(tmp_path / "p.csv"), "--scan-out", out, "--scan-regions", "all"]) == 0
    z = np.load(out)
    assert len(calls) == 1 and calls[0][0] == list(range(S + 1))      # 20 genes, one batch, one call
    lg = calls[0][1]                                                   # [9, 20, 161, 2] from nine perturbation_scan calls
    vals = np.stack([np.stack([torch.sigmoid(lg[k, :, v].contiguous()).numpy()[:, 1] for v in range(lg.shape[2])], axis=1) for k in range(S + 1)])
    scan = vals[:, :, 1:].reshape(S + 1, 20, 8, W)
    ds = ChromoformerDataset(meta, npy, table.gene_id.tolist())
    assert np.array_equal(z["prediction"], vals[0, :, 0]) and np.array_equal(z["promoter"], scan[0])
    for i, gid in enumerate(ds.target_genes):
        pc = ds.genes[gid]["pcres"]
        for s in range(S):
            n_win = -(-(pc[s][2] - pc[s][1]) // 2000) if s < len(pc) else 0
            assert np.array_equal(z["pcres"][i, s, :, :n_win], scan[1 + s, i, :, :n_win]), (gid, s)
            assert np.isnan(z["pcres"][i, s, :, n_win:]).all(), (gid, s)
    # the generator: chunks of 3 genes, one call per chunk over the slots some gene of the chunk has
    model = ChromoformerClassifier(seed=123, max_batch=32).cuda(0)
    model.load_state_dict(P)
    genes = ds.target_genes[:5]
    del calls[:]
    res = list(model.perturbation_scan_dataset(ds, genes=genes, regions="all", bsz=3))
    assert [d["gene_id"] for d in res] == genes and len(calls) == 2
    for i, d in enumerate(res):
        named, blocks = calls[i // 3]
        blocks = blocks.numpy()
        n_pc = len(ds.genes[d["gene_id"]]["pcres"])
        assert len(d["scan"]) == 1 + n_pc and set(range(1 + n_pc)) <= set(named)
        assert np.array_equal(d["logits"], blocks[0, i % 3, 0])
        for region, sc in enumerate(d["scan"]):
            q = named.index(region)
            assert np.array_equal(sc, blocks[q, i % 3, 1:].reshape(8, W, -1)[:, :sc.shape[1]]), (d["gene_id"], region)
