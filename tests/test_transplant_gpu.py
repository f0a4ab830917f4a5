"""pCRE transplant screen on the GPU (cf_pcre_transplant, chromoformer_amd.transplant, predict --transplant-out):

  * row (b, 1 + c Q + q) is model(...) on the tensors tests/transplant_oracle.py edits, bit for bit, and row (b, 0) is model(...);
    explicit slots and "append", a gene without a free slot, the identities of the rule;
  * other model shapes against model(...) and the CPU oracle; the same bits whatever max_batch is, call after call, for the packed
    forms; the reference's golden cases end to end;
  * the launch contract, every refusal by name, no side effects on training, the dataset generator and the CLI.

Three genes of the 20-gene synthetic dataset read at w_prom = 39000 (those of tests/test_perturbation_scan_gpu.py): a '-' strand gene
whose promoter is stored mirrored and whose first pCRE has 12,201 samples, a '+' strand gene with an 1,800-sample pCRE -- both with all
eight slots live -- and a gene whose slots are all dummies.  C = 11 candidates (a 12,201-sample, an 1,800-sample and one without a
real bin among them), Q = 2: 23 rows per gene, at max_batch = 4 the 69 rows run in 18 chunks, genes straddling them, and the 6 pseudo
rows (U = 2, the second pseudo-gene holding 3 candidates and 5 dummies) in 2."""
import ctypes as C
import os

import numpy as np
import pandas as pd
import pytest
import torch

from chromoformer_amd import _lib
from chromoformer_amd import transplant as tp
from oracle import chromoformer_oracle as orc
from tests import scan_oracle as so
from tests import transplant_oracle as to
from tests.helpers import GOLDEN
from tests.test_input_grads_gpu import _model
from tests.test_perturbation_scan_gpu import GENES, SHAPES
from tests.transplant_cases import choose_cases

pytestmark = pytest.mark.gpu
BINS = (2000, 500, 100)
TOL = 1e-4
FREQ = torch.tensor([2.5, 0.75])


def _args(batch):
    return tuple(batch[k] for k in to.KEYS)


def _cols(lib):
    return {b: m.bool() for b, m in lib.mask_rows.items()}


def _model_rows(model, batch, lib, freq, slots, variants=None):
    """model(...) on the oracle-edited batch of the same B genes, per (c, q) -> [B, nv, n_out] on the host."""
    Cn, Q = freq.shape[1], freq.shape[2]
    variants = [(c, q) for c in range(Cn) for q in range(Q)] if variants is None else variants
    out = []
    with torch.no_grad():
        for c, q in variants:
            out.append(model(*_args(to.edited_batch(batch, lib.feats, _cols(lib), c, freq, q, slots))).cpu())
    return torch.stack(out, 1)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """-> (dataset, the three genes' batch, the 11-candidate library): built once, shared, never written."""
    ds = so.scan_dataset(str(tmp_path_factory.mktemp("transplant")), w_prom=39000)
    batch = so.dataset_batch(ds, GENES)
    ids = ds.target_genes
    regions = [ds.genes[ids[1]]["pcres"][0], ds.genes[ids[0]]["pcres"][0]] + ds.genes[ids[3]]["pcres"][:4] + ds.genes[ids[7]]["pcres"] + [ds.genes[ids[9]]["pcres"][0]]
    real = tp.library_from_regions(ds, regions)
    assert len(real) == 10 and regions[0][2] - regions[0][1] == 12201 and regions[1][2] - regions[1][1] == 1800
    feats = {b: torch.cat([t, torch.zeros(1, *t.shape[1:])]) for b, t in real.feats.items()}          # ... and one without a real bin
    rows = {b: torch.cat([t, torch.ones(1, t.shape[1], dtype=torch.uint8)]) for b, t in real.mask_rows.items()}
    return ds, batch, tp.Library(feats, rows, real.names + ["empty"])


@pytest.fixture(scope="module")
def small():
    """The seed-42 classifier (the golden's weights) at max_batch = 4."""
    return _model(None, False, orc.init_params(None, 42, False), 4)


@pytest.fixture(scope="module")
def reference(data, small):
    """The explicit-slot call's reference rows, computed once: (slots, freq [3, 11, 2], model rows [3, 22, 2], base [3, 2])."""
    ds, batch, lib = data
    slots = [3, 0, 5]      # a live slot; slot 0 (the 1,800-sample pCRE, live); a dead slot past n_part = 0
    freq = tp.broadcast_freq(FREQ, 3, len(lib))
    freq[1] *= 2.0         # (per-gene frequencies)
    with torch.no_grad():
        base = small(*_args(batch)).cpu()
    return slots, freq, _model_rows(small, batch, lib, freq, slots), base


def test_every_row_is_the_plain_forward_on_the_edited_tensors_explicit_slots(data, small, reference):
    ds, batch, lib = data
    slots, freq, ref, base = reference
    assert [len(ds.genes[g]["pcres"]) for g in GENES] == [8, 8, 0] and ds.genes[GENES[0]]["tss"][2] == "-"
    got, info = tp.pcre_transplant(small, *_args(batch), library=lib, freq=freq, slot=slots)
    assert got.shape == (3, 11, 2, 2) and not got.requires_grad
    assert info["slot"].tolist() == slots and info["placed"].tolist() == [True] * 3 and info["names"] == lib.names
    assert torch.equal(info["logits"].cpu(), base)
    got = got.cpu().reshape(3, 22, 2)
    for b in range(3):
        for v in range(22):
            assert torch.equal(got[b, v], ref[b, v]), (b, divmod(v, 2))
    assert bool((got != base[:, None]).any(-1).all())      # every transplant moves every gene's logits


def test_append_and_not_placed(data, small):
    ds, batch, lib = data
    freq = tp.broadcast_freq(FREQ, 3, len(lib))
    got, info = tp.pcre_transplant(small, *_args(batch), library=lib, freq=FREQ, slot="append")
    want = [to.append_slot(batch, g) for g in range(3)]
    assert want == [-1, -1, 0] and info["slot"].tolist() == want and info["placed"].tolist() == [False, False, True]
    got, base = got.cpu().reshape(3, 22, 2), info["logits"].cpu()
    ref = _model_rows(small, batch, lib, freq, want)
    assert torch.equal(got, ref)
    assert torch.equal(got[:2], base[:2, None].expand(2, 22, 2))      # the genes without a free slot: the baseline's bits
    mixed, info = tp.pcre_transplant(small, *_args(batch), library=lib, freq=FREQ, slot=[-1, 7, 0])
    assert info["slot"].tolist() == [-1, 7, 0] and torch.equal(mixed.cpu().reshape(3, 22, 2)[2], got[2])
    assert torch.equal(mixed.cpu().reshape(3, 22, 2)[0], got[0])


def test_append_on_a_full_gene_is_the_baseline():
    batch = orc.synthetic_batch(2, seed=5, regime="dense")      # every slot live
    model = _model(None, False, orc.init_params(None, 42, False), 4)
    lib = tp.library_from_batch(orc.synthetic_batch(2, seed=6, regime="realistic"), [(0, 0), (1, 0), (0, 1)])
    got, info = tp.pcre_transplant(model, *_args(batch), library=lib, freq=[1.0, 4.0], slot="append")
    with torch.no_grad():
        base = model(*_args(batch))
    assert info["slot"].tolist() == [-1, -1] and info["placed"].tolist() == [False, False]
    assert torch.equal(info["logits"], base) and torch.equal(got, base[:, None, None].expand(2, 3, 2, 2))


def test_identities_bit_for_bit(data, small, reference):
    ds, batch, lib = data
    slots, freq, ref, base = reference
    # a gene's own slot put back with its own frequency is the baseline
    for g, j in ((0, 3), (1, 0)):
        own = tp.library_from_batch(batch, [(g, j)])
        f = float(batch["interaction_freq"][g, 0, j + 1])
        got, info = tp.pcre_transplant(small, *_args(batch), library=own, freq=f, slot=[j if b == g else -1 for b in range(3)])
        assert torch.equal(got[:, 0, 0].cpu(), base) and torch.equal(info["logits"].cpu(), base), (g, j)
    # permuting the library permutes the rows; a repeated candidate or frequency gives equal rows
    perm = [4, 0, 10, 7, 1, 9, 2, 8, 3, 6, 5, 4]
    got, _ = tp.pcre_transplant(small, *_args(batch), library=lib.select(perm), freq=freq[:, perm], slot=slots)
    assert torch.equal(got.cpu(), ref.reshape(3, 11, 2, 2)[:, perm])
    assert torch.equal(got[:, 0], got[:, 11])
    rep, _ = tp.pcre_transplant(small, *_args(batch), library=lib.select([1, 0]), freq=[2.5, 0.75, 2.5], slot=slots[0])
    assert torch.equal(rep[:, :, 0], rep[:, :, 2]) and not torch.equal(rep[:, :, 0], rep[:, :, 1])
    # a candidate without a real bin is what a dummy slot holds: in a dead slot with the token live ... it still is a live token
    empty = lib.select([10])
    a, _ = tp.pcre_transplant(small, *_args(batch), library=empty, freq=1.5, slot=[-1, -1, 0])
    b = _model_rows(small, batch, empty, tp.broadcast_freq(1.5, 3, 1), [-1, -1, 0])
    assert torch.equal(a.cpu().reshape(3, 1, 2), b)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_other_shapes_against_the_forward_and_the_oracle(name):
    over, regression = SHAPES[name]
    cfg = orc._cfg(over)
    S = cfg["i_max"]
    batch = orc.synthetic_batch(2, cfg=cfg, seed=13, regime="realistic")
    P = orc.init_params(cfg, 3, regression)
    model = _model(cfg, regression, P, 5)
    Cn = 20 if S == 16 else 5
    src = orc.synthetic_batch(3, cfg=cfg, seed=14, regime="dense")
    lib = tp.library_from_batch(src, [(c % 3, (c * 5) % S) for c in range(Cn)])
    freq = tp.broadcast_freq(torch.tensor([[1.5 + 0.25 * c, 3.0] for c in range(Cn)]), 2, Cn)
    slots = [1, max(to.append_slot(batch, 1), 0)]
    got, info = tp.pcre_transplant(model, *_args(batch), library=lib, freq=freq, slot=slots)
    assert got.shape == (2, Cn, 2, 1 if regression else 2) and info["slot"].tolist() == slots
    got = got.cpu().reshape(2, Cn * 2, -1)
    assert torch.equal(got, _model_rows(model, batch, lib, freq, slots)), name
    with torch.no_grad():
        assert torch.equal(info["logits"], model(*_args(batch)))
    vs = [(0, 0), (Cn // 2, 1), (Cn - 1, 0)]
    ora = to.oracle_logits(P, batch, lib.feats, _cols(lib), freq, slots, cfg, variants=vs)
    d = (got[:, [c * 2 + q for c, q in vs]] - ora).abs().max().item()
    print(name, "vs oracle %.2e" % d)
    assert d < TOL, (name, d)


def test_same_bits_for_every_max_batch_call_after_call_and_packed_forms(data, small, reference):
    from chromoformer_amd.engine import Slot
    ds, batch, lib = data
    slots, freq, ref, base = reference
    ref = ref.reshape(3, 11, 2, 2)
    kw = dict(library=lib, freq=freq, slot=slots)
    for _ in range(2):
        assert torch.equal(tp.pcre_transplant(small, *_args(batch), **kw)[0].cpu(), ref)
    P = orc.init_params(None, 42, False)
    for cap in (7, 64):
        got, info = tp.pcre_transplant(_model(None, False, P, cap), *_args(batch), **kw)
        assert torch.equal(got.cpu(), ref) and torch.equal(info["logits"].cpu(), base), cap
    packed = small.pack_batch(batch)
    slot = Slot(small, 3).fill(small, batch)
    for p in (packed, slot):
        assert torch.equal(tp.pcre_transplant(small, p, **kw)[0].cpu(), ref)
        assert tp.pcre_transplant(small, p, library=lib, freq=FREQ, slot="append")[1]["slot"].tolist() == [-1, -1, 0]


def test_golden_cases_end_to_end(data):
    ds, batch, lib = data
    z = np.load(os.path.join(GOLDEN, "transplant.npz"))
    at = {False: 0, True: 0}
    models = {r: _model(None, r, orc.init_params(None, 42, r), 4) for r in (False, True)}
    for name, gid, slot, cand, f, regression in choose_cases(ds):
        gene = so.dataset_batch(ds, [gid])
        n_part = len(ds.genes[gid]["pcres"])
        got, info = tp.pcre_transplant(models[regression], *_args(gene), library=tp.library_from_regions(ds, [cand]), freq=f,
                                       slot="append" if slot == n_part else slot)
        gold = torch.from_numpy(z["reg" if regression else "clf"][at[regression]])
        at[regression] += 1
        d = max((info["logits"][0].cpu() - gold[0]).abs().max().item(), (got[0, 0, 0].cpu() - gold[1]).abs().max().item())
        print("%s: vs golden %.2e" % (name, d))
        assert info["slot"].tolist() == [slot] and d < TOL, (name, d)


def test_launch_contract(data):
    ds, batch, lib = data
    P = orc.init_params(None, 42, False)
    B, S, n_reg_head = 3, 8, 2
    for cap in (64, 7):
        model = _model(None, False, P, cap)
        with torch.no_grad():
            model(*_args(batch))
        n_trunk = model.launch_counts()[0] - n_reg_head
        for Cn, Q in ((11, 2), (3, 5)):
            tp.pcre_transplant(model, *_args(batch), library=lib.select(range(Cn)), freq=torch.arange(1.0, Q + 1), slot=[3, 0, 5])
            U = -(-Cn // S)
            want = (n_trunk + 1) + -(-B * U // cap) * (n_trunk + 2) + -(-B * (1 + Cn * Q) // cap) * (1 + n_reg_head)
            assert model.launch_counts()[0] == want, (cap, Cn, Q, model.launch_counts()[0], want)


def test_refusals_by_name_before_anything_is_launched(data):
    ds, batch, lib = data
    L = _lib.lib()
    model = _model(None, False, orc.init_params(None, 42, False), 4)
    bs, keep = model.pack_batch(batch)
    st = torch.cuda.current_stream().cuda_stream
    Cn, Q = 2, 2
    out = torch.full((3, 1 + Cn * Q, 2), float("nan"), device="cuda")
    lf = [lib.feats[b][:Cn].cuda().contiguous() for b in BINS]
    lm = [lib.mask_rows[b][:Cn].cuda().contiguous() for b in BINS]
    fq = torch.ones(3, Cn, Q, device="cuda")
    f0 = model.launch_counts()[0]

    def call(h=model._handle, b=bs, lg=out, no_opts=False, feats=None, masks=None, **kw):
        o = _lib.cf_transplant_opts()
        o.n_cand, o.n_freq, o.slot_all, o.freq = Cn, Q, -1, fq.data_ptr()
        for r in range(3):
            o.lib_feats[r], o.lib_mask[r] = lf[r].data_ptr(), lm[r].data_ptr()
        for r, p in (feats or {}).items():
            o.lib_feats[r] = p
        for r, p in (masks or {}).items():
            o.lib_mask[r] = p
        for k, v in kw.items():
            setattr(o, k, v)
        return L.cf_pcre_transplant(h, C.byref(b) if b is not None else None, None if no_opts else C.byref(o),
                                    lg.data_ptr() if lg is not None else None, st)

    big = _lib.cf_batch.from_buffer_copy(bs)
    big.B = 5
    cases = [(dict(h=None), b"null handle"), (dict(b=None), b"null batch"), (dict(no_opts=True), b"null opts"), (dict(lg=None), b"null logits"),
             (dict(freq=None), b"null freq"), (dict(feats={1: None}), b"lib_feats / lib_mask[1]"), (dict(masks={2: None}), b"lib_feats / lib_mask[2]"),
             (dict(b=big), b"max_batch"), (dict(n_cand=0), b"n_cand"), (dict(n_freq=0), b"n_freq"),
             (dict(n_cand=1 << 20, n_freq=1 << 10), b"do not fit an int"), (dict(slot_all=-2), b"slot_all"), (dict(slot_all=8), b"slot_all")]
    for kw, msg in cases:
        assert call(**kw) != 0, kw
        err = L.cf_last_error()
        assert msg in err and b"cf_pcre_transplant" in err, (kw, err)
    # (a lib_feats / lib_mask index >= n_res cannot be formed: cf_create takes exactly CF_MAX_RES = 3 resolutions)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and model.launch_counts()[0] == f0      # nothing was launched
    # a slot[b] outside [-1, i_max) is device data: read as -1
    wild = torch.tensor([99, -7, 0], dtype=torch.int32, device="cuda")
    used = torch.full((3,), 55, dtype=torch.int32, device="cuda")
    assert call(slot=wild.data_ptr(), slot_out=used.data_ptr()) == 0, L.cf_last_error()
    torch.cuda.synchronize()
    assert used.tolist() == [-1, -1, 0] and torch.equal(out[:2], out[:2, :1].expand(2, 1 + Cn * Q, 2)) and not bool(torch.isnan(out).any())
    out.fill_(float("nan"))
    for bad, msg in (("prepend", "append"), (8, "outside"), ([0, 1], "one per gene")):      # (raised by the function before it calls the library)
        with pytest.raises(ValueError, match=msg):
            tp.pcre_transplant(model, (bs, keep), library=lib, slot=bad)
    with pytest.raises(ValueError, match="candidates"):
        tp.pcre_transplant(model, (bs, keep), library=lib, freq=torch.ones(3, 2))
    # armed riders (a training step in flight): refused; the handle is not used again
    assert L.cf_rider_arm(model._handle, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, 0, 8) == 0, L.cf_last_error()
    assert call() != 0 and b"riders" in L.cf_last_error() and b"cf_pcre_transplant" in L.cf_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    del keep


def test_no_side_effects_on_training_and_a_stale_backward_is_refused():
    from chromoformer_amd.engine import Trainer
    batches = [orc.synthetic_batch(8, seed=41 + i, regime="realistic") for i in range(3)]
    P = orc.init_params(None, 42, False)
    lib = tp.library_from_batch(batches[2], [(g, 0) for g in range(8)] + [(0, 1)])

    def run(interpose):
        model = _model(None, False, P, 8)
        tr = Trainer(model, lr=1e-3)
        slots = [tr.stage(b) for b in batches[:2]]
        tr.step(slots[0])
        torch.cuda.synchronize()
        snap = [t.clone() for t in (model._flat, model._gflat, model._mflat, model._vflat)]
        if interpose:
            tp.pcre_transplant(model, *_args(batches[2]), library=lib, freq=[1.0, 2.0], slot=2)
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
        lg, _ = tp.pcre_transplant(model, *_args(batches[1]), library=lib, freq=1.0)
        assert not lg.requires_grad
        with pytest.raises(RuntimeError, match="pcre_transplant"):
            out[:, 1].sum().backward()
        model(*_args(b))[:, 1].sum().backward()      # a fresh forward trains as before
    # the C ABI itself refuses a backward without a new saving forward
    bs, keep = model.pack_batch(b)
    st = torch.cuda.current_stream().cuda_stream
    lgt = torch.empty(8, 2, device="cuda")
    _lib.check(_lib.lib().cf_forward(model._handle, C.byref(bs), lgt.data_ptr(), 1, st), "cf_forward")
    tp.pcre_transplant(model, (bs, keep), library=lib, freq=1.0)
    dl = torch.zeros(8, 2, device="cuda")
    assert _lib.lib().cf_backward_from(model._handle, C.byref(bs), dl.data_ptr(), st) != 0
    assert b"must follow cf_forward" in _lib.lib().cf_last_error()


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
    ds = ChromoformerDataset(meta, npy, table.gene_id.tolist())
    regions = [tuple(ds.genes[ds.target_genes[3]]["pcres"][0]) + ("hijacked",), tuple(ds.genes[ds.target_genes[0]]["pcres"][0]),
               tuple(ds.genes[ds.target_genes[7]]["pcres"][2])]
    bed = str(tmp_path / "cand.bed")
    with open(bed, "w") as fh:
        fh.write("# candidates\n" + "".join("\t".join(str(x) for x in r) + "\n" for r in regions))
    out = str(tmp_path / "t.npz")
    assert predict.main(["-m", meta, "-d", npy, "-w", ck, "-o", str(tmp_path / "p.csv"), "--transplant-bed", bed, "--transplant-out", out,
                         "--transplant-freq", "1,4"]) == 0
    z = np.load(out)
    assert sorted(z.files) == ["candidates", "freqs", "gene_ids", "placed", "prediction", "slot", "transplant"]
    assert list(z["gene_ids"]) == table.gene_id.tolist() and z["freqs"].tolist() == [1.0, 4.0]
    assert z["candidates"].tolist() == ["hijacked", "%s:%d-%d" % regions[1], "%s:%d-%d" % regions[2]]
    assert z["transplant"].shape == (20, 3, 2) and z["transplant"].dtype == np.float32 and np.isfinite(z["transplant"]).all()
    n_part = [len(ds.genes[g]["pcres"]) for g in ds.target_genes]
    assert z["slot"].tolist() == [n if n < 8 else -1 for n in n_part] and z["placed"].tolist() == [n < 8 for n in n_part]
    assert np.array_equal(pd.read_csv(str(tmp_path / "p.csv"))["prediction"].to_numpy().astype(np.float32), z["prediction"])
    model = ChromoformerClassifier(seed=123, max_batch=32).cuda(0)
    model.load_state_dict(P)
    batch = torch.utils.data.default_collate([ds[i] for i in range(len(ds))])
    lib = tp.library_from_regions(ds, regions)
    direct, info = tp.pcre_transplant(model, *_args(batch), library=lib, freq=[1.0, 4.0], slot="append")
    ref = torch.sigmoid(direct.cpu())[..., 1].numpy()
    assert np.abs(z["transplant"] - ref).max() <= 1e-6 and np.abs(z["prediction"] - torch.sigmoid(info["logits"].cpu())[:, 1].numpy()).max() <= 1e-6
    full = [i for i, n in enumerate(n_part) if n == 8]
    assert full and np.array_equal(z["transplant"][full], np.broadcast_to(z["prediction"][full, None, None], (len(full), 3, 2)))
    # the generator: keys, shapes, the same numbers; an explicit slot replaces
    genes = ds.target_genes[:5]
    res = list(tp.pcre_transplant_dataset(model, ds, regions, [1.0, 4.0], genes=genes, bsz=3))
    assert [d["gene_id"] for d in res] == genes
    for i, d in enumerate(res):
        assert sorted(d) == ["candidates", "gene_id", "logits", "placed", "slot", "transplant"]
        assert d["transplant"].shape == (3, 2, 2) and d["transplant"].dtype == np.float32 and d["logits"].shape == (2,)
        assert d["slot"] == int(z["slot"][i]) and d["placed"] == bool(z["placed"][i]) and d["candidates"] == lib.names
        sig = 1 / (1 + np.exp(-d["transplant"][..., 1].astype(np.float64)))      # (the store is binned on the device: compared as the CLI's output is)
        assert np.abs(sig - z["transplant"][i]).max() <= 1e-6
    res = list(tp.pcre_transplant_dataset(model, ds, lib, 2.0, slot=0, genes=genes[:2], bsz=2))
    want, _ = tp.pcre_transplant(model, *_args(torch.utils.data.default_collate([ds[0], ds[1]])), library=lib, freq=2.0, slot=0)
    sig = torch.sigmoid(torch.from_numpy(np.stack([d["transplant"] for d in res])))[..., 1]
    assert all(d["slot"] == 0 and d["placed"] for d in res) and (sig - torch.sigmoid(want.cpu())[..., 1]).abs().max().item() <= 1e-6
