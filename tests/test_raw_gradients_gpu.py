"""Raw-signal saliency on the GPU: cf_bin_regions_multi_backward (backward of the one-launch binning) and raw_signal_gradients.

  * the kernel against the definition (tests/raw_grad_oracle.py: closed form in fp64, fp32 autograd through bin_log1p / centred as the
    yardstick of what fp32 can give) on the regions of test_one_pass_kernel_equals_the_per_resolution_kernel: every alignment class,
    windows inside the file, partial last bins, mirrored regions, nested and non-nested bin sizes, dfeat with non-zero pad rows,
    NaN-prefilled output with two row pitches; run to run bit-identical; gradient x input;
  * the one-pass path and the per-region walk agree (same regions, output moved by one float);
  * end to end: raw_signal_gradients against the model's own x.grad pushed through the closed form, and against the oracle's
    autograd from the raw signal to the logit; genomic orientation of a '-' strand promoter; no side effects; the CLI.

Referee rule (tests/test_input_grads_gpu.py): per region |hip - ref64| <= max(2 |host32 - ref64|, 2e-5 |ref64|) in the 2-norm."""
import ctypes as C
import os

import numpy as np
import pandas as pd
import pytest
import torch

from oracle import chromoformer_oracle as orc
from tests.raw_grad_oracle import autograd_form, closed_form, make_small_dataset

pytestmark = pytest.mark.gpu
F, W = 7, 40000


def _referee(hip, host32, ref64, what):
    n = float(np.linalg.norm(ref64))
    err_h = float(np.linalg.norm(hip.astype(np.float64) - ref64))
    err_32 = float(np.linalg.norm(np.asarray(host32, dtype=np.float64) - ref64))
    print("%s: |hip - ref64| / |ref64| = %.3e, |host32 - ref64| / |ref64| = %.3e" % (what, err_h / max(n, 1e-30), err_32 / max(n, 1e-30)))
    assert err_h <= max(2 * err_32, 2e-5 * n) + 1e-12, (what, err_h / max(n, 1e-30), err_32 / max(n, 1e-30))


def _regions(lens, rng):
    """(raw fp16 [F, len], col0, ncols, flip) per region, drawn as the forward's test draws them."""
    out = []
    for k, (ln, col0, ncols) in enumerate(lens):
        a = (rng.random((F, ln)) * rng.choice([0.5, 4.0, 60.0])).astype(np.float16)
        a[:, rng.random(ln) < 0.3] = 0
        out.append((a, col0, ncols, k % 2))
    return out


def _run_backward(regs, binsizes, Ls, dfeat, pitch, times_input, shift=0):
    """One cf_bin_regions_multi_backward launch -> (draw buffers [F, ld_out] per region as numpy, NaN-prefilled).  shift: floats by which
    every draw is moved off its 16-byte alignment."""
    from chromoformer_amd import _lib
    from chromoformer_amd.data import BIN_GRAD_JOB
    dev = torch.device("cuda", 0)
    nres = len(binsizes)
    offs, n = [], 0
    for a, _, _, _ in regs:
        offs.append(n)
        n += -(-a.size // 4) * 4
    flat = np.zeros(n, dtype=np.float16)
    for (a, _, _, _), o in zip(regs, offs):
        flat[o:o + a.size] = a.reshape(-1)
    raw = torch.from_numpy(flat).to(dev)
    d_dev = [[torch.from_numpy(d.astype(np.float32)).to(dev) for d in per] for per in dfeat]
    ooffs, n = [], 0
    for ld_out in pitch:
        ooffs.append(n)
        n += -(-F * ld_out // 4) * 4
    draw = torch.full((n + 4,), float("nan"), device=dev)
    jobs = np.zeros(len(regs), dtype=BIN_GRAD_JOB)
    for k, (a, col0, ncols, flip) in enumerate(regs):
        jobs[k]["raw"], jobs[k]["ld"], jobs[k]["col0"], jobs[k]["ncols"], jobs[k]["flip"] = raw.data_ptr() + 2 * offs[k], a.shape[1], col0, ncols, flip
        for r in range(nres):
            jobs[k]["dfeat"][r] = d_dev[k][r].data_ptr()
        jobs[k]["draw"], jobs[k]["ld_out"] = draw.data_ptr() + 4 * (ooffs[k] + shift), pitch[k]
    tab = torch.from_numpy(jobs.view(np.uint8)).to(dev)
    bs, nb = (C.c_int * nres)(*binsizes), (C.c_int * nres)(*Ls)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.lib().cf_bin_regions_multi_backward(C.c_void_p(tab.data_ptr()), len(regs), F, nres, bs, nb, max(r[2] for r in regs),
                                                        int(times_input), st), "cf_bin_regions_multi_backward")
    torch.cuda.synchronize()
    host = draw.cpu().numpy()
    return [host[o + shift:o + shift + F * ld].reshape(F, ld) for o, ld in zip(ooffs, pitch)]


@pytest.mark.parametrize("binsizes", [(2000, 500, 100), (500, 100), (2000, 300, 100), (1000, 200, 40)])
def test_kernel_against_the_definition(binsizes):
    rng = np.random.default_rng(3)
    lens = [(40000, 0, 40000), (40000, 4, 39996), (40000, 15000, 10000)]
    lens += [(n, 0, n) for n in (4, 7, 36, 96, 100, 104, 500, 1833, 1996, 2000, 2001, 2004, 3999, 8000, 12344, 12345, 39996)]
    regs = _regions(lens, rng)
    Ls = [W // b for b in binsizes]
    dfeat = [[rng.standard_normal((L, F)) for L in Ls] for _ in regs]                      # pad rows included
    pitch = [nc if (k // 2) % 2 == 0 else -(-nc // 4) * 4 + 4 for k, (_, _, nc, _) in enumerate(regs)]
    got = _run_backward(regs, binsizes, Ls, dfeat, pitch, 0)
    again = _run_backward(regs, binsizes, Ls, dfeat, pitch, 0)
    timed = _run_backward(regs, binsizes, Ls, dfeat, pitch, 1)
    for k, (a, col0, ncols, flip) in enumerate(regs):
        d32 = [d.astype(np.float32) for d in dfeat[k]]
        ref64 = closed_form(a, col0, ncols, flip, binsizes, Ls, d32)
        host32 = autograd_form(a, col0, ncols, flip, binsizes, Ls, d32, torch.float32).numpy()
        win, rest = got[k][:, :ncols], got[k][:, ncols:]
        what = "%s len %d col0 %d ncols %d flip %d pitch %d" % (binsizes, a.shape[1], col0, ncols, flip, pitch[k])
        assert np.isfinite(win).all(), what
        assert np.isnan(rest).all(), (what, "written past the window")
        _referee(win, host32, ref64, what)
        assert np.array_equal(got[k].view(np.int32), again[k].view(np.int32)), (what, "not run-to-run identical")
        x = a[:, col0:col0 + ncols].astype(np.float32)
        assert np.isnan(timed[k][:, ncols:]).all(), what
        assert np.allclose(timed[k][:, :ncols], win * x, rtol=1e-6, atol=1e-30), (what, "gradient x input")


def test_one_pass_path_and_per_region_walk_agree():
    """The same 4-aligned regions once with a 16-byte aligned output (one-pass path) and once with the output moved by one float (the
    per-region walk): another order of the additions inside a bin, 1e-6 relative as the forward's test allows."""
    rng = np.random.default_rng(9)
    binsizes = (2000, 500, 100)
    lens = [(40000, 0, 40000), (40000, 4, 39996), (40000, 15000, 10000)] + [(n, 0, n) for n in (4, 36, 100, 1996, 2004, 8000, 12344)]
    regs = _regions(lens, rng)
    Ls = [W // b for b in binsizes]
    dfeat = [[rng.standard_normal((L, F)) for L in Ls] for _ in regs]
    pitch = [nc + 4 for _, _, nc, _ in regs]
    fast = _run_backward(regs, binsizes, Ls, dfeat, pitch, 0)
    walk = _run_backward(regs, binsizes, Ls, dfeat, pitch, 0, shift=1)
    for k, (a, col0, ncols, flip) in enumerate(regs):
        x, y = fast[k][:, :ncols].astype(np.float64), walk[k][:, :ncols].astype(np.float64)
        assert np.isnan(fast[k][:, ncols:]).all() and np.isnan(walk[k][:, ncols:]).all()
        assert np.linalg.norm(x - y) <= 1e-6 * np.linalg.norm(x), (k, np.linalg.norm(x - y) / np.linalg.norm(x))


# ----------------------------------------------------------------------------------------------------------------- end to end
def _setup(tmp_path, regression=False, w_prom=40000, genes=None):
    from chromoformer_amd.data import ChromoformerDataset
    from tests.test_input_grads_gpu import _model, _params
    meta, orphan = make_small_dataset(str(tmp_path / "npy"))
    table = pd.read_csv(meta)
    ids = table.gene_id.tolist() if genes is None else [table.gene_id[i] for i in genes]
    ds = ChromoformerDataset(meta, str(tmp_path / "npy"), ids, w_prom=w_prom, regression=regression)
    P = _params(None, regression)
    return ds, table, orphan, P, _model(None, regression, P, 8)


def test_end_to_end_is_the_models_input_gradient_pushed_through_the_binning(tmp_path):
    from chromoformer_amd.data import GeneStore, load_raw_regions, raw_window
    ds, table, orphan, P, model = _setup(tmp_path, w_prom=10000)
    out = list(model.raw_signal_gradients(ds, bsz=4))                                       # two chunks
    assert [d["gene_id"] for d in out] == ds.target_genes
    store = GeneStore(ds, device="cuda:0", resident=True)
    b = store.batch(list(range(len(ds))))
    pf = {k: v.clone().requires_grad_(True) for k, v in b["promoter_feats"].items()}
    cf = {k: v.clone().requires_grad_(True) for k, v in b["pcre_feats"].items()}
    logits = model(pf, b["promoter_pad_masks"], cf, b["pcre_pad_masks"], b["interaction_masks"], b["interaction_freq"])
    logits[:, 1].sum().backward()
    n_bins = [ds.w_max // bs for bs in ds.binsizes]
    minus = 0
    for i, d in enumerate(out):
        g = ds.genes[d["gene_id"]]
        assert np.abs(d["logits"] - logits[i].detach().cpu().numpy()).max() < 1e-5
        assert len(d["pcres"]) == len(g["pcres"]) and len(d["regions"]) == 1 + len(g["pcres"])
        for s, flip, a in load_raw_regions(ds, d["gene_id"]):
            c0, nc = raw_window(ds, s, a.shape[1])
            dfeat = [(pf[bs].grad[i, 0] if s < 0 else cf[bs].grad[i, s]).cpu().numpy() for bs in ds.binsizes]
            ref64 = closed_form(a, c0, nc, flip, ds.binsizes, n_bins, dfeat)
            host32 = autograd_form(a, c0, nc, flip, ds.binsizes, n_bins, dfeat, torch.float32).numpy()
            hip = d["promoter"] if s < 0 else d["pcres"][s]
            assert hip.shape == (F, nc) and hip.dtype == np.float32
            _referee(hip, host32, ref64, "%s slot %d" % (d["gene_id"], s))
            if s < 0:
                chrom, tss, strand = g["tss"]
                assert d["regions"][0] == (chrom, tss - 20000 + c0, tss - 20000 + c0 + nc)
                if strand == "-":                                                          # genomic orientation: the mirror is undone
                    minus += 1
                    err = np.linalg.norm(hip - ref64)
                    assert np.linalg.norm(hip[:, ::-1] - ref64) >= 10 * err
            else:
                assert d["regions"][1 + s] == tuple(g["pcres"][s])
    assert minus >= 1


def _oracle_raw_grads(ds, P, gene_ids, col, dtype, regression):
    """Autograd from the raw signals to logits[:, col] through bin_log1p + centred and the oracle's forward -> {(gene, slot): grad}."""
    leaves = {}

    def load(chrom, start, end):
        key = (chrom, start, end)
        if key not in leaves:
            a = np.load("%s/%s:%d-%d.npy" % (ds.npy_dir, chrom, start, end))
            leaves[key] = torch.from_numpy(a.astype(np.float64)).to(dtype).requires_grad_(True)
        return leaves[key]

    S = ds.i_max
    items = [ds[ds.target_genes.index(g)] for g in gene_ids]                               # masks, frequencies (fp32 loader)
    keep, ds._load = ds._load, load
    try:
        batch = {k: {} for k in ("promoter_feats", "promoter_pad_masks", "pcre_feats", "pcre_pad_masks", "interaction_masks")}
        regs = [ds.regions(g, dtype=dtype) for g in gene_ids]
    finally:
        ds._load = keep
    for b in ds.binsizes:
        L = ds.w_max // b
        pfs, cfs = [], []
        for reg in regs:
            p, _, _, pcs = reg[b]
            pfs.append(p.t().unsqueeze(0))
            rows = [x.t() for x, _, _ in pcs] + [torch.zeros(L, F, dtype=dtype)] * (S - len(pcs))
            cfs.append(torch.stack(rows))
        batch["promoter_feats"][b], batch["pcre_feats"][b] = torch.stack(pfs), torch.stack(cfs)
        for k in ("promoter_pad_masks", "pcre_pad_masks", "interaction_masks"):
            batch[k][b] = torch.stack([it[k][b] for it in items])
    batch["interaction_freq"] = torch.stack([it["interaction_freq"] for it in items]).to(dtype)
    Pd = {k: v.detach().to(dtype) for k, v in P.items()}
    orc.forward(Pd, batch, None)[:, col].sum().backward()
    out = {}
    for g in gene_ids:
        chrom, tss, _ = ds.genes[g]["tss"]
        out[g, -1] = leaves[chrom, tss - 20000, tss + 20000].grad
        for s, p in enumerate(ds.genes[g]["pcres"]):
            out[g, s] = leaves[tuple(p)].grad
    return out


@pytest.mark.parametrize("regression", [False, True], ids=["classifier", "regressor"])
def test_end_to_end_against_the_oracle_from_the_raw_signal(tmp_path, regression):
    from chromoformer_amd.data import raw_window
    ds, table, orphan, P, model = _setup(tmp_path, regression=regression)
    minus = [g for g in ds.target_genes if ds.genes[g]["tss"][2] == "-" and ds.genes[g]["pcres"]][0]
    assert not ds.genes[orphan]["pcres"]
    ids = [minus, orphan]
    col = 0 if regression else 1
    out = list(model.raw_signal_gradients(ds, genes=ids))                                   # default target
    g32 = _oracle_raw_grads(ds, P, ids, col, torch.float32, regression)
    g64 = _oracle_raw_grads(ds, P, ids, col, torch.float64, regression)
    assert [d["gene_id"] for d in out] == ids and out[1]["pcres"] == []
    for d in out:
        tracks = [(-1, d["promoter"])] + list(enumerate(d["pcres"]))
        for s, hip in tracks:
            key = (d["gene_id"], s)
            c0, nc = raw_window(ds, s, g64[key].shape[1])
            _referee(hip, g32[key][:, c0:c0 + nc].numpy(), g64[key][:, c0:c0 + nc].numpy(), "%s slot %d" % key)


def test_no_side_effects(tmp_path):
    ds, table, orphan, P, model = _setup(tmp_path, genes=[1, 2])
    batch = orc.synthetic_batch(4, seed=3, regime="realistic")
    args = [batch[k] for k in ("promoter_feats", "promoter_pad_masks", "pcre_feats", "pcre_pad_masks", "interaction_masks", "interaction_freq")]
    logits = model(*args)
    logits[:, 1].sum().backward()
    torch.cuda.synchronize()
    l0 = logits.detach().clone()
    p0 = {k: p.detach().clone() for k, p in model.named_parameters()}
    g0 = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    assert g0
    a = list(model.raw_signal_gradients(ds))
    b = list(model.raw_signal_gradients(ds, times_input=True))
    torch.cuda.synchronize()
    assert all(torch.equal(p0[k], p.detach()) for k, p in model.named_parameters()), "parameters changed"
    assert {k for k, p in model.named_parameters() if p.grad is not None} == set(g0)
    assert all(torch.equal(g0[k], p.grad) for k, p in model.named_parameters() if p.grad is not None), "parameter gradients changed"
    with torch.no_grad():
        assert torch.equal(model(*args), l0)
    c = list(model.raw_signal_gradients(ds))
    assert all(np.array_equal(x["promoter"], y["promoter"]) for x, y in zip(a, c))
    x = np.load("%s/%s:%d-%d.npy" % ((ds.npy_dir,) + a[0]["regions"][0])).astype(np.float32)
    assert np.allclose(b[0]["promoter"], a[0]["promoter"] * x, rtol=1e-6, atol=1e-30)


def test_refusals_by_name(tmp_path):
    from chromoformer_amd.data import ChromoformerDataset
    from tests.test_input_grads_gpu import _model
    ds, table, orphan, P, model = _setup(tmp_path, genes=[2])
    with pytest.raises(ValueError, match="target = 5"):
        next(model.raw_signal_gradients(ds, target=5))
    ds4 = ChromoformerDataset(ds.meta, ds.npy_dir, ds.target_genes, binsizes=[2000, 500, 500])
    with pytest.raises(ValueError, match="repeated bin sizes"):
        next(model.raw_signal_gradients(ds4))
    cfg = orc._cfg(dict(embed=dict(n_layers=2, n_heads=2, d_model=128, d_ff=128)))
    deep = _model(cfg, False, orc.init_params(cfg, 42, False), 2)
    with pytest.raises(RuntimeError, match="promoter_feats.*embed.n_layers"):
        next(deep.raw_signal_gradients(ds))
    # the C ABI refuses a row pitch shorter than the window, by name
    from chromoformer_amd import _lib
    rng = np.random.default_rng(1)
    regs = _regions([(100, 0, 100)], rng)
    with pytest.raises(RuntimeError, match="ld_out = 96 < ncols = 100"):
        _run_backward(regs, (2000, 500, 100), [20, 80, 400], [[rng.standard_normal((L, F)) for L in (20, 80, 400)]], [96], 0)


def test_cli_writes_one_npz_per_gene(tmp_path):
    from chromoformer_amd import predict
    meta, orphan = make_small_dataset(str(tmp_path / "npy"))
    table = pd.read_csv(meta)
    ck = str(tmp_path / "w.pt")
    torch.save({"net": orc.init_params(seed=7)}, ck)
    d = str(tmp_path / "sal")
    assert predict.main(["-m", meta, "-d", str(tmp_path / "npy"), "-w", ck, "-o", str(tmp_path / "p.csv"), "--raw-saliency-dir", d]) == 0
    assert sorted(os.listdir(d)) == sorted("%s.npz" % g for g in table.gene_id)
    for r in table.to_dict("records"):
        z = np.load(os.path.join(d, "%s.npz" % r["gene_id"]))
        names = r["neighbors"].split(";") if isinstance(r["neighbors"], str) else []
        assert list(z["regions"]) == ["%s:%d-%d" % (r["chrom"], r["start"] - 20000, r["start"] + 20000)] + names
        assert z["promoter"].shape == (7, 40000) and z["promoter"].dtype == np.float32 and z["logits"].shape == (2,)
        assert np.isfinite(z["promoter"]).all() and np.abs(z["promoter"]).max() > 0
        for s, nm in enumerate(names):
            a, e = nm.split(":")[1].split("-")
            assert z["pcre_%d" % s].shape == (7, int(e) - int(a))
        assert "pcre_%d" % len(names) not in z.files
