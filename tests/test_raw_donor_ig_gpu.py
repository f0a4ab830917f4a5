"""Integrated gradients in raw-signal space against a donor cell type on the GPU (cf_integrated_gradients_raw_donor,
cf_bin_spread_difference, integrated_gradients(path="signal", donor=...), raw_integrated_gradients(donor_dataset=...)):

  * tensor level at bsz 3 against the fp32 and fp64 oracles of tests/raw_donor_ig_oracle.py by the referee rule of
    tests/test_raw_ig_gpu.py, classifier and regressor; exact zeros where the oracle has exact zeros; delta by its 1e-5 gap + 1e-6 rule;
  * bit identities: a donor of zeros is cf_integrated_gradients_raw; the batch as its own donor gives zeros; the two logits outputs
    are model(...) on the two batches; an unchanged mark and dummy slots get exactly 0;
  * the same bits whatever max_batch is, call after call, one gene alone, one node; the scalar branch; i_max = 16;
  * cf_bin_spread_difference alone against the numpy reference, both paths, guard values intact;
  * end to end on the 20-gene dataset and a donor dataset, generator and CLI; refusals by name with nothing launched; a pending
    backward is refused afterwards; no side effects on training."""
import ctypes as C
import os

import numpy as np
import pandas as pd
import pytest
import torch

from chromoformer_amd import _lib
from chromoformer_amd.attribution import ig_quadrature
from oracle import chromoformer_oracle as orc
from tests import donor_oracle as do
from tests import scan_oracle as so
from tests.raw_donor_ig_oracle import oracle_ig_signal_donor, spread_reference
from tests.raw_ig_oracle import FEATS
from tests.test_input_grads_gpu import _batch, _model, _params
from tests.test_raw_ig_gpu import _args, _flat, _referee, _same, _slice

pytestmark = pytest.mark.gpu
BINS = (2000, 500, 100)
ALL = FEATS + ("interaction_freq",)
SAME_MARK = 2


def _donor(batch, seed, same_mark=SAME_MARK):
    """A second cell type for a synthetic batch: every feature scaled by a factor in [0.3, 1.7] drawn per element (zeros -- padded
    rows, dummy slots -- stay zeros), mark `same_mark` left as it is, bit for bit -> {"promoter_feats": ..., "pcre_feats": ...}."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k in FEATS:
        out[k] = {}
        for b, t in batch[k].items():
            d = t * (0.3 + 1.4 * torch.rand(t.shape, generator=g))
            if same_mark is not None:
                d[..., same_mark] = t[..., same_mark]
            out[k][b] = d.contiguous()
    return out


def _dev(donor):
    return tuple({b: t.cuda().contiguous() for b, t in donor[k].items()} for k in FEATS)


def _run(model, batch, donor, **kw):
    """-> (attr and cmean flattened into one dict, info on the CPU without cmean)."""
    attr, info = model.integrated_gradients(*_args(batch), path="signal", donor=_dev(donor), **kw)
    assert "coeff" not in info
    out = _flat(attr)
    out.update({"cmean." + k: v for k, v in _flat(info["cmean"]).items()})
    return out, {k: v.cpu() for k, v in info.items() if k != "cmean"}


def _oracles(P, batch, donor, a, w, t, **kw):
    res = []
    for dt in (torch.float32, torch.float64):
        at, cm, lx, lb, d = oracle_ig_signal_donor(P, batch, donor, a, w, t, inputs=ALL, dtype=dt, **kw)
        r = _flat(at)
        r.update({"cmean." + k: v for k, v in _flat(cm).items()})
        res.append((r, lx, lb, d))
    return res


def _check(got, info, o32, o64, t, what=""):
    (r32, _, _, _), (r64, lx64, lb64, d64) = o32, o64
    assert sorted(got) == sorted(r64)
    for k in r64:
        _referee(got[k], r32[k], r64[k], what + k)
        zero = r32[k] == 0
        assert bool((got[k][zero] == 0).all()), (k, "non-zero where the oracle has exact zeros")
    assert (info["logits"].double() - lx64).abs().max().item() < 1e-4
    assert (info["baseline_logits"].double() - lb64).abs().max().item() < 1e-4
    gap = (lx64[:, t] - lb64[:, t]).abs()
    err = (info["delta"].double() - d64).abs()
    print(what, "delta", info["delta"], d64, err, 1e-5 * gap + 1e-6)
    assert bool((err <= 1e-5 * gap + 1e-6).all()), (err, gap)


@pytest.mark.parametrize("regression", [False, True], ids=["classifier", "regressor"])
def test_matches_the_oracles_default_config(regression):
    # (seed 77 and 20 Gauss-Legendre nodes, as tests/test_raw_ig_gpu.py::test_matches_the_oracle_default_config, whose comment records
    # the open point of cf_backward_from_inputs; here B = 3, a batch of its own.  On the CPU the fp32 oracle passes every
    # bound below against the fp64 one for this seed and node count: logits 2.2e-7 / 3.2e-7 off (classifier / regressor),
    # |delta32 - delta64| at most 0.16 / 0.08 of its bound, attr and cmean 0.7e-7 .. 3.3e-7 relative, interaction_freq 4.6e-7 / 7.5e-7.)
    B, t, n = 3, 0 if regression else 1, 20
    batch = _batch(B, 77)
    donor = _donor(batch, 78)
    P = _params(None, regression)
    model = _model(None, regression, P, B)
    a, w = ig_quadrature("gausslegendre", n)
    got, info = _run(model, batch, donor, n_steps=n)
    o32, o64 = _oracles(P, batch, donor, a, w, t)
    _check(got, info, o32, o64, t)
    # padded promoter bins, dummy pCRE slots and the unchanged mark: exact zeros in attr
    dummy = batch["pcre_pad_masks"][100][:, :, 0, 200].all(-1)
    assert bool(dummy.any())
    for b in BINS:
        assert bool((got["pcre_feats.%d" % b][dummy] == 0).all()), b
        for k in FEATS:
            assert bool((got["%s.%d" % (k, b)][..., SAME_MARK] == 0).all()), (k, b)
            assert bool((got["%s.%d" % (k, b)][..., 0] != 0).any()), (k, b)


def test_bit_identities():
    B, n = 3, 5
    batch = _batch(B, 31)
    donor = _donor(batch, 32)
    P = _params(None, False)
    model = _model(None, False, P, 8)
    # a donor of zeros: the zero-signal path, bit for bit (cmean is C, coeff is (1 + m) C: not compared)
    zeros = {k: {b: torch.zeros_like(t) for b, t in batch[k].items()} for k in FEATS}
    got, info = _run(model, batch, zeros, n_steps=n)
    attr, ref_info = model.integrated_gradients(*_args(batch), path="signal", n_steps=n)
    ref = _flat(attr)
    for k, v in ref.items():
        assert torch.equal(got[k], v), k
    for k in ("logits", "baseline_logits", "delta"):
        assert torch.equal(info[k], ref_info[k].cpu()), k
    # the batch as its own donor: attr and delta exactly 0
    own = {k: batch[k] for k in FEATS}
    got, info = _run(model, batch, own, n_steps=n, inputs=FEATS)
    for k, v in got.items():
        if not k.startswith("cmean."):
            assert bool((v == 0).all()), k
    assert bool((info["delta"] == 0).all()) and torch.equal(info["logits"], info["baseline_logits"])
    # logits / baseline_logits: model(...) on the gene's batch and on the donor's features under the gene's masks and frequencies
    # (features only: an interpolated interaction_freq would put its own baseline into the baseline row)
    got, info = _run(model, batch, donor, n_steps=n, inputs=FEATS)
    with torch.no_grad():
        lx = model(*_args(batch)).cpu()
        lb = model(*_args(dict(batch, **donor))).cpu()
    assert torch.equal(info["logits"], lx) and torch.equal(info["baseline_logits"], lb) and not torch.equal(lx, lb)
    dummy = batch["pcre_pad_masks"][100][:, :, 0, 200].all(-1)
    assert bool(dummy.any())
    for b in BINS:
        assert bool((got["pcre_feats.%d" % b][dummy] == 0).all())
        for k in FEATS:
            assert bool((got["%s.%d" % (k, b)][..., SAME_MARK] == 0).all()) and bool((got["%s.%d" % (k, b)] != 0).any())


def test_chunking_determinism_single_gene_and_one_node():
    B, n = 3, 4
    batch = _batch(B, 31)
    donor = _donor(batch, 32)
    P = _params(None, False)
    small = _model(None, False, P, 3)      # chunks of 3 rows, V = 6 rows per gene: the interior rows of every gene straddle two chunks
    big = _model(None, False, P, 64)
    ref, ref_info = _run(big, batch, donor, n_steps=n)
    again, again_info = _run(big, batch, donor, n_steps=n)
    _same(ref, again, "twice in a row")
    _same(ref_info, again_info)
    part, info = _run(small, batch, donor, n_steps=n)
    more, more_info = _run(small, batch, donor, n_steps=n)
    _same(part, more, "twice in a row, max_batch 3")
    _same(part, ref, "max_batch 3 against 64")
    _same(info, ref_info)
    _same(more_info, ref_info)
    one, info = _run(big, _slice(batch, 1, 2), _slice(donor, 1, 2), n_steps=n)
    for k, v in one.items():
        assert torch.equal(v[0], ref[k][1]), k
    assert torch.equal(info["delta"][0], ref_info["delta"][1])
    # one node (riemann_middle: a = 0.5, w = 1)
    got, info = _run(big, batch, donor, n_steps=1, method="riemann_middle")
    o32, o64 = _oracles(P, batch, donor, [0.5], [1.0], 1)
    _check(got, info, o32, o64, 1, "one node ")
    tiny, tiny_info = _run(small, batch, donor, n_steps=1, method="riemann_middle")
    _same(tiny, got, "one node, max_batch 3")
    _same(tiny_info, info)


def test_scalar_branch_odd_row_length():
    """The odd_lengths shape of test_config_variants_gpu.py, L = 10 / 50 / 250 bins: the promoter rows have 70 / 350 / 1750 floats, no
    multiple of 4 (the pCRE rows, 8 slots each, are: both branches run)."""
    cfg = orc._cfg(dict(binsizes=[4000, 800, 160], w_max=40000))
    B, n = 3, 4
    batch = orc.synthetic_batch(B, cfg=cfg, seed=13, regime="realistic")
    donor = _donor(batch, 14)
    assert all(batch["promoter_feats"][b][0].numel() % 4 != 0 for b in cfg["binsizes"])
    P = orc.init_params(cfg, 3, False)
    model = _model(cfg, False, P, 8)
    a, w = ig_quadrature("gausslegendre", n)
    got, info = _run(model, batch, donor, n_steps=n)
    o32, o64 = _oracles(P, batch, donor, a, w, 1, cfg=cfg)
    _check(got, info, o32, o64, 1)


def test_i_max16():
    cfg = orc._cfg(dict(i_max=16))
    B, n = 3, 4
    batch = orc.synthetic_batch(B, cfg=cfg, seed=13, regime="realistic")
    donor = _donor(batch, 14)
    P = orc.init_params(cfg, 3, False)
    model = _model(cfg, False, P, 8)
    a, w = ig_quadrature("gausslegendre", n)
    got, info = _run(model, batch, donor, n_steps=n)
    o32, o64 = _oracles(P, batch, donor, a, w, 1, cfg=cfg)
    _check(got, info, o32, o64, 1)


# ------------------------------------------------------------------------------------------------- cf_bin_spread_difference alone
GUARD = 777.0
U = 2.0 ** -24


def _spread_case(binsizes, n_bins, specs, F=7, seed=3):
    """specs: dicts (ncols, flip, col0, odd_ld, draw_shift, no_donor, no_cmean) -> one launch, every job checked against the numpy
    reference: |device - exact| <= gamma_7 |x - xd| sum_r |C_r| / cnt_r, and no element outside draw[f, :ncols] written."""
    from chromoformer_amd.data import BIN_SPREAD_JOB
    rng = np.random.default_rng(seed)
    nres = len(binsizes)
    jobs = np.zeros(len(specs), dtype=BIN_SPREAD_JOB)
    keep, host = [], []
    for k, sp in enumerate(specs):
        nc, col0 = sp["ncols"], sp.get("col0", 8)
        ld = -(-(col0 + nc) // 4) * 4 + (1 if sp.get("odd_ld") else 0)
        x = rng.poisson(3.0, size=(F, ld)).astype(np.float16)
        xd = rng.poisson(2.0, size=(F, ld)).astype(np.float16)
        xd[:, ::5] = x[:, ::5]                                    # samples where the two signals agree: exact zeros
        cm = [rng.normal(0, 1, size=(L, F)).astype(np.float32) for L in n_bins]
        if sp.get("no_cmean") is not None:
            cm[sp["no_cmean"]] = None
        ld_out = -(-nc // 4) * 4 + 4
        shift = 1 if sp.get("draw_shift") else 0
        xt, dt = torch.from_numpy(x).cuda(), torch.from_numpy(xd).cuda()
        ct = [None if c is None else torch.from_numpy(c).cuda() for c in cm]
        out = torch.full((F * ld_out + 8,), GUARD, device="cuda")
        keep += [xt, dt, ct, out]
        j = jobs[k]
        j["raw"], j["ld"], j["col0"], j["ncols"], j["flip"] = xt.data_ptr(), ld, col0, nc, int(sp.get("flip", 0))
        if not sp.get("no_donor"):
            j["raw_donor"], j["ld_donor"] = dt.data_ptr(), ld
        for r in range(nres):
            j["cmean"][r] = 0 if ct[r] is None else ct[r].data_ptr()
        j["draw"], j["ld_out"] = out.data_ptr() + 4 * shift, ld_out
        host.append((x, None if sp.get("no_donor") else xd, cm, out, ld_out, shift))
    tab = torch.from_numpy(jobs.view(np.uint8)).cuda()
    cb, cl = (C.c_int * nres)(*binsizes), (C.c_int * nres)(*n_bins)
    max_cols = max(sp["ncols"] for sp in specs)
    st = torch.cuda.current_stream().cuda_stream
    L = _lib.lib()
    assert L.cf_bin_spread_difference(C.c_void_p(tab.data_ptr()), len(specs), F, nres, cb, cl, max_cols, st) == 0, L.cf_last_error()
    torch.cuda.synchronize()
    g7 = 7 * U / (1 - 7 * U)
    for sp, (x, xd, cm, out, ld_out, shift) in zip(specs, host):
        nc = sp["ncols"]
        flat = out.cpu().numpy().astype(np.float64)
        assert np.all(flat[:shift] == GUARD) and np.all(flat[shift + F * ld_out:] == GUARD), sp
        got = flat[shift:shift + F * ld_out].reshape(F, ld_out)
        assert np.all(got[:, nc:] == GUARD), (sp, "an element past ncols was written")
        ref, mag = spread_reference(x, xd, sp.get("col0", 8), nc, sp.get("flip", 0), binsizes, n_bins, cm)
        err = np.abs(got[:, :nc] - ref)
        print(sp, "max err / bound", float((err / np.maximum(g7 * mag, 1e-300)).max()), "max |ref|", float(np.abs(ref).max()))
        assert np.all(err <= g7 * mag + 16 * 2.0 ** -53 * mag), (sp, float(err.max()))
        assert np.all(got[:, :nc][mag == 0] == 0) and np.abs(ref).max() > 0
        assert xd is None or nc < 60 or bool((mag == 0).any())      # (samples where the two signals agree)


def test_spread_against_the_numpy_reference():
    """cf_bin_spread_difference on jobs built directly.  Bound, from the operation count: per sample the device rounds x - xd once, the
    three quotients C_r / cnt_r once each, the two additions of the sum once each and the final product once -- seven roundings of
    relative size u = 2^-24, each acting on a partial result no larger than |x - xd| sum_r |C_r| / cnt_r, so
    |device - exact| <= ((1 + u)^7 - 1) |x - xd| sum_r |C_r| / cnt_r <= gamma_7 |x - xd| sum_r |C_r| / cnt_r, gamma_7 = 7 u / (1 - 7 u)
    (the fp16 samples, the fp32 cmean and the integer counts are exact inputs; the float64 reference adds 16 * 2^-53 of the same
    magnitude at the most).  Fewer resolutions, a null donor or a null cmean[r] only drop roundings."""
    bins, L = [2000, 500, 100], [20, 80, 400]
    specs = []
    for flip in (0, 1):
        for nc in (60, 1234, 6000, 6001, 40000):      # below the finest bin | no multiple of 4 | coarsest bins exactly | one past | full
            specs.append(dict(ncols=nc, flip=flip))
    specs.append(dict(ncols=6001, flip=1, no_donor=True))
    specs.append(dict(ncols=1234, flip=0, no_cmean=1))
    specs.append(dict(ncols=1, flip=0))
    _spread_case(bins, L, specs)
    # the per-sample walk by three routes: an odd ld, a draw offset by 4 bytes, bin sizes that do not nest
    _spread_case(bins, L, [dict(ncols=nc, flip=f, odd_ld=True) for nc in (60, 1234, 6001) for f in (0, 1)], seed=4)
    _spread_case(bins, L, [dict(ncols=nc, flip=f, draw_shift=True) for nc in (1234, 6000, 40000) for f in (0, 1)], seed=5)
    _spread_case([2000, 300, 100], [20, 134, 400], [dict(ncols=nc, flip=f) for nc in (60, 1234, 6001, 40000) for f in (0, 1)], seed=6)
    _spread_case([500, 100], [80, 400], [dict(ncols=nc, flip=f) for nc in (1234, 6001) for f in (0, 1)], seed=7)


def test_spread_refusals():
    from chromoformer_amd.data import BIN_SPREAD_JOB
    L = _lib.lib()
    x = torch.zeros(7, 64, dtype=torch.float16, device="cuda")
    out = torch.full((7 * 64,), GUARD, device="cuda")
    cb, cl = (C.c_int * 3)(2000, 500, 100), (C.c_int * 3)(20, 80, 400)
    st = torch.cuda.current_stream().cuda_stream
    for kw, msg in ((dict(ld_out=32), b"ld_out"), (dict(ncols=60, max_cols=40), b"max_cols"), (dict(ld=40), b"does not fit"),
                    (dict(raw=0), b"null raw")):
        j = np.zeros(1, dtype=BIN_SPREAD_JOB)
        j[0]["raw"], j[0]["ld"], j[0]["ncols"], j[0]["draw"], j[0]["ld_out"] = x.data_ptr(), 64, 60, out.data_ptr(), 64
        for k, v in kw.items():
            if k != "max_cols":
                j[0][k] = v
        tab = torch.from_numpy(j.view(np.uint8)).cuda()
        assert L.cf_bin_spread_difference(C.c_void_p(tab.data_ptr()), 1, 7, 3, cb, cl, kw.get("max_cols", 64), st) != 0, kw
        assert msg in L.cf_last_error() and b"cf_bin_spread_difference" in L.cf_last_error(), (kw, L.cf_last_error())
        torch.cuda.synchronize()
        assert bool((out == GUARD).all()), kw


# ----------------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def cell_types(tmp_path_factory):
    """-> (dataset, donor dataset, checkpoint path, parameters): the 20-gene dataset at the CLI's geometry and a donor over the same regions."""
    ds = so.scan_dataset(str(tmp_path_factory.mktemp("genes")), w_prom=40000)
    dn = do.donor_dataset(ds.npy_dir, str(tmp_path_factory.mktemp("donor")), do.DONOR_SEED, w_prom=40000)
    P = orc.init_params(seed=7)
    ck = str(tmp_path_factory.mktemp("ck") / "w.pt")
    torch.save({"net": P}, ck)
    return ds, dn, ck, P


def test_generator_and_cli_end_to_end(cell_types, tmp_path):
    """The generator's keys and shapes; per gene the tracks against the per-bin attr of the same call rebuilt from the chunk -- the
    sums differ by what fp32 rounding allows: each track value carries gamma_7 of its magnitude (the spread, above), and the device's
    m - md comes from fp32 bin means (a sum of cnt <= b samples and a division: at most (b + 2) u relative) through log1pf and expm1f
    (2 u each on the feature, which expm1 turns into (1 + m) log1p(m) of absolute error), so a bin contributes at most
    u ((b + 2) m + 4 (1 + m) log1p(m)) |C| for each of m and md -- and delta, which the device sums in fp32 over some 64 levels of
    additions, reproduced from the yielded values within the same bound; the CLI's files carry the generator's bits."""
    from chromoformer_amd import predict
    from chromoformer_amd.attribution import _RawChunk
    ds, dn, ck, P = cell_types
    ids, n, t = list(ds.target_genes), 4, 1
    model = _model(None, False, P, 32)
    out = list(model.raw_integrated_gradients(ds, n_steps=n, donor_dataset=dn))
    plain = {d["gene_id"]: d for d in model.raw_integrated_gradients(ds, genes=ids[:2], n_steps=n)}
    assert [d["gene_id"] for d in out] == ids
    n_bins = [ds.w_max // b for b in ds.binsizes]
    ch, dch = _RawChunk(model, ds, ids, list(ds.binsizes), n_bins), _RawChunk(model, dn, ids, list(ds.binsizes), n_bins)
    donor = ({b: dch.pf[r] for r, b in enumerate(ds.binsizes)}, {b: dch.cf[r] for r, b in enumerate(ds.binsizes)})
    attr, info = model.integrated_gradients(*ch.model_args(), target=t, n_steps=n, inputs=FEATS, path="signal", donor=donor)
    with torch.no_grad():
        own = model(*dch.model_args()).cpu().numpy()
    g7 = 7 * U / (1 - 7 * U)
    for i, d in enumerate(out):
        assert sorted(d) == sorted(("gene_id", "logits", "baseline_logits", "delta", "donor_prediction", "promoter", "pcres", "regions"))
        g = ds.genes[d["gene_id"]]
        assert d["promoter"].shape == (7, 40000) and d["promoter"].dtype == np.float32 and len(d["pcres"]) == len(g["pcres"])
        assert all(p.shape == (7, e - s) for p, (_, s, e) in zip(d["pcres"], g["pcres"]))
        assert d["logits"].shape == (2,) and d["baseline_logits"].shape == (2,) and d["donor_prediction"].shape == (2,) and d["delta"].shape == ()
        assert np.array_equal(d["logits"], info["logits"][i].cpu().numpy()) and np.array_equal(d["delta"], info["delta"][i].cpu().numpy())
        assert np.array_equal(d["baseline_logits"], info["baseline_logits"][i].cpu().numpy()) and np.array_equal(d["donor_prediction"], own[i])
        if d["gene_id"] in plain:
            assert np.array_equal(d["logits"], plain[d["gene_id"]]["logits"]) and "donor_prediction" not in plain[d["gene_id"]]
        tracks = [d["promoter"]] + d["pcres"]
        total = sum(float(p.astype(np.float64).sum()) for p in tracks)
        tol = g7 * sum(float(np.abs(p.astype(np.float64)).sum()) for p in tracks)
        at = at_abs = 0.0
        for r, b in enumerate(ds.binsizes):
            for k, u, ud in (("promoter_feats", ch.pf[r][i], dch.pf[r][i]), ("pcre_feats", ch.cf[r][i], dch.cf[r][i])):
                a_ = attr[k][b][i].double().cpu()
                c_ = info["cmean"][k][b][i].double().cpu().reshape(a_.shape)
                at += float(a_.sum())
                at_abs += float(a_.abs().sum())
                for m in (torch.expm1(u.double().cpu()).reshape(a_.shape), torch.expm1(ud.double().cpu()).reshape(a_.shape)):
                    tol += float((U * ((b + 2) * m + 4 * (1 + m) * torch.log1p(m)) * c_.abs()).sum())
                tol += U * float(a_.abs().sum())                                    # attr = fl(d C)
        gap = float(d["logits"][t]) - float(d["baseline_logits"][t])
        print(d["gene_id"], "tracks - attr", total - at, "tol", tol, "delta", float(d["delta"]), "from the tracks", total - gap)
        assert abs(total - at) <= tol, (d["gene_id"], total - at, tol)
        assert abs((total - gap) - float(d["delta"])) <= tol + 64 * U * at_abs + 2 * U * abs(gap), d["gene_id"]
    # the CLI: one .npz per gene with the generator's bits
    out_dir = str(tmp_path / "rawdonorig")
    meta = os.path.join(ds.npy_dir, "meta.csv")
    assert predict.main(["-m", meta, "-d", ds.npy_dir, "-w", ck, "-o", str(tmp_path / "p.csv"), "--donor-npy-dir", dn.npy_dir,
                         "--raw-donor-ig-dir", out_dir, "--ig-steps", str(n)]) == 0
    assert sorted(os.listdir(out_dir)) == sorted("%s.npz" % g for g in ids)
    table = pd.read_csv(meta).set_index("gene_id")
    for d in out:
        z = np.load(os.path.join(out_dir, "%s.npz" % d["gene_id"]))
        names = table.loc[d["gene_id"], "neighbors"]
        names = names.split(";") if isinstance(names, str) else []
        assert sorted(z.files) == sorted(["promoter", "logits", "baseline_logits", "delta", "donor_prediction", "regions"]
                                         + ["pcre_%d" % s for s in range(len(names))])
        for k in ("promoter", "logits", "baseline_logits", "delta", "donor_prediction"):
            assert np.array_equal(z[k], d[k]), (d["gene_id"], k)
        assert all(np.array_equal(z["pcre_%d" % s], p) for s, p in enumerate(d["pcres"]))
        assert list(z["regions"]) == ["%s:%d-%d" % tuple(r) for r in d["regions"]]


def test_generator_refuses_other_regions(cell_types, tmp_path):
    ds, dn, ck, P = cell_types
    other = so.scan_dataset(str(tmp_path / "g"), w_prom=39000)
    model = _model(None, False, P, 8)
    with pytest.raises(ValueError, match="same_regions"):
        next(model.raw_integrated_gradients(ds, n_steps=2, donor_dataset=other))


# ----------------------------------------------------------------------------------------------------------------- the C ABI
def test_c_abi_refuses_by_name_before_any_launch():
    B, n = 3, 3
    batch = _batch(B, 55)
    donor = _dev(_donor(batch, 56))
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
        for r, b in enumerate(model.binsizes):
            op.base_promoter_feats[r], op.base_pcre_feats[r] = donor[0][b].data_ptr(), donor[1][b].data_ptr()
        for k, v in kw.items():
            setattr(op, k, v)
        return op

    st = torch.cuda.current_stream().cuda_stream

    def call(op, o, co, ts):
        return L.cf_integrated_gradients_raw_donor(model._handle, C.byref(bs), C.byref(op), C.byref(o), C.byref(co) if co is not None else None,
                                                   ts[-3].data_ptr(), ts[-2].data_ptr(), ts[-1].data_ptr(), st)

    o, co, ts = outs()
    assert call(opts(), o, co, ts) == 0, L.cf_last_error()
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t_).all()) for t_ in ts)
    first = [t_.clone() for t_ in ts]
    o, co, ts = outs()
    assert call(opts(), o, None, ts) == 0, L.cf_last_error()          # cmean may be NULL: the same attr
    torch.cuda.synchronize()
    n_attr = 2 * len(model.n_bins) + 1
    assert all(torch.equal(x, y) for x, y in zip(first[:n_attr] + first[-3:], ts[:n_attr] + ts[-3:]))
    assert all(bool(torch.isnan(t_).all()) for t_ in ts[n_attr:-3])
    f0 = C.c_int()
    _lib.check(L.cf_launch_counts(model._handle, C.byref(f0), None, None), "cf_launch_counts")
    hole_p = (C.c_void_p * 3)(donor[0][2000].data_ptr(), None, donor[0][100].data_ptr())
    hole_c = (C.c_void_p * 3)(donor[1][2000].data_ptr(), donor[1][500].data_ptr(), None)
    for kw, msg in ((dict(n_steps=0), b"n_steps"), (dict(target=2), b"target"), (dict(interpolate=0), b"interpolate"),
                    (dict(interpolate=8), b"interpolate"), (dict(interpolate=3), b"interaction_freq"), (dict(alphas=None), b"alphas"),
                    (dict(interpolate=4), b"signal path needs"), (dict(base_promoter_feats=hole_p), b"donor's features are required"),
                    (dict(base_pcre_feats=hole_c), b"donor's features are required"), (dict(base_broadcast=1), b"base_broadcast")):
        o, co, ts = outs()
        assert call(opts(**kw), o, co, ts) != 0, kw
        assert msg in L.cf_last_error() and b"cf_integrated_gradients_raw_donor" in L.cf_last_error(), (kw, L.cf_last_error())
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(t_).all()) for t_ in ts), kw      # nothing launched
    o, co, ts = outs()                                                 # a cmean field for an input that is not interpolated
    for r in range(3):
        o.promoter_feats[r] = None
    assert call(opts(interpolate=6), o, co, ts) != 0 and b"cmean promoter_feats" in L.cf_last_error(), L.cf_last_error()
    o, co, ts = outs()
    co.interaction_freq = ts[n_attr - 1].data_ptr()
    assert call(opts(), o, co, ts) != 0 and b"cmean interaction_freq" in L.cf_last_error(), L.cf_last_error()
    o, co, ts = outs()
    assert L.cf_integrated_gradients_raw_donor(None, C.byref(bs), C.byref(opts()), C.byref(o), C.byref(co), ts[-3].data_ptr(), ts[-2].data_ptr(),
                                               ts[-1].data_ptr(), st) != 0 and b"null handle" in L.cf_last_error()
    bs.B = 9
    assert call(opts(), o, co, ts) != 0 and b"max_batch" in L.cf_last_error()
    bs.B = B
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t_).all()) for t_ in ts)
    f1 = C.c_int()
    _lib.check(L.cf_launch_counts(model._handle, C.byref(f1), None, None), "cf_launch_counts")
    assert f1.value == f0.value
    # the Python keyword: a donor of the wrong size, a broadcast frequency baseline next to a donor
    with pytest.raises(ValueError, match="integrated_gradients: donor"):
        model.integrated_gradients(*_args(batch), n_steps=2, path="signal", donor=tuple({b: t[:2] for b, t in d.items()} for d in donor))
    with pytest.raises(ValueError, match="one row per gene"):
        model.integrated_gradients(*_args(batch), n_steps=2, path="signal", donor=donor,
                                   baselines={"interaction_freq": torch.zeros(1, T, T)})
    del keep


def test_no_side_effects_on_training_and_a_stale_backward_is_refused():
    from chromoformer_amd.engine import Trainer
    batches = [orc.synthetic_batch(8, seed=41 + i, regime="realistic") for i in range(3)]
    donor = _dev(_donor(batches[2], 9))
    P = _params(None, False)

    def run(interpose):
        model = _model(None, False, P, 8)
        tr = Trainer(model, lr=1e-3)
        slots = [tr.stage(b) for b in batches[:2]]
        tr.step(slots[0])
        torch.cuda.synchronize()
        snap = [t.clone() for t in (model._flat, model._gflat, model._mflat, model._vflat)]
        if interpose:
            model.integrated_gradients(*_args(batches[2]), n_steps=6, path="signal", donor=donor)
            model.integrated_gradients(*_args(batches[2]), n_steps=6, inputs=("pcre_feats",), path="signal", donor=donor)
            torch.cuda.synchronize()
            for a, b in zip(snap, (model._flat, model._gflat, model._mflat, model._vflat)):
                assert torch.equal(a, b)
        tr.step(slots[1])
        tr.step(slots[0])
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
        attr, info = model.integrated_gradients(*_args(batches[2]), n_steps=4, path="signal", donor=donor)
        assert not info["logits"].requires_grad and not info["cmean"]["pcre_feats"][100].requires_grad
        assert all(torch.equal(p.grad, grads[k]) for k, p in model.named_parameters() if k in grads)
        with pytest.raises(RuntimeError, match="integrated_gradients"):
            out[:, 1].sum().backward()
