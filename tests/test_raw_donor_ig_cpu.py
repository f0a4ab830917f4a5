"""Integrated gradients in raw-signal space against a donor cell type, the parts that need no GPU:

  * the identity the device path rests on, in fp64 on the scan dataset and a donor dataset over the same regions (eight pCRE lengths,
    both strands, the promoter narrowed to 39,000 and mirrored): the per-bin cmean = C of the tensor-level oracle pushed through the
    spread formula equals integrated gradients computed directly from the two raw signals (autograd to the raw leaf xd + a (x - xd)
    per node, never a bin mean); per resolution the tracks sum, bin by bin, to attr = (m - md) C; padded bins get exact zeros;
  * completeness against the fp64 oracle's own forwards: the tracks' total differs from F(x) - F(xd) by the tensor-level delta, and
    at one node the attributions sum to the derivative of the forward along the path (a central difference of forwards);
  * the job record is 88 bytes in both mirrors and the new symbols are exported; the CLI and the keyword refuse misuse before the
    device."""
import ctypes as C

import numpy as np
import pytest
import torch

from chromoformer_amd import _lib
from chromoformer_amd.attribution import ig_quadrature64
from oracle import chromoformer_oracle as orc
from tests import donor_oracle as do
from tests import scan_oracle as so
from tests.raw_donor_ig_oracle import batch_on_raw_path, oracle_ig_from_raw_donor, oracle_ig_signal_donor, spread_reference


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """-> (dataset, donor dataset): built once, shared, never written."""
    ds = so.scan_dataset(str(tmp_path_factory.mktemp("genes")), w_prom=39000)
    dn = do.donor_dataset(ds.npy_dir, str(tmp_path_factory.mktemp("donor")), do.DONOR_SEED, w_prom=39000)
    return ds, dn


def test_bin_mean_identity_against_a_donor_in_fp64(data):
    """Tolerances of tests/test_raw_ig_cpu.py::test_bin_mean_identity_in_fp64: 1e-9 of the track's norm, 1e-9 relative per bin."""
    from chromoformer_amd.data import load_raw_regions, raw_window
    ds, dn = data
    ids = list(ds.target_genes)
    lengths = {e - s for g in ids for _, s, e in ds.genes[g]["pcres"]}
    assert len(ids) == 20 and len(lengths) >= 8 and {ds.genes[g]["tss"][2] for g in ids} == {"+", "-"} and ds.w_prom == 39000
    P = orc.init_params(seed=7)
    t, dt = 1, torch.float64
    a, w = ig_quadrature64("gausslegendre", 2)      # (the identity holds node by node: two nodes keep the 20-gene fp64 passes short)
    tracks, lx, lb = oracle_ig_from_raw_donor(ds, dn.npy_dir, P, ids, a, w, t, dt)
    with torch.no_grad():
        batch = batch_on_raw_path(ds, dn.npy_dir, ids, dt, 1.0)[0]
        donor = batch_on_raw_path(ds, dn.npy_dir, ids, dt, 0.0)[0]
    attr, cmean, lx2, lb2, delta = oracle_ig_signal_donor(P, batch, donor, a, w, t, dtype=dt)
    assert torch.equal(lx, lx2) and torch.equal(lb, lb2)
    n_bins = [ds.w_max // b for b in ds.binsizes]
    partial = mirrored = 0
    for i, g in enumerate(ids):
        total = 0.0
        donor_regs = {s: x for s, _, x in load_raw_regions(dn, g)}
        for s, flip, x in load_raw_regions(ds, g):
            c0, nc = raw_window(ds, s, x.shape[1])
            pick = (lambda d, b: d["promoter_feats"][b][i, 0]) if s < 0 else (lambda d, b: d["pcre_feats"][b][i, s])
            cm = [pick(cmean, b).numpy() for b in ds.binsizes]
            got, _ = spread_reference(x, donor_regs[s], c0, nc, flip, ds.binsizes, n_bins, cm)
            ref = tracks[g, s].numpy()
            assert np.abs(ref[:, :c0]).max(initial=0) == 0 and np.abs(ref[:, c0 + nc:]).max(initial=0) == 0
            ref = ref[:, c0:c0 + nc]
            assert np.linalg.norm(got - ref) <= 1e-9 * np.linalg.norm(ref), (g, s)
            total += got.sum()
            mirrored += bool(flip) and s < 0
            for r, (b, L) in enumerate(zip(ds.binsizes, n_bins)):        # one resolution at a time: bin sums of the track = attr
                one = [d if k == r else None for k, d in enumerate(cm)]
                tr, _ = spread_reference(x, donor_regs[s], c0, nc, flip, ds.binsizes, n_bins, one)
                n = min(-(-nc // b), L)
                left = -(-(L - n) // 2)
                at = pick(attr, b).numpy()
                seen = np.zeros(L, dtype=bool)
                for k in range(n):
                    p = L - 1 - (left + k) if flip else left + k
                    seen[p] = True
                    assert np.allclose(tr[:, k * b:(k + 1) * b].sum(1), at[p], rtol=1e-9, atol=1e-13 * np.abs(at).max()), (g, s, b, k)
                assert np.all(at[~seen] == 0)                              # padded bins: m = md = 0
                partial += nc % b != 0
        gap = float(lx[i, t] - lb[i, t])
        assert abs((total - gap) - float(delta[i])) <= 1e-9 * abs(gap) + 1e-12, (g, total - gap, float(delta[i]))
    assert partial > 0 and mirrored > 0


def test_completeness_against_the_fp64_forwards(data):
    """By the fundamental theorem of calculus the attributions are complete when, at every a, they sum to dF(x(a)) / da; the
    quadrature then integrates that derivative.  At one node a with weight 1 the sum of attr is checked against the central difference
    (F(x(a + h)) - F(x(a - h))) / 2h of the oracle's own forwards binned from the raw files.  The network is piecewise smooth (ReLU), so
    the difference must not straddle a kink: h = 1e-6 keeps the bracket 2e-6 wide.  The truncation term h^2 F''' / 6 is then
    negligible and the rounding term dominates: a forward in fp64 carries some 1e-13 of accumulated rounding (thousands of additions
    at 1e-16), divided by 2h = 2e-6 that is 5e-8; asserted: 1e-7 max(1, |dF/da|).  The many-node delta, the quadrature error itself, is
    printed per gene next to the gap it belongs to."""
    ds, dn = data
    ids = ["ENSGSYN00001", "ENSGSYN00000", "ENSGSYN00002"]
    P = orc.init_params(seed=7)
    Pd = {k: v.double() for k, v in P.items()}
    t, dt, h = 1, torch.float64, 1e-6
    with torch.no_grad():
        batch = batch_on_raw_path(ds, dn.npy_dir, ids, dt, 1.0)[0]
        donor = batch_on_raw_path(ds, dn.npy_dir, ids, dt, 0.0)[0]
    for a in (0.25, 0.8):
        attr, _, _, _, _ = oracle_ig_signal_donor(P, batch, donor, [a], [1.0], t, dtype=dt)
        total = sum(v.reshape(len(ids), -1).sum(1) for d in attr.values() for v in d.values())
        with torch.no_grad():
            up = orc.forward(Pd, batch_on_raw_path(ds, dn.npy_dir, ids, dt, a + h)[0], None)[:, t]
            dn_ = orc.forward(Pd, batch_on_raw_path(ds, dn.npy_dir, ids, dt, a - h)[0], None)[:, t]
        deriv = (up - dn_) / (2 * h)
        print("a = %.2f: sum of attr" % a, total, "dF/da", deriv)
        assert bool(((total - deriv).abs() <= 1e-7 * deriv.abs().clamp(min=1.0)).all()), (a, total, deriv)
    al, w = ig_quadrature64("gausslegendre", 16)
    _, _, lx, lb, delta = oracle_ig_signal_donor(P, batch, donor, al, w, t, dtype=dt)
    print("16 nodes: delta", delta, "gap", lx[:, t] - lb[:, t])
    assert bool((lx[:, t] != lb[:, t]).all())


def test_the_job_record_is_88_bytes_and_the_symbols_are_exported():
    from chromoformer_amd.data import BIN_SPREAD_JOB
    assert C.sizeof(_lib.cf_bin_spread_job) == 88 and BIN_SPREAD_JOB.itemsize == 88
    for name, _ in _lib.cf_bin_spread_job._fields_:
        assert getattr(_lib.cf_bin_spread_job, name).offset == BIN_SPREAD_JOB.fields[name][1], name
    L = _lib.lib()
    assert L.cf_abi_version() == 1
    for name in ("cf_integrated_gradients_raw_donor", "cf_bin_spread_difference"):
        assert name in _lib.SYMBOLS and getattr(L, name) is not None
    assert L.cf_bin_spread_difference(None, 0, 7, 3, None, None, 0, None) != 0
    assert L.cf_last_error() == b"cf_bin_spread_difference: null argument"
    assert L.cf_integrated_gradients_raw_donor(None, None, None, None, None, None, None, None, None) != 0
    assert b"cf_integrated_gradients_raw_donor" in L.cf_last_error() and b"null handle" in L.cf_last_error()


def test_cli_options_and_their_misuse(tmp_path):
    from chromoformer_amd import predict
    base = ["-m", "m.csv", "-d", "npy", "-o", "p.csv"]
    args = predict.build_parser().parse_args(base + ["--donor-npy-dir", "dn", "--raw-donor-ig-dir", "ig", "--ig-steps", "8"])
    assert args.raw_donor_ig_dir == "ig" and args.donor_npy_dir == "dn" and args.ig_steps == 8
    assert predict.build_parser().parse_args(base).raw_donor_ig_dir is None
    for extra in (["--raw-donor-ig-dir", "ig"],                                               # no donor signals
                  ["--raw-donor-ig-dir", "ig", "--donor-npy-dir", "dn", "--donor-store", "x.cfstore"],      # a store holds no raw signal
                  ["--donor-npy-dir", "dn"]):                                                 # donor signals nobody reads
        with pytest.raises(SystemExit) as e:
            predict.main(base + extra)
        assert e.value.code == 2, extra


def test_the_donor_keyword_refuses_misuse_before_the_device():
    from chromoformer_amd import ChromoformerClassifier
    cfg = orc._cfg(None)
    model = ChromoformerClassifier(cfg["n_feats"], cfg["d_emb"], cfg["d_head"], cfg["embed"], cfg["pairwise_interaction"], cfg["regulation"],
                                   binsizes=cfg["binsizes"], seed=1, i_max=cfg["i_max"], w_max=cfg["w_max"], max_batch=2)      # (never .cuda())
    batch = orc.synthetic_batch(2, seed=1, regime="realistic")
    args = [batch[k] for k in so.KEYS]
    donor = (batch["promoter_feats"], batch["pcre_feats"])
    with pytest.raises(ValueError, match="path='linear'"):
        model.integrated_gradients(*args, n_steps=2, donor=donor)
    base = {"pcre_feats": {b: torch.zeros_like(v[:1]) for b, v in batch["pcre_feats"].items()}}
    with pytest.raises(ValueError, match="the donor is the feature baseline"):
        model.integrated_gradients(*args, n_steps=2, baselines=base, path="signal", donor=donor)
    with pytest.raises(ValueError, match="needs promoter_feats or pcre_feats"):
        model.integrated_gradients(*args, n_steps=2, inputs=("interaction_freq",), path="signal", donor=donor)
