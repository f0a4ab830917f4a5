"""Time raw-signal integrated gradients against a donor cell type and the kernel that spreads it over the raw signals; the legs of a
comparison interleaved in one process, HIP events, median (min / max) of the rounds.  Prints one JSON line.

  * integrated_gradients(path="signal") without and with donor=: same model, B genes, n nodes, both feature inputs;
  * cf_bin_spread_difference (k_bin_spread_diff) against cf_bin_regions_multi_backward(times_input = 1) (k_bin_multi_bwd) on
    promoter-sized regions: 7 marks x 40,000 samples each, bin sizes 2000 / 500 / 100.  Bytes per second over the algorithmic
    bytes of each kernel -- the spread reads two fp16 signals and writes fp32 (8 bytes per sample), the backward reads one
    (6 bytes per sample); the cmean / dfeat gathers are left out -- set against 8 TB/s.

    python tools/raw_donor_ig_bench.py --batch 64 --steps 50 --rounds 11 --regions 4096
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from chromoformer_amd import ChromoformerClassifier, _lib  # noqa: E402
from chromoformer_amd.data import BIN_GRAD_JOB, BIN_SPREAD_JOB  # noqa: E402
from oracle import chromoformer_oracle as orc  # noqa: E402

KEYS = ("promoter_feats", "promoter_pad_masks", "pcre_feats", "pcre_pad_masks", "interaction_masks", "interaction_freq")
FEATS = ("promoter_feats", "pcre_feats")
HBM = 8e12


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def interleaved(legs, rounds):
    """legs: {name: callable} -> {name: {"median", "min", "max"}} in ms; one warm-up each, then the legs in turn per round."""
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            times[k].append(timed(fn))
    return {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()}


def ig_legs(batch, steps):
    cfg = orc._cfg(None)
    model = ChromoformerClassifier(cfg["n_feats"], cfg["d_emb"], cfg["d_head"], cfg["embed"], cfg["pairwise_interaction"], cfg["regulation"],
                                   binsizes=cfg["binsizes"], seed=42, i_max=cfg["i_max"], w_max=cfg["w_max"], max_batch=batch).cuda(0)
    b = orc.synthetic_batch(batch, seed=7, regime="realistic")
    dev = {k: ({s: t.cuda() for s, t in v.items()} if isinstance(v, dict) else v.cuda()) for k, v in b.items() if k in KEYS}
    call = [dev[k] for k in KEYS]
    g = torch.Generator().manual_seed(8)
    donor = tuple({s: (t * (0.3 + 1.4 * torch.rand(t.shape, generator=g))).cuda().contiguous() for s, t in b[k].items()} for k in FEATS)
    return {"zero_baseline": lambda: model.integrated_gradients(*call, n_steps=steps, inputs=FEATS, path="signal"),
            "donor": lambda: model.integrated_gradients(*call, n_steps=steps, inputs=FEATS, path="signal", donor=donor)}


def spread_legs(regions, F=7, ncols=40000, bins=(2000, 500, 100)):
    L = _lib.lib()
    n_bins = [40000 // b for b in bins]
    g = torch.Generator(device="cuda").manual_seed(3)
    raw = (4 * torch.rand(regions, F, ncols, device="cuda", generator=g)).half()
    don = (4 * torch.rand(regions, F, ncols, device="cuda", generator=g)).half()
    coef = [torch.randn(regions, nb, F, device="cuda", generator=g) for nb in n_bins]
    draw = torch.empty(regions, F, ncols, device="cuda")
    sj, bj = np.zeros(regions, dtype=BIN_SPREAD_JOB), np.zeros(regions, dtype=BIN_GRAD_JOB)
    for k in range(regions):
        for j in (sj[k], bj[k]):
            j["raw"], j["ld"], j["ncols"], j["draw"], j["ld_out"] = raw[k].data_ptr(), ncols, ncols, draw[k].data_ptr(), ncols
        sj[k]["raw_donor"], sj[k]["ld_donor"] = don[k].data_ptr(), ncols
        for r in range(len(bins)):
            sj[k]["cmean"][r] = bj[k]["dfeat"][r] = coef[r][k].data_ptr()
    st, bt = torch.from_numpy(sj.view(np.uint8)).cuda(), torch.from_numpy(bj.view(np.uint8)).cuda()
    cb, cl = (C.c_int * len(bins))(*bins), (C.c_int * len(bins))(*n_bins)
    stream = torch.cuda.current_stream().cuda_stream

    def spread():
        _lib.check(L.cf_bin_spread_difference(C.c_void_p(st.data_ptr()), regions, F, len(bins), cb, cl, ncols, stream), "cf_bin_spread_difference")

    def backward():
        _lib.check(L.cf_bin_regions_multi_backward(C.c_void_p(bt.data_ptr()), regions, F, len(bins), cb, cl, ncols, 1, stream),
                   "cf_bin_regions_multi_backward")

    samples = regions * F * ncols
    return {"k_bin_spread_diff": spread, "k_bin_multi_bwd": backward}, {"k_bin_spread_diff": 8 * samples, "k_bin_multi_bwd": 6 * samples}, (raw, don, coef, draw, st, bt)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--regions", type=int, default=4096)
    args = ap.parse_args(argv)
    out = {"batch": args.batch, "n_steps": args.steps, "rounds": args.rounds, "regions": args.regions, "unit": "ms per call"}
    out["integrated_gradients_signal"] = interleaved(ig_legs(args.batch, args.steps), args.rounds)
    ig = out["integrated_gradients_signal"]
    ig["donor_over_zero_baseline"] = ig["donor"]["median"] / ig["zero_baseline"]["median"]
    legs, nbytes, keep = spread_legs(args.regions)
    res = out["spread"] = interleaved(legs, args.rounds)
    for k, v in res.items():
        v["algorithmic_bytes"] = nbytes[k]
        v["bytes_per_second"] = nbytes[k] / (v["median"] * 1e-3)
        v["fraction_of_8_TB_per_s"] = v["bytes_per_second"] / HBM
    del keep
    print(json.dumps(out))


if __name__ == "__main__":
    main()
