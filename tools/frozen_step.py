"""Step time of training on a frozen trunk against the full step -- default model, bsz 64, dense-regime synthetic store (the bench
shape), one process, the three legs interleaved over `--repeats` rounds of `--steps` steps each (HIP events on the trainer's stream
around a round; `--warmup` steps of every leg first):

    python tools/frozen_step.py [--steps N] [--repeats R] [--warmup W] [--batch B] [--genes G]

  (a) the unfrozen fused step                           Trainer(model)
  (b) frozen trunk, no cache (the trunk forward runs)   Trainer(model, freeze_trunk=True)
  (c) frozen trunk from cached trunk outputs            Trainer(model, freeze_trunk=True) + EpochFeed(..., cache=TrunkCache)

Prints one JSON line: per leg the median over the rounds of the mean step time (us), the rounds' minimum / maximum and the spread
(max - min); the orderings the feature is expected to give -- (c) < (b) < (a), each by more than the spread of (a) -- as booleans.
The per-kernel split comes from a kernel trace of the same run:

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/frozen_step.py --repeats 3
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from chromoformer_amd import ChromoformerClassifier  # noqa: E402
from chromoformer_amd.engine import EpochFeed, Trainer, TrunkCache  # noqa: E402
from chromoformer_amd.synth import synthetic_store  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--genes", type=int, default=2048)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    store = synthetic_store(a.genes, dev, seed=2024, regime="dense")
    per_epoch = max(a.steps, a.warmup)
    g = torch.Generator().manual_seed(0)

    def epoch():
        idx = torch.cat([torch.randperm(a.genes, generator=g) for _ in range(per_epoch * a.batch // a.genes + 1)])
        return idx[: per_epoch * a.batch].view(per_epoch, a.batch).tolist()

    legs = {}
    for key, frozen, cached in (("a_unfrozen_fused", False, False), ("b_frozen_no_cache", True, False), ("c_frozen_cached", True, True)):
        model = ChromoformerClassifier(seed=42, max_batch=a.batch).cuda(0)
        tr = Trainer(model, lr=3e-5, freeze_trunk=frozen)
        cache = TrunkCache(model, store, a.batch) if cached else None
        legs[key] = (model, tr, EpochFeed(model, store, a.batch, max_batches=per_epoch, cache=cache))

    def run(key, n):
        model, tr, feed = legs[key]
        feed.begin_epoch(epoch()[:n], tr.stream)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        tr.step(feed.slot)                       # (the first step of an epoch may carry a gather launch of its own: not timed)
        ev[0].record(tr.stream)
        for _ in range(n - 1):
            tr.step(feed.slot)
        ev[1].record(tr.stream)
        torch.cuda.synchronize()
        if feed.check(tr.stream):
            raise RuntimeError("%s: the device-side gather reported errors" % key)
        return ev[0].elapsed_time(ev[1]) * 1e3 / (n - 1)

    for key in legs:
        run(key, a.warmup)
    times = {key: [] for key in legs}
    for _ in range(a.repeats):
        for key in legs:
            times[key].append(run(key, a.steps))
    out = {"tool": "frozen_step", "batch": a.batch, "genes": a.genes, "steps_per_round": a.steps - 1, "rounds": a.repeats, "warmup_steps": a.warmup,
           "unit": "us per step (HIP events; median over rounds of a round's mean)"}
    for key, t in times.items():
        out[key] = {"median": round(statistics.median(t), 2), "min": round(min(t), 2), "max": round(max(t), 2), "spread": round(max(t) - min(t), 2)}
    spread_a = out["a_unfrozen_fused"]["spread"]
    med = {k: out[k]["median"] for k in times}
    out["b_faster_than_a_by_more_than_spread_of_a"] = bool(med["a_unfrozen_fused"] - med["b_frozen_no_cache"] > spread_a)
    out["c_faster_than_b_by_more_than_spread_of_a"] = bool(med["b_frozen_no_cache"] - med["c_frozen_cached"] > spread_a)
    out["launches_fwd_bwd_opt"] = {k: list(legs[k][0].launch_counts()) for k in legs}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
