"""Time integrated_gradients on the linear path and, where the tree has it, on the signal path: same model, B genes, n nodes, all
feature inputs; the paths interleaved in one process, HIP events, median (min / max) of the rounds.  With --raw-genes also the
per-gene time of raw_integrated_gradients on promoter-sized regions of a synthetic dataset.  Prints one JSON line.

    python tools/ig_path_bench.py --batch 64 --steps 50 --rounds 11 [--raw-genes 12]
"""
import argparse
import inspect
import json
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from chromoformer_amd import ChromoformerClassifier  # noqa: E402
from oracle import chromoformer_oracle as orc  # noqa: E402

KEYS = ("promoter_feats", "promoter_pad_masks", "pcre_feats", "pcre_pad_masks", "interaction_masks", "interaction_freq")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--raw-genes", type=int, default=0)
    args = ap.parse_args(argv)
    cfg = orc._cfg(None)
    model = ChromoformerClassifier(cfg["n_feats"], cfg["d_emb"], cfg["d_head"], cfg["embed"], cfg["pairwise_interaction"], cfg["regulation"],
                                   binsizes=cfg["binsizes"], seed=42, i_max=cfg["i_max"], w_max=cfg["w_max"], max_batch=args.batch).cuda(0)
    batch = orc.synthetic_batch(args.batch, seed=7, regime="realistic")
    dev = {k: ({b: t.cuda() for b, t in v.items()} if isinstance(v, dict) else v.cuda()) for k, v in batch.items() if k in KEYS}
    call = [dev[k] for k in KEYS]
    feats = ("promoter_feats", "pcre_feats")
    paths = ["linear"] + (["signal"] if "path" in inspect.signature(model.integrated_gradients).parameters else [])

    def run(path):
        kw = {} if path == "linear" else {"path": path}
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        model.integrated_gradients(*call, n_steps=args.steps, inputs=feats, **kw)
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    for p in paths:      # warm-up: buffers, LDS attribute
        run(p)
    times = {p: [] for p in paths}
    for _ in range(args.rounds):
        for p in paths:
            times[p].append(run(p))
    out = {"batch": args.batch, "n_steps": args.steps, "rounds": args.rounds, "inputs": list(feats), "unit": "ms per call"}
    for p in paths:
        out[p] = {"median": statistics.median(times[p]), "min": min(times[p]), "max": max(times[p])}
    if args.raw_genes and hasattr(model, "raw_integrated_gradients"):
        from chromoformer_amd.data import ChromoformerDataset
        import pandas as pd
        from tests.synth_data import make_dataset
        with tempfile.TemporaryDirectory() as d:
            meta = make_dataset(d, n_genes=args.raw_genes, seed=11)
            ds = ChromoformerDataset(meta, d, pd.read_csv(meta).gene_id.tolist())
            list(model.raw_integrated_gradients(ds, n_steps=args.steps))      # warm-up (file cache)
            rounds = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                n = len(list(model.raw_integrated_gradients(ds, n_steps=args.steps)))
                torch.cuda.synchronize()
                rounds.append(1e3 * (time.perf_counter() - t0) / n)
            out["raw_integrated_gradients"] = {"genes": n, "unit": "ms per gene, wall clock, files to host tracks", "median": statistics.median(rounds),
                                               "min": min(rounds), "max": max(rounds)}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
