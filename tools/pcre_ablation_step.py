"""Cost of model.pcre_ablation (cf_pcre_ablation: the trunk once, the Regulation stack + head on B x (i_max + 2) gene-variants)
against what a user does without it -- one inference forward per explicitly masked copy of the batch -- default model, bsz 64,
realistic-regime batch, HIP events around N calls each:

    python tools/pcre_ablation_step.py [--steps N] [--batch B]

  (a) pcre_ablation, max_batch = B          (i_max + 2 chunks of B gene-variants)
  (b) pcre_ablation, max_batch = B (i_max + 2)   (one chunk)
  (c) i_max + 2 inference forwards (cf_forward(save = 0)) of the masked batches, packed beforehand

The per-kernel split comes from a kernel trace of the same run:

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/pcre_ablation_step.py
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from chromoformer_amd import ChromoformerClassifier  # noqa: E402
from oracle import chromoformer_oracle as orc  # noqa: E402
from tests.ablation_oracle import variant_masks  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    batch = orc.synthetic_batch(a.batch, seed=2024, regime="realistic")
    chunked = ChromoformerClassifier(seed=42, max_batch=a.batch).cuda(0)
    V = chunked.i_max + 2
    whole = ChromoformerClassifier(seed=42, max_batch=a.batch * V).cuda(0)
    p_chunked, p_whole = chunked.pack_batch(batch), whole.pack_batch(batch)
    masked = [chunked.pack_batch(variant_masks(batch, v, chunked.i_max)) for v in range(V)]

    def forwards():
        for p in masked:
            chunked._run_forward(p[0], save=False)

    runs = {
        "(a) pcre_ablation, max_batch %d" % a.batch: lambda: chunked.pcre_ablation(p_chunked),
        "(b) pcre_ablation, max_batch %d" % (a.batch * V): lambda: whole.pcre_ablation(p_whole),
        "(c) %d inference forwards of masked batches" % V: forwards,
    }
    times = {}
    for name, fn in runs.items():
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for i in range(a.steps + 5):
            if i == 5:
                ev[0].record()
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        times[name] = ev[0].elapsed_time(ev[1]) / a.steps
    # the results agree: column v of the ablation is the forward of masked batch v, bit for bit
    got = chunked.pcre_ablation(p_chunked)
    same = all(torch.equal(got[:, v], chunked._run_forward(masked[v][0], save=False)) for v in range(V))
    launches = {}
    for name, m, p in (("a", chunked, p_chunked), ("b", whole, p_whole)):
        m.pcre_ablation(p)
        launches[name] = m.launch_counts()[0]
    chunked._run_forward(p_chunked[0], save=False)
    n_fwd = chunked.launch_counts()[0]
    print("bsz %d, %d gene-variants, %d calls each (HIP events, ms per call):" % (a.batch, a.batch * V, a.steps))
    for name, t in times.items():
        print("  %-46s %.4f" % (name, t))
    tc = times["(c) %d inference forwards of masked batches" % V]
    print("  ratios to (c): (a) %.3f  (b) %.3f" % tuple(times[k] / tc for k in list(times)[:2]))
    print("  launches per call: (a) %d  (b) %d  (c) %d x %d;  ablation column v == forward of masked batch v: %s" % (
        launches["a"], launches["b"], V, n_fwd, same))


if __name__ == "__main__":
    main()
