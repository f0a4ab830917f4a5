"""Cost of model.integrated_gradients (cf_integrated_gradients: B x (n_steps + 2) interpolated rows through forward + backward, no
weight-gradient reductions) against what a user does without it -- the hand-written loop over the public API: per node a
grad-enabled model(...) on xb + a_k (x - xb) and backward() (which also runs the reductions into p.grad) -- default model,
realistic-regime batch, zero baseline, Gauss-Legendre, HIP events around N calls each:

    python tools/ig_step.py [--steps N] [--batch B] [--n-steps K]

  (a) integrated_gradients, max_batch = B          (chunks of B rows)
  (b) integrated_gradients, max_batch = 512
  (c) the hand-written loop (K forward + backward pairs, .grad summed in node order, times x - xb)
  (d) integrated_gradients, inputs = ("interaction_freq",), max_batch = B   (the trunk once)

The per-kernel split comes from a kernel trace of the same run:

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/ig_step.py --steps 2
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from chromoformer_amd import ChromoformerClassifier  # noqa: E402
from chromoformer_amd.attribution import ig_quadrature  # noqa: E402
from oracle import chromoformer_oracle as orc  # noqa: E402

KEYS = ("promoter_feats", "pcre_feats", "interaction_freq")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--n-steps", type=int, default=50)
    a = ap.parse_args()
    batch = orc.synthetic_batch(a.batch, seed=2024, regime="realistic")
    dev = {k: ({b: t.cuda() for b, t in v.items()} if isinstance(v, dict) else v.cuda()) for k, v in batch.items()}
    args = lambda d: (d["promoter_feats"], d["promoter_pad_masks"], d["pcre_feats"], d["pcre_pad_masks"],  # noqa: E731
                      d["interaction_masks"], d["interaction_freq"])
    chunked = ChromoformerClassifier(seed=42, max_batch=a.batch).cuda(0)
    wide = ChromoformerClassifier(seed=42, max_batch=max(512, a.batch)).cuda(0)
    p_chunked, p_wide = chunked.pack_batch(batch), wide.pack_batch(batch)
    alphas, weights = ig_quadrature("gausslegendre", a.n_steps)

    def hand_loop():
        acc = None
        for al, w in zip(alphas, weights):
            al, w = float(al), float(w)
            cur = dict(dev)
            leaves = []
            for k in KEYS:
                x = dev[k]
                if isinstance(x, dict):
                    cur[k] = {b: (0 + al * (t - 0)).requires_grad_(True) for b, t in x.items()}
                    leaves += list(cur[k].values())
                else:
                    cur[k] = (0 + al * (x - 0)).requires_grad_(True)
                    leaves.append(cur[k])
            with torch.enable_grad():
                (chunked(*args(cur))[:, 1] * w).sum().backward()
            g = [t.grad for t in leaves]
            acc = g if acc is None else [p + q for p, q in zip(acc, g)]
        xs = [t for k in KEYS for t in (dev[k].values() if isinstance(dev[k], dict) else [dev[k]])]
        return [x * g for x, g in zip(xs, acc)]

    runs = {
        "(a) integrated_gradients, max_batch %d" % a.batch: lambda: chunked.integrated_gradients(p_chunked, n_steps=a.n_steps),
        "(b) integrated_gradients, max_batch %d" % max(512, a.batch): lambda: wide.integrated_gradients(p_wide, n_steps=a.n_steps),
        "(c) hand-written loop, %d forward + backward" % a.n_steps: hand_loop,
        "(d) interaction_freq only, max_batch %d" % a.batch: lambda: chunked.integrated_gradients(p_chunked, n_steps=a.n_steps,
                                                                                                  inputs=("interaction_freq",)),
    }
    times = {}
    for name, fn in runs.items():
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for i in range(a.steps + 1):
            if i == 1:
                ev[0].record()
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        times[name] = ev[0].elapsed_time(ev[1]) / a.steps
    attr, info = chunked.integrated_gradients(*args(dev), n_steps=a.n_steps)
    ref = hand_loop()
    got = [t for k in KEYS for t in (attr[k].values() if isinstance(attr[k], dict) else [attr[k]])]
    same = all(torch.equal(g.reshape(r.shape), r) for g, r in zip(got, ref))
    gap = (info["logits"][:, 1] - info["baseline_logits"][:, 1]).abs()
    print("bsz %d, n_steps %d, %d rows, %d calls each (HIP events, ms per call):" % (a.batch, a.n_steps, a.batch * (a.n_steps + 2), a.steps))
    for name, t in times.items():
        print("  %-46s %.3f" % (name, t))
    tc = times[list(times)[2]]
    print("  ratios to (c): (a) %.3f  (b) %.3f  (d) %.3f" % (times[list(times)[0]] / tc, times[list(times)[1]] / tc, times[list(times)[3]] / tc))
    print("  (a) == hand-written loop, bit for bit: %s;  |delta| / |F(x) - F(xb)|: median %.2e, max %.2e" % (
        same, float((info["delta"].abs() / gap).median()), float((info["delta"].abs() / gap).max())))


if __name__ == "__main__":
    main()
