"""Forward + backward of the default model at bsz 64 with gradients of every float input requested (saliency maps), then the same
without them; for a kernel trace of cf_backward_from_inputs against cf_backward_from:

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/input_grad_step.py [--steps N]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from chromoformer_amd import ChromoformerClassifier  # noqa: E402
from oracle import chromoformer_oracle as orc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    batch = orc.synthetic_batch(a.batch, seed=2024, regime="dense")
    model = ChromoformerClassifier(seed=42, max_batch=a.batch).cuda(0)
    dev = torch.device("cuda", 0)
    leaves = lambda want: ({b: t.to(dev).requires_grad_(want) for b, t in batch["promoter_feats"].items()},
                           {b: t.to(dev).requires_grad_(want) for b, t in batch["pcre_feats"].items()},
                           batch["interaction_freq"].to(dev).requires_grad_(want))
    masks = [{b: t.to(dev) for b, t in batch[k].items()} for k in ("promoter_pad_masks", "pcre_pad_masks", "interaction_masks")]
    times = {}
    for want in (True, False):
        pf, cf, fr = leaves(want)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for i in range(a.steps + 3):
            if i == 3:
                ev[0].record()
            for t in list(pf.values()) + list(cf.values()) + [fr]:
                t.grad = None
            model(pf, masks[0], cf, masks[1], masks[2], fr)[:, 1].sum().backward()
        ev[1].record()
        torch.cuda.synchronize()
        times[want] = ev[0].elapsed_time(ev[1]) / a.steps
    print("forward + backward, bsz %d: %.3f ms with input gradients, %.3f ms without (%+.1f %%)"
          % (a.batch, times[True], times[False], 100.0 * (times[True] / times[False] - 1)))


if __name__ == "__main__":
    main()
