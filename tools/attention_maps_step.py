"""Cost of model.attention_maps (cf_attention_maps: cf_forward(save = 1) + k_attn_maps) against a grad-enabled forward (cf_forward(save = 1)
alone) and an inference forward (save = 0), default model at bsz 64, HIP events around N calls each:

    python tools/attention_maps_step.py [--steps N] [--batch B]

The k_attn_maps launch alone comes from a kernel trace of the same run:

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/attention_maps_step.py
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
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    batch = orc.synthetic_batch(a.batch, seed=2024, regime="realistic")
    model = ChromoformerClassifier(seed=42, max_batch=a.batch).cuda(0)
    packed = model.pack_batch(batch)
    runs = {
        "attention_maps (all four outputs)": lambda: model.attention_maps(packed),
        "attention_maps (nothing requested)": lambda: model.attention_maps(packed, which=()),
        "grad-enabled forward (save = 1)": lambda: model._run_forward(packed[0], save=True),
        "inference forward (save = 0)": lambda: model._run_forward(packed[0], save=False),
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
    f, _, _ = model.launch_counts()
    model.attention_maps(packed)
    f_maps, _, _ = model.launch_counts()
    print("bsz %d, %d calls each (HIP events, ms per call):" % (a.batch, a.steps))
    for name, t in times.items():
        print("  %-38s %.4f" % (name, t))
    print("  attention_maps - grad-enabled forward: %+.4f ms; launches %d vs %d" % (
        times["attention_maps (all four outputs)"] - times["grad-enabled forward (save = 1)"], f_maps, f))


if __name__ == "__main__":
    main()
