"""Exact pCRE Shapley values against the loop a user would write today: python tools/coalition_bench.py [--out profiles/r12_pcre_shapley.json]

Shape: B = 64 genes (realistic regime), the default model (i_max = 8): 256 coalitions per gene, 16,384 Regulation + head rows.
  shapley  one model.pcre_shapley call (cf_pcre_shapley: the trunk once, 256 chunks of 64 rows built by k_coalition_expand, k_shapley);
  loop     existing public calls only: per coalition word the interaction masks edited with torch on the device, model(...) under
           no_grad on the 64 genes (256 full forwards, each re-running the trunk), then the Shapley sums with torch on the device.
The two legs are interleaved in one process; HIP events around each; median of --rounds rounds with min and max, two warm-up rounds.
The coalition logits of the two legs must be bit-equal before a time is reported."""
import argparse, json, os, sys
from math import factorial
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from chromoformer_amd import ChromoformerClassifier
from oracle import chromoformer_oracle as orc

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=11)
ap.add_argument("--out", default=None, help="also write the result line to this file")
a = ap.parse_args()
dev = torch.device("cuda", 0)
B, S = 64, 8
BINS = (2000, 500, 100)
N = 1 << S
batch = orc.synthetic_batch(B, seed=77, regime="realistic")
model = ChromoformerClassifier(seed=42, max_batch=B).cuda(0)
KEYS = ("promoter_feats", "promoter_pad_masks", "pcre_feats", "pcre_pad_masks", "interaction_masks", "interaction_freq")
d = {k: ({b: t.to(dev) for b, t in v.items()} if isinstance(v, dict) else v.to(dev)) for k, v in batch.items() if k in KEYS}
args = tuple(d[k] for k in KEYS)
words = torch.arange(N, device=dev)
size = torch.tensor([bin(m).count("1") for m in range(N)], device=dev)
w = torch.tensor([factorial(k) * factorial(S - k - 1) / factorial(S) for k in range(S)], dtype=torch.float32, device=dev)


def shapley():
    return model.pcre_shapley(*args, return_coalitions=True)


def loop():
    """The same values with existing public calls: 256 model(...) calls on edited masks, the subset formula with torch."""
    with torch.no_grad():
        v = torch.empty(B, N, 2, device=dev)
        for m in range(N):
            gone = [j + 1 for j in range(S) if not m >> j & 1]
            masks = {}
            for bs in BINS:
                im = d["interaction_masks"][bs].clone()
                im[:, 0, gone, :] = True
                im[:, 0, :, gone] = True
                masks[bs] = im
            v[:, m] = model(d["promoter_feats"], d["promoter_pad_masks"], d["pcre_feats"], d["pcre_pad_masks"], masks, d["interaction_freq"])
        phi = torch.empty(B, S, 2, device=dev)
        for j in range(S):
            sub = words[(words >> j & 1) == 0]
            phi[:, j] = ((v[:, sub | 1 << j] - v[:, sub]) * w[size[sub]][None, :, None]).sum(1)
        return phi, v


px, ix = shapley()
n_launch = model.launch_counts()[0]
py, vy = loop()
same = bool(torch.equal(ix["coalitions"], vy))
worst = float((ix["coalitions"] - vy).abs().max())
if not same:
    raise SystemExit("coalition_bench: the coalition logits of the two legs differ (max %.3e); no time is reported" % worst)
phi_diff = float((px - py).abs().max())      # (the summation orders differ: rounding only)
legs = {"shapley": shapley, "loop": loop}
times = {k: [] for k in legs}
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for rnd in range(2 + a.rounds):                      # two warm-up rounds
    for k, fn in legs.items():
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if rnd >= 2:
            times[k].append(e0.elapsed_time(e1))
res = {}
for k, t in times.items():
    t = sorted(t)
    res[k] = {"ms_median": round(t[len(t) // 2], 3), "ms_min": round(t[0], 3), "ms_max": round(t[-1], 3), "rounds": len(t)}
res["loop_over_shapley"] = round(res["loop"]["ms_median"] / res["shapley"]["ms_median"], 3)
line = json.dumps({"workload": "B = 64, default model, realistic regime: exact Shapley values of 8 pCRE slots, %d Regulation + head rows" % (B * N),
                   "coalition_logits_bit_equal": same, "phi_max_abs_diff": phi_diff, "launches_per_shapley_call": n_launch,
                   "timing": "HIP events around one call per leg, legs interleaved, two warm-up rounds", "call": res})
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(line + "\n")
