"""Greedy selection among the 63 (mark, region) players in one call against the loop a user could write before it:
python tools/backselect_bench.py [--out profiles/r26_backselect.json]

Shape: B = 64 genes (realistic regime), the default model, players "cells" (P = 63), backward mode, s = 0: P (P + 1) / 2 + 1 = 2,017
forwards per gene, 129,088 in all.
  call   one backselect.mark_backselect call (cf_mark_backselect: per round one k_backselect_step, then the round's B (P - t) rows in chunks
         of 64 on the per-gene word table; the host sees no logit);
  loop   public calls only, per gene and per round: model.mark_coalitions_wide on that gene's P - t candidates (one chunk), an argmax
         with torch, the pick read back (a host round trip per step) and the next candidate words built on the host.
The two legs alternate in one process; HIP events around each; median of --rounds rounds with min and max, one warm-up round.  Whether
the two legs pick the same orders is recorded, not assumed: the loop's rows run one gene at a time and bit-equality with the 64-gene
call is not promised off the fused trunk; a near-tie may then go the other way.

k_backselect_step's own time needs a kernel trace of a run of its own:
    rocprofv3 --kernel-trace --stats -d OUT -o run --output-format csv -- python tools/backselect_bench.py --call-only
    python tools/backselect_bench.py --kernel-stats OUT/<host>/run_kernel_stats.csv --out profiles/r26_backselect.json"""
import argparse, csv, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from chromoformer_amd import ChromoformerClassifier
from chromoformer_amd import backselect as bs
from oracle import chromoformer_oracle as orc

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=11)
ap.add_argument("--genes", type=int, default=64)
ap.add_argument("--call-only", action="store_true", help="two mark_backselect calls and nothing else (for a profiler run)")
ap.add_argument("--kernel-stats", default=None, help="rocprofv3 --stats CSV of a --call-only run: adds k_backselect_step's own time")
ap.add_argument("--out", default=None, help="also write the result line to this file")
a = ap.parse_args()
dev = torch.device("cuda", 0)
B, F, S, T = a.genes, 7, 8, 9
P = F * T
batch = orc.synthetic_batch(B, seed=77, regime="realistic")
model = ChromoformerClassifier(seed=42, max_batch=64).cuda(0)
KEYS = ("promoter_feats", "promoter_pad_masks", "pcre_feats", "pcre_pad_masks", "interaction_masks", "interaction_freq")
d = {k: ({b: t.to(dev) for b, t in v.items()} if isinstance(v, dict) else v.to(dev)) for k, v in batch.items() if k in KEYS}
args = tuple(d[k] for k in KEYS)
one = [tuple(({b: t[g:g + 1].contiguous() for b, t in d[k].items()} if isinstance(d[k], dict) else d[k][g:g + 1].contiguous()) for k in KEYS)
       for g in range(B)]      # the genes one at a time, sliced once


def call():
    return bs.mark_backselect(model, *args, players="cells")


def loop():
    """The same path with public calls: per gene and round one mark_coalitions_wide, a torch argmax, the pick read back."""
    orders = np.zeros((B, P), dtype=np.int32)
    for g in range(B):
        ends = model.mark_coalitions_wide(*one[g], keep=[0, (1 << P) - 1])
        s = 1.0 if float(ends[0, 1, 1]) >= float(ends[0, 0, 1]) else -1.0
        present = np.ones(P, dtype=bool)
        for t in range(P - 1):
            cand = np.flatnonzero(present)
            keep = np.repeat(present[None], len(cand), 0)
            keep[np.arange(len(cand)), cand] = False
            v = model.mark_coalitions_wide(*one[g], keep=keep)
            pick = int(torch.argmax(s * v[0, :, 1]))      # (the round trip: the next words depend on it)
            orders[g, t] = cand[pick]
            present[cand[pick]] = False
        orders[g, P - 1] = np.flatnonzero(present)[0]
    return orders


if a.call_only:
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    sys.exit(0)

legs = {"call": call, "loop": loop}
times, last = {k: [] for k in legs}, {}
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for rnd in range(1 + a.rounds):                      # one warm-up round
    for k, fn in legs.items():
        torch.cuda.synchronize()
        e0.record()
        last[k] = fn()
        e1.record()
        torch.cuda.synchronize()
        if rnd >= 1:
            times[k].append(e0.elapsed_time(e1))
res = {}
for k, v in times.items():
    v = sorted(v)
    res[k] = {"ms_median": round(v[len(v) // 2], 3), "ms_min": round(v[0], 3), "ms_max": round(v[-1], 3), "rounds": len(v)}
res["loop_over_call"] = round(res["loop"]["ms_median"] / res["call"]["ms_median"], 3)
order_c, info = last["call"]
order_c, order_l = order_c.cpu().numpy(), last["loop"]
agree = (order_c == order_l).all(1)
chunks = -(-2 * B // 64) + sum(-(-B * (P - t) // 64) for t in range(P - 1))
step = {"launches_per_call": P}
if a.kernel_stats:
    with open(a.kernel_stats) as f:
        hit = [r for r in csv.DictReader(f) if "k_backselect_step" in r["Name"]]
    if not hit:
        raise SystemExit("backselect_bench: no k_backselect_step row in %s" % a.kernel_stats)
    step.update({"us_average": round(float(hit[0]["AverageNs"]) / 1e3, 2), "calls_in_profile": int(hit[0]["Calls"]),
                 "source": "rocprofv3 --kernel-trace --stats, a run of its own"})
else:
    step["us_average"] = "not measured (no kernel trace was taken)"
line = json.dumps({"workload": "B = %d, one player per (mark, region) pair (P = %d), backward, s = 0: %d forwards in %d chunks of at most 64"
                               % (B, P, B * (P * (P + 1) // 2 + 1), chunks),
                   "timing": "HIP events around one call per leg, legs alternating, one warm-up round", "call": res,
                   "ms_per_chunk_call": round(res["call"]["ms_median"] / chunks, 4),
                   "orders_agree_genes": int(agree.sum()), "genes": B,
                   "first_move_agrees_genes": int((order_c[:, 0] == order_l[:, 0]).sum()),
                   "mean_size": float(info["size"].float().mean()), "k_backselect_step": step})
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(line + "\n")
