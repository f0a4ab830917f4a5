"""Pairwise Shapley interaction indices against the Shapley call they ride on and against the loop a user would write:
python tools/shapley_interactions_bench.py [--out profiles/r23_shapley_interactions.json]

  (a) B = 64 genes (realistic regime), the seven marks as players, s = 0: one model.mark_shapley_interactions call (the 8,192 forwards,
      k_shapley_pairs and k_shapley) against one model.mark_shapley call (the forwards and k_shapley).  Reported, not asserted: the
      difference next to the Shapley call's own min-max spread.
  (b) the operator at P = 16, B = 8 on a random table: model.shapley_interactions (one k_shapley_pairs launch, 136 workgroups per
      gene) against the torch loop over the 120 pairs on the device from the same table; both outputs' distance to the float64
      definition (tests/interaction_oracle.py) in units of its rounding bound.  No entry point runs k_shapley on a caller's table: the
      two reducers are compared on leg (a)'s table, in the profiler run below.
The two legs of (a), then of (b), are interleaved in one process and swap places every round; HIP events around each; median of
--rounds rounds with min and max, two warm-up rounds.

  (c) kernel times and bytes per second need the profiler, in a run of its own:
    rocprofv3 --kernel-trace --stats -d OUT -o run --output-format csv -- python tools/shapley_interactions_bench.py --call-only
    python tools/shapley_interactions_bench.py --kernel-stats OUT/<host>/run_kernel_stats.csv --out profiles/r23_shapley_interactions.json
--call-only launches k_shapley_pairs on leg (b)'s table three times, then leg (a)'s call once (its k_shapley_pairs and k_shapley share
the P = 7 table): of the CSV's k_shapley_pairs row the per-launch maximum is taken as the P = 16 time and the minimum as the P = 7 one;
the k_shapley row is the P = 7 launch.  Bytes of one launch: compulsory = the table once (B 2^P n_out 4 B); executed = every workgroup of a gene walks the whole
table once per output column in full cache lines, (P (P - 1) / 2 + P) n_out table reads per gene under sii."""
import argparse, csv, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from chromoformer_amd import ChromoformerClassifier
from chromoformer_amd.attribution import interaction_weights
from oracle import chromoformer_oracle as orc

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=11)
ap.add_argument("--index", default="sii", choices=("sii", "sti"))
ap.add_argument("--call-only", action="store_true", help="the reducer launches and one interactions call, nothing else (for a profiler run)")
ap.add_argument("--kernel-stats", default=None, help="rocprofv3 --stats CSV of a --call-only run: adds the reducers' times and bytes per second")
ap.add_argument("--out", default=None, help="also write the result line to this file")
a = ap.parse_args()
dev = torch.device("cuda", 0)
B, P16, B16 = 64, 16, 8
KEYS = ("promoter_feats", "promoter_pad_masks", "pcre_feats", "pcre_pad_masks", "interaction_masks", "interaction_freq")
batch = orc.synthetic_batch(B, seed=77, regime="realistic")
model = ChromoformerClassifier(seed=42, max_batch=B).cuda(0)
args = tuple({b: t.to(dev) for b, t in batch[k].items()} if isinstance(batch[k], dict) else batch[k].to(dev) for k in KEYS)
g = torch.Generator().manual_seed(16)
table = (torch.randn(B16, 1 << P16, 2, generator=g) * 3).to(dev)
w16 = torch.tensor(interaction_weights(P16, a.index), dtype=torch.float32, device=dev)
words = torch.arange(1 << P16, device=dev)
size = sum(words >> k & 1 for k in range(P16))


def shapley():
    return model.mark_shapley(*args)


def interactions():
    return model.mark_shapley_interactions(*args, index=a.index)


def pairs():
    return model.shapley_interactions(table, index=a.index)


def loop():
    """The off-diagonal entries with torch on the device, pair by pair, in the kernel's grouping (the summation order is torch's)."""
    out = torch.zeros(B16, P16, P16, 2, device=dev)
    for i in range(P16):
        for j in range(i + 1, P16):
            m = words[((words >> i | words >> j) & 1) == 0]
            d = (table[:, m | 1 << i | 1 << j] - table[:, m | 1 << j]) - (table[:, m | 1 << i] - table[:, m])
            out[:, i, j] = out[:, j, i] = (d * w16[size[m]][None, :, None]).sum(1)
    return out


if a.call_only:
    for _ in range(3):
        pairs()
    interactions()
    torch.cuda.synchronize()
    sys.exit(0)

from tests.interaction_oracle import pair_index_fp64      # noqa: E402
(phi_s, info_s), (inter, info_i) = shapley(), interactions()
same_phi = bool(torch.equal(phi_s, info_i["phi"]))
got, ref = pairs(), loop()
torch.cuda.synchronize()
I64, scale = pair_index_fp64(table.cpu().numpy(), a.index)
off = ~np.eye(P16, dtype=bool)
n = 2 ** (P16 - 2) + 5
bound = (n * 2.0 ** -24 / (1 - n * 2.0 ** -24) * scale)[:, off]
dist = {k: np.abs(x.cpu().numpy().astype(np.float64) - I64)[:, off] for k, x in (("k_shapley_pairs", got), ("torch_loop", ref))}
times = {k: [] for k in ("mark_shapley", "mark_shapley_interactions", "k_shapley_pairs_P16_B8", "torch_loop_P16_B8")}
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed(name, fn, keep):
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    if keep:
        times[name].append(e0.elapsed_time(e1))


# (a) and (b) in loops of their own, so that the torch loop's many small launches do not sit in front of a call leg; within a loop the
# two legs swap places every round (a leg that always follows the other would inherit its clocks and caches)
for pair in ((("mark_shapley", shapley), ("mark_shapley_interactions", interactions)),
             (("k_shapley_pairs_P16_B8", pairs), ("torch_loop_P16_B8", loop))):
    for rnd in range(2 + a.rounds):                  # two warm-up rounds
        for name, fn in (pair if rnd % 2 == 0 else pair[::-1]):
            timed(name, fn, rnd >= 2)
res = {}
for k, v in times.items():
    v = sorted(v)
    res[k] = {"ms_median": round(v[len(v) // 2], 3), "ms_min": round(v[0], 3), "ms_max": round(v[-1], 3), "rounds": len(v)}
res["interactions_minus_shapley_ms"] = round(res["mark_shapley_interactions"]["ms_median"] - res["mark_shapley"]["ms_median"], 3)
res["shapley_spread_ms"] = round(res["mark_shapley"]["ms_max"] - res["mark_shapley"]["ms_min"], 3)
res["loop_over_kernel"] = round(res["torch_loop_P16_B8"]["ms_median"] / res["k_shapley_pairs_P16_B8"]["ms_median"], 2)
table_bytes = B16 * (1 << P16) * 2 * 4
groups = P16 * (P16 - 1) // 2 + (P16 if a.index == "sii" else 0)
reducer = {"table_bytes": table_bytes, "executed_bytes": groups * 2 * table_bytes,
           "served_by": "the 4 MiB table is re-read by up to 136 workgroups per gene: beyond the first pass the reads are served by L2 / "
                        "Infinity Cache, not HBM (stated from the sizes; no counter run)"}
if a.kernel_stats:
    with open(a.kernel_stats) as f:
        rows = list(csv.DictReader(f))
    hit = {k: [r for r in rows if r["Name"].split("(")[0].endswith(k)] for k in ("k_shapley_pairs", "k_shapley")}
    if not hit["k_shapley_pairs"]:
        raise SystemExit("shapley_interactions_bench: no k_shapley_pairs row in %s" % a.kernel_stats)
    r = hit["k_shapley_pairs"][0]
    us = float(r.get("MaxNs") or r["AverageNs"]) / 1e3
    reducer.update({"k_shapley_pairs_P16_B8_us": round(us, 2), "calls_in_profile": int(r["Calls"]),
                    "compulsory_TB/s": round(table_bytes / us / 1e6, 4), "executed_TB/s": round(groups * 2 * table_bytes / us / 1e6, 3),
                    "k_shapley_pairs_P7_B64_us": round(float(r.get("MinNs") or r["AverageNs"]) / 1e3, 2),
                    "source": "rocprofv3 --kernel-trace --stats, a run of its own (--call-only)"})
    if hit["k_shapley"]:
        reducer["k_shapley_P7_B64_us"] = round(float(hit["k_shapley"][0]["AverageNs"]) / 1e3, 2)
else:
    reducer["kernel_time"] = "not measured"
line = json.dumps({"workload": "(a) B = 64, the seven marks, s = 0: 8,192 forwards; (b) the operator at P = 16, B = 8", "index": a.index,
                   "phi_bit_equal_to_mark_shapley": same_phi,
                   "timing": "HIP events around one call per leg; the two legs of (a), then of (b), interleaved, swapping places every round; two warm-up rounds", "ms": res,
                   "distance_to_fp64_over_bound": {k: {"max": round(float((v / np.maximum(bound, 1e-300)).max()), 4),
                                                        "max_abs": float(v.max())} for k, v in dist.items()},
                   "reducer": reducer})
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(line + "\n")
