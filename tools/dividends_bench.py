"""Harsanyi dividends against the loop a user would write and against the Shapley call they ride on:
python tools/dividends_bench.py [--out profiles/r25_dividends.json]

  (a) the transform at P = 16, B = 8 on a random table: model.shapley_dividends (k_moebius + k_moebius_high) against the same
      butterfly as 16 strided torch subtractions on the device (in place on a copy of the table; the copy is part of both legs: the
      operator writes a fresh output).  The two outputs must be bit-equal in this run, or the tool exits 1.
  (b) B = 64 genes (realistic regime), the seven marks as players, s = 0: one model.mark_dividends call (the 8,192 forwards, k_shapley,
      k_moebius with the mass) against one model.mark_shapley call.  Reported, not asserted: the difference next to the Shapley
      call's own min-max spread.
  (c) model.set_interactions at P = 16, B = 8, order 3 (696 sets, "sii"): one k_set_index launch.
The legs of (a), then of (b), are interleaved in one process and swap places every round; (c) runs alone.  HIP events around each call
(host launch overhead included: these are call times); median of --rounds rounds with min and max, two warm-up rounds.
Bytes: the transform's compulsory traffic is the table read once and the dividends written once; over the CALL time that is a lower
bound of what the kernels reach, stated against 8 TB/s as a fact, not a target (the kernels are latency-bound at this size).

  (d) kernel times need the profiler, in a run of its own:
    rocprofv3 --kernel-trace --stats -d OUT -o run --output-format csv -- python tools/dividends_bench.py --call-only
    python tools/dividends_bench.py --kernel-stats OUT/<host>/run_kernel_stats.csv --out profiles/r25_dividends.json
--call-only launches leg (a)'s operator and leg (c)'s three times each, nothing else."""
import argparse, csv, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from chromoformer_amd import ChromoformerClassifier
from chromoformer_amd.attribution import interaction_sets
from oracle import chromoformer_oracle as orc

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=11)
ap.add_argument("--call-only", action="store_true", help="the operator launches, nothing else (for a profiler run)")
ap.add_argument("--kernel-stats", default=None, help="rocprofv3 --stats CSV of a --call-only run: adds the kernels' times and bytes per second")
ap.add_argument("--out", default=None, help="also write the result line to this file")
a = ap.parse_args()
dev = torch.device("cuda", 0)
B, P16, B16, ORDER = 64, 16, 8, 3
KEYS = ("promoter_feats", "promoter_pad_masks", "pcre_feats", "pcre_pad_masks", "interaction_masks", "interaction_freq")
model = ChromoformerClassifier(seed=42, max_batch=B).cuda(0)
g = torch.Generator().manual_seed(16)
table = (torch.randn(B16, 1 << P16, 2, generator=g) * 3).to(dev)
sets = interaction_sets(P16, ORDER)


def operator():
    return model.shapley_dividends(table)


def butterfly():
    """The recurrence with torch on the device: stage k subtracts the half with bit k clear from the half with bit k set, in place."""
    x = table.clone()
    for k in range(P16):
        y = x.view(B16, (1 << P16) >> (k + 1), 2, 1 << k, 2)
        y[:, :, 1] -= y[:, :, 0]
    return x


div16 = operator()


def index():
    return model.set_interactions(div16, order=ORDER, index="sii", sets=sets)


if a.call_only:
    for _ in range(3):
        operator()
        index()
    torch.cuda.synchronize()
    sys.exit(0)

batch = orc.synthetic_batch(B, seed=77, regime="realistic")
args = tuple({b: t.to(dev) for b, t in batch[k].items()} if isinstance(batch[k], dict) else batch[k].to(dev) for k in KEYS)


def shapley():
    return model.mark_shapley(*args)


def dividends():
    return model.mark_dividends(*args)


same = bool(torch.equal(operator(), butterfly()))
(phi_s, info_s), (div7, info_d) = shapley(), dividends()
same_phi = bool(torch.equal(phi_s, info_d["phi"]))
torch.cuda.synchronize()
if not same:
    raise SystemExit("dividends_bench: cf_dividends_from_rows and the torch butterfly differ")
times = {k: [] for k in ("dividends_P16_B8", "torch_butterfly_P16_B8", "mark_shapley", "mark_dividends", "set_interactions_P16_B8_order3")}
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed(name, fn, keep):
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    if keep:
        times[name].append(e0.elapsed_time(e1))


# within a loop the two legs swap places every round (a leg that always follows the other would inherit its clocks and caches)
for legs in ((("dividends_P16_B8", operator), ("torch_butterfly_P16_B8", butterfly)), (("mark_shapley", shapley), ("mark_dividends", dividends)),
             (("set_interactions_P16_B8_order3", index),)):
    for rnd in range(2 + a.rounds):                  # two warm-up rounds
        for name, fn in (legs if rnd % 2 == 0 else legs[::-1]):
            timed(name, fn, rnd >= 2)
res = {}
for k, v in times.items():
    v = sorted(v)
    res[k] = {"ms_median": round(v[len(v) // 2], 4), "ms_min": round(v[0], 4), "ms_max": round(v[-1], 4), "rounds": len(v)}
res["butterfly_over_operator"] = round(res["torch_butterfly_P16_B8"]["ms_median"] / res["dividends_P16_B8"]["ms_median"], 2)
res["dividends_minus_shapley_ms"] = round(res["mark_dividends"]["ms_median"] - res["mark_shapley"]["ms_median"], 3)
res["shapley_spread_ms"] = round(res["mark_shapley"]["ms_max"] - res["mark_shapley"]["ms_min"], 3)
table_bytes = B16 * (1 << P16) * 2 * 4
# k_set_index: a set of s players reads its 2^(P - s) supersets once per output column
index_bytes = sum(B16 * (1 << (P16 - bin(int(s)).count("1"))) * 2 * 4 for s in sets)
kernels = {"table_bytes": table_bytes, "transform_compulsory_bytes": 2 * table_bytes, "transform_executed_bytes": 4 * table_bytes,
           "transform_executed_note": "k_moebius reads the table and writes the dividends, k_moebius_high reads and writes them again",
           "transform_call_TB/s_of_8": round(2 * table_bytes / res["dividends_P16_B8"]["ms_median"] / 1e9, 4),
           "set_index_read_bytes": index_bytes,
           "set_index_call_TB/s_of_8": round(index_bytes / res["set_interactions_P16_B8_order3"]["ms_median"] / 1e9, 4),
           "served_by": "the 4 MiB tables fit L2 / Infinity Cache: re-reads are not HBM traffic (stated from the sizes; no counter run)"}
if a.kernel_stats:
    with open(a.kernel_stats) as f:
        rows = list(csv.DictReader(f))
    for name in ("k_moebius", "k_moebius_high", "k_set_index"):
        hit = [r for r in rows if r["Name"].split("(")[0].split("<")[0].endswith(name)]
        if not hit:
            raise SystemExit("dividends_bench: no %s row in %s" % (name, a.kernel_stats))
        kernels[name + "_us"] = round(float(hit[0]["AverageNs"]) / 1e3, 2)
        kernels[name + "_calls_in_profile"] = int(hit[0]["Calls"])
    us = kernels["k_moebius_us"] + kernels["k_moebius_high_us"]
    kernels.update({"transform_kernels_us": round(us, 2), "transform_compulsory_TB/s_of_8": round(2 * table_bytes / us / 1e6, 3),
                    "transform_executed_TB/s_of_8": round(4 * table_bytes / us / 1e6, 3),
                    "set_index_TB/s_of_8": round(index_bytes / kernels["k_set_index_us"] / 1e6, 3),
                    "source": "rocprofv3 --kernel-trace --stats, a run of its own (--call-only)"})
else:
    kernels["kernel_time"] = "not measured"
line = json.dumps({"workload": "(a) the transform at P = 16, B = 8; (b) B = 64, the seven marks, s = 0: 8,192 forwards; (c) 696 sets at P = 16, B = 8",
                   "transform_bit_equal_to_torch_butterfly": same, "phi_bit_equal_to_mark_shapley": same_phi,
                   "timing": "HIP events around one call per leg; the legs of (a), then of (b), interleaved, swapping places every round; two warm-up rounds",
                   "ms": res, "kernels": kernels})
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(line + "\n")
