"""Permutation-sampled Shapley values of the 63 (mark, region) players against the loop a user would write with public calls:
python tools/mark_sampled_bench.py [--out profiles/r16_mark_sampled.json]

Shape: B = 64 genes (realistic regime), the default model, players "cells" (P = 63), n_perm = 16, s = 0: R = 2 + 16 * 62 = 994 rows per
gene, 63,616 forwards.
  call   one model.mark_shapley_sampled call (cf_mark_shapley_sampled: rows built by k_mark_expand, 994 chunks of 64, then
         k_perm_shapley);
  loop   public calls only: per 64 rows the prefix coalitions' inputs built with torch on the device (the same rule on the absent
         players' columns), model(...) under no_grad, then the estimator (mean and standard error over the orders) with torch.
The two legs are interleaved in one process; HIP events around each; median of --rounds rounds with min and max, two warm-up rounds.
The row logits of the two legs are compared for bit-equality in the same run (they must agree within 1e-4 before a time is reported).

k_mark_expand's bytes per second need the kernel's own time: run the call leg alone under the profiler and pass its statistics in,
    rocprofv3 --kernel-trace --stats -d OUT -o run --output-format csv -- python tools/mark_sampled_bench.py --call-only
    python tools/mark_sampled_bench.py --kernel-stats OUT/<host>/run_kernel_stats.csv --out profiles/r16_mark_sampled.json
Algorithmic bytes of one launch as in tools/mark_shapley_bench.py: every feature element read and written once, the masks and
frequencies likewise."""
import argparse, csv, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from chromoformer_amd import ChromoformerClassifier
from chromoformer_amd.attribution import shapley_permutations
from oracle import chromoformer_oracle as orc

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=11)
ap.add_argument("--perms", type=int, default=16)
ap.add_argument("--call-only", action="store_true", help="two mark_shapley_sampled calls and nothing else (for a profiler run)")
ap.add_argument("--kernel-stats", default=None, help="rocprofv3 --stats CSV of a --call-only run: adds k_mark_expand's time and bytes per second")
ap.add_argument("--out", default=None, help="also write the result line to this file")
a = ap.parse_args()
dev = torch.device("cuda", 0)
B, F, S, T = 64, 7, 8, 9
P, NP = F * T, a.perms
R = 2 + NP * (P - 1)
BINS, NB = (2000, 500, 100), (20, 80, 400)
batch = orc.synthetic_batch(B, seed=77, regime="realistic")
model = ChromoformerClassifier(seed=42, max_batch=B).cuda(0)
KEYS = ("promoter_feats", "promoter_pad_masks", "pcre_feats", "pcre_pad_masks", "interaction_masks", "interaction_freq")
d = {k: ({b: t.to(dev) for b, t in v.items()} if isinstance(v, dict) else v.to(dev)) for k, v in batch.items() if k in KEYS}
# compact centre rows of the pad masks (what a resident store holds)
for bs, L in zip(BINS, NB):
    d["promoter_pad_masks"][bs] = d["promoter_pad_masks"][bs].reshape(B, L, L)[:, L // 2].contiguous()
    d["pcre_pad_masks"][bs] = d["pcre_pad_masks"][bs].reshape(B, S, L, L)[:, :, L // 2].contiguous()
args = tuple(d[k] for k in KEYS)
perms = shapley_permutations(P, NP, 0)


def call():
    return model.mark_shapley_sampled(*args, players="cells", permutations=perms, return_rows=True)


def loop():
    """The same values with public calls: the prefix rows by torch, model(...) per 64 rows, mean and standard error by torch."""
    with torch.no_grad():
        pi = torch.from_numpy(perms.astype("int64")).to(dev)
        rank = torch.empty_like(pi).scatter_(1, pi, torch.arange(P, device=dev).expand(NP, P))      # rank[q, p]: the position of player p
        k = torch.arange(1, P, device=dev)
        present = torch.cat([torch.zeros(1, P, dtype=torch.bool, device=dev), torch.ones(1, P, dtype=torch.bool, device=dev),
                             (rank[:, None, :] < k[None, :, None]).reshape(NP * (P - 1), P)])                # [R, P]
        absent = present.logical_not().reshape(R, T, F)                                                       # player rho * F + f
        out = torch.empty(B * R, 2, device=dev)
        for g0 in range(0, B * R, B):
            idx = torch.arange(g0, g0 + B, device=dev)
            gene, gone = idx // R, absent[idx % R]
            pf, cf = {}, {}
            for bs, L in zip(BINS, NB):
                x = d["promoter_feats"][bs][gene].reshape(B, 1, L, F)
                pf[bs] = torch.where(gone[:, 0, None, None, :], torch.log1p(0.0 * torch.expm1(x)), x)
                x = d["pcre_feats"][bs][gene].reshape(B, S, L, F)
                cf[bs] = torch.where(gone[:, 1:, None, :], torch.log1p(0.0 * torch.expm1(x)), x)
            out[g0:g0 + B] = model(pf, {bs: d["promoter_pad_masks"][bs][gene] for bs in BINS}, cf, {bs: d["pcre_pad_masks"][bs][gene] for bs in BINS},
                                   {bs: d["interaction_masks"][bs][gene] for bs in BINS}, d["interaction_freq"][gene])
        v = out.reshape(B, R, 2)
        q = torch.arange(NP, device=dev)[:, None]

        def col(kk):      # the column of the first kk players of order q
            return torch.where(kk == 0, 0, torch.where(kk == P, 1, 2 + q * (P - 1) + kk - 1))

        dq = v[:, col(rank + 1)] - v[:, col(rank)]                                                            # [B, n_perm, P, 2]
        phi = dq.sum(1) / NP
        se = (((dq - phi[:, None]) ** 2).sum(1) / (NP * (NP - 1))).sqrt() if NP > 1 else torch.zeros_like(phi)
        return phi, se, v


if a.call_only:
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    sys.exit(0)

(phi_c, info), (phi_l, se_l, v_l) = call(), loop()
v_c = info["rows"]
same, worst = bool(torch.equal(v_c, v_l)), float((v_c - v_l).abs().max())
worst_phi, worst_se = float((phi_c - phi_l).abs().max()), float((info["stderr"] - se_l).abs().max())
if not worst < 1e-4:
    raise SystemExit("mark_sampled_bench: the row logits of the two legs disagree by %.3e; no time is reported" % worst)
legs = {"call": call, "loop": loop}
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
for k, v in times.items():
    v = sorted(v)
    res[k] = {"ms_median": round(v[len(v) // 2], 3), "ms_min": round(v[0], 3), "ms_max": round(v[-1], 3), "rounds": len(v)}
res["loop_over_call"] = round(res["loop"]["ms_median"] / res["call"]["ms_median"], 3)
res["call_minus_loop_ms"] = round(res["call"]["ms_median"] - res["loop"]["ms_median"], 3)
res["call_median_below_loop_min"] = bool(res["call"]["ms_median"] < res["loop"]["ms_min"])
row_bytes = sum(8 * (1 + S) * L * F + 2 * (1 + S) * L + 2 * T * T for L in NB) + 8 * T * T       # one chunk row, read + written
expand = {"bytes_per_chunk_of_64": 64 * row_bytes, "launches_per_call": B * R // B}
if a.kernel_stats:
    with open(a.kernel_stats) as f:
        hit = [r for r in csv.DictReader(f) if "k_mark_expand" in r["Name"]]
    if not hit:
        raise SystemExit("mark_sampled_bench: no k_mark_expand row in %s" % a.kernel_stats)
    us = float(hit[0]["AverageNs"]) / 1e3
    expand.update({"us_average": round(us, 2), "calls_in_profile": int(hit[0]["Calls"]), "TB/s": round(64 * row_bytes / us / 1e6, 3),
                   "frac_of_8TBs": round(64 * row_bytes / us / 1e6 / 8, 3), "source": "rocprofv3 --kernel-trace --stats, a run of its own"})
else:
    expand["TB/s"] = "not measured"
line = json.dumps({"workload": "B = 64, one player per (mark, region) pair (P = %d), n_perm = %d, s = 0: %d forwards" % (P, NP, B * R),
                   "row_logits_bit_equal": same, "row_logits_max_abs_diff": worst, "phi_max_abs_diff": worst_phi, "stderr_max_abs_diff": worst_se,
                   "stderr_max": float(info["stderr"].max()), "phi_abs_max": float(phi_c.abs().max()),
                   "timing": "HIP events around one call per leg, legs interleaved, two warm-up rounds", "call": res, "k_mark_expand": expand})
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(line + "\n")
