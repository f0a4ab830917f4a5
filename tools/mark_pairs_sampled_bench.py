"""Sampled Shapley interaction indices of four focal (mark, region) players against the loop a user can write with the public calls of
the parent: python tools/mark_pairs_sampled_bench.py [--out profiles/r24_mark_pairs_sampled.json]

Shape: B = 8 genes (realistic regime), the default model, players "cells" (P = 63), n_perm = 16, four focal players, s = 0.
  call   one model.mark_shapley_interactions_sampled call (cf_mark_shapley_interactions_sampled: the shared row layout through
         k_mark_expand, k_perm_pairs, k_perm_shapley);
  loop   model.mark_coalitions_wide on the same coalition words, then the estimator with torch on the device (gathers through the same
         column table, mean and standard error over the orders).
The two legs are interleaved in one process; HIP events around each; median of --rounds rounds with min and max, two warm-up rounds.
The row logits of the two legs must be bit-equal in the same run before a time is reported.  `forwards` records the rows per call beside
the layout that shares nothing with the Shapley estimate's table (2 + 2 n_focal + n_focal n_perm (2 (P - 1) - 2) rows per gene).

--sibling: model.mark_shapley_sampled alone at tools/mark_sampled_bench.py's shape (B = 64, n_perm = 16): run it in this tree and in a
checkout of the parent in one visit to see what the row stride of k_perm_shapley costs.
--call-only: two calls and nothing else, for `rocprofv3 --kernel-trace --stats -- python tools/mark_pairs_sampled_bench.py --call-only`
(k_perm_pairs's own time)."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from chromoformer_amd import ChromoformerClassifier
from chromoformer_amd.attribution import shapley_permutations
from oracle import chromoformer_oracle as orc

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=11)
ap.add_argument("--perms", type=int, default=16)
ap.add_argument("--sibling", action="store_true", help="time mark_shapley_sampled alone at B = 64 (parent against branch)")
ap.add_argument("--call-only", action="store_true", help="two interactions calls and nothing else (for a profiler run)")
ap.add_argument("--out", default=None, help="also write the result line to this file")
a = ap.parse_args()
dev = torch.device("cuda", 0)
F, S, T = 7, 8, 9
P, NP = F * T, a.perms
B = 64 if a.sibling else 8
FOCAL = [0, 10, 31, 62]
BINS, NB = (2000, 500, 100), (20, 80, 400)
batch = orc.synthetic_batch(B, seed=77, regime="realistic")
model = ChromoformerClassifier(seed=42, max_batch=64).cuda(0)
KEYS = ("promoter_feats", "promoter_pad_masks", "pcre_feats", "pcre_pad_masks", "interaction_masks", "interaction_freq")
d = {k: ({b: t.to(dev) for b, t in v.items()} if isinstance(v, dict) else v.to(dev)) for k, v in batch.items() if k in KEYS}
for bs, L in zip(BINS, NB):      # compact centre rows of the pad masks (what a resident store holds)
    d["promoter_pad_masks"][bs] = d["promoter_pad_masks"][bs].reshape(B, L, L)[:, L // 2].contiguous()
    d["pcre_pad_masks"][bs] = d["pcre_pad_masks"][bs].reshape(B, S, L, L)[:, :, L // 2].contiguous()
args = tuple(d[k] for k in KEYS)
perms = shapley_permutations(P, NP, 0)


def timed(legs, rounds):
    times = {k: [] for k in legs}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rnd in range(2 + rounds):                      # two warm-up rounds
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
    return res


def emit(line):
    line = json.dumps(line)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if a.sibling:
    res = timed({"mark_shapley_sampled": lambda: model.mark_shapley_sampled(*args, players="cells", permutations=perms)}, a.rounds)
    emit({"workload": "B = 64, P = %d, n_perm = %d: mark_shapley_sampled alone, %d forwards" % (P, NP, B * (2 + NP * (P - 1))), **res})
    sys.exit(0)

from chromoformer_amd.attribution import focal_words      # (the parent has none: below the sibling leg)
words, col = focal_words(perms, FOCAL)
R = len(words)


def call():
    return model.mark_shapley_interactions_sampled(*args, players="cells", focal=FOCAL, permutations=perms, return_rows=True)


def loop():
    """The same values with the parent's public calls: the rows by mark_coalitions_wide, the estimator with torch."""
    v = model.mark_coalitions_wide(*args, keep=words, players="cells")                       # [B, R, 2]
    c = torch.as_tensor(col.astype(np.int64), device=dev)                                    # [F, n_perm, P, 2]
    m = v[:, c[..., 1]] - v[:, c[..., 0]]                                                    # [B, F, n_perm, P, 2]: i's marginal on T_k
    dk = m[:, :, :, 1:] - m[:, :, :, :-1]                                                    # at a = 0 .. P - 2
    pi = torch.from_numpy(perms.astype(np.int64)).to(dev)
    rank = torch.empty_like(pi).scatter_(1, pi, torch.arange(P, device=dev).expand(NP, P))   # [n_perm, P]
    out = torch.empty(B, len(FOCAL), P, 2, device=dev)
    se = torch.empty_like(out)
    for f, i in enumerate(FOCAL):
        r = rank[:, i]
        pos = rank - (rank > r[:, None]).long()                                              # a of player j in order q (i itself: r)
        s = torch.gather(dk[:, f], 2, pos.clamp(max=P - 2)[None, :, :, None].expand(B, NP, P, 2))
        s[:, torch.arange(NP, device=dev), i] = m[:, f, torch.arange(NP, device=dev), r]     # the diagonal: i's own marginal
        out[:, f] = s.sum(1) / NP
        se[:, f] = (((s - out[:, f, None]) ** 2).sum(1) / (NP * (NP - 1))).sqrt()
    return out, se, v


if a.call_only:
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    sys.exit(0)

(inter_c, info), (inter_l, se_l, v_l) = call(), loop()
same = bool(torch.equal(info["rows"], v_l))
if not same:
    raise SystemExit("mark_pairs_sampled_bench: the row logits of the two legs differ by %.3e; no time is reported"
                     % float((info["rows"] - v_l).abs().max()))
res = timed({"call": call, "loop": loop}, a.rounds)
res["loop_over_call"] = round(res["loop"]["ms_median"] / res["call"]["ms_median"], 3)
unshared = 2 + 2 * len(FOCAL) + len(FOCAL) * NP * (2 * (P - 1) - 2)
emit({"workload": "B = %d, one player per (mark, region) pair (P = %d), n_perm = %d, focal %s, s = 0" % (B, P, NP, FOCAL),
      "row_logits_bit_equal": same, "inter_max_abs_diff": float((inter_c - inter_l).abs().max()),
      "stderr_max_abs_diff": float((info["stderr"] - se_l).abs().max()), "inter_abs_max": float(inter_c.abs().max()),
      "stderr_max": float(info["stderr"].max()),
      "forwards": {"rows_per_gene": R, "per_call": B * R, "shapley_estimate_alone": 2 + NP * (P - 1), "unshared_layout_rows_per_gene": unshared},
      "timing": "HIP events around one call per leg, legs interleaved, two warm-up rounds", "call": res,
      "k_perm_pairs": "not measured"})
