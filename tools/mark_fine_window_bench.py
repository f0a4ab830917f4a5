"""Permutation-sampled Shapley values of the 70 (mark, 200-bp window) players inside one coarse promoter window against the loop a user
would write with public calls:  python tools/mark_fine_window_bench.py [--out profiles/r20_mark_fine_window.json]

Shape: B = 64 genes (realistic regime), the default model, the promoter, players "cells" at width 2 inside coarse window 9 (start =
180, ten fine windows: P = 70), n_perm = 16, s = 0: R = 2 + 16 * 69 = 1,106 rows per gene, 70,784 forwards.
  call   one model.mark_fine_window_shapley_sampled call (cf_mark_fine_shapley_sampled: rows built by k_mark_fine_expand, 1,106 chunks
         of 64, then k_perm_shapley);
  loop   public calls only: per 64 rows the prefix coalitions' inputs built with torch on the device, as perturbation_scan_fine's
         return_feats describes them (the finest bins of the absent players' marks by the scan's rule; a coarser bin covered wholly
         likewise, one covered in part rebuilt from its finest children in fp64, ascending), model(...) under no_grad, then the
         estimator (mean and standard error over the orders) with torch.
The two legs are interleaved in one process; HIP events around each; median of --rounds rounds with min and max, two warm-up rounds.
The row logits of the two legs are compared in the same run (they must agree within 1e-4 before a time is reported; whether they are
bit-equal is recorded).

The per-chunk time of k_mark_fine_expand beside k_mark_window_expand's needs the kernels' own times: run the call legs of both games
alone under the profiler and pass the statistics in,
    rocprofv3 --kernel-trace --stats -d OUT -o run --output-format csv -- python tools/mark_fine_window_bench.py --call-only
    python tools/mark_fine_window_bench.py --kernel-stats OUT/<host>/run_kernel_stats.csv --out profiles/r20_mark_fine_window.json
(--call-only: two mark_fine_window_shapley_sampled calls, then two mark_window_shapley_sampled calls of the 70 "promoter_cells" players
at width 2, n_perm = 16).  Algorithmic bytes of one launch as in tools/mark_window_bench.py: every feature element read and written
once, the masks and frequencies likewise; the bytes-per-second figure stands beside the 8 TB/s of the device's memory."""
import argparse, csv, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from chromoformer_amd import ChromoformerClassifier
from chromoformer_amd.attribution import fine_window_players, shapley_permutations
from oracle import chromoformer_oracle as orc

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=11)
ap.add_argument("--perms", type=int, default=16)
ap.add_argument("--call-only", action="store_true", help="two calls of the fine game and two of the window game, nothing else (for a profiler run)")
ap.add_argument("--kernel-stats", default=None, help="rocprofv3 --stats CSV of a --call-only run: adds the two expand kernels' times")
ap.add_argument("--out", default=None, help="also write the result line to this file")
a = ap.parse_args()
dev = torch.device("cuda", 0)
B, F, S, T, WIDTH, START, NW = 64, 7, 8, 9, 2, 180, 10
P, NP = F * NW, a.perms
R = 2 + NP * (P - 1)
BINS, NB = (2000, 500, 100), (20, 80, 400)
LF, BF = NB[-1], BINS[-1]
batch = orc.synthetic_batch(B, seed=77, regime="realistic")
model = ChromoformerClassifier(seed=42, max_batch=B).cuda(0)
KEYS = ("promoter_feats", "promoter_pad_masks", "pcre_feats", "pcre_pad_masks", "interaction_masks", "interaction_freq")
d = {k: ({b: t.to(dev) for b, t in v.items()} if isinstance(v, dict) else v.to(dev)) for k, v in batch.items() if k in KEYS}
# compact centre rows of the pad masks (what a resident store holds)
for bs, L in zip(BINS, NB):
    d["promoter_pad_masks"][bs] = d["promoter_pad_masks"][bs].reshape(B, L, L)[:, L // 2].contiguous()
    d["pcre_pad_masks"][bs] = d["pcre_pad_masks"][bs].reshape(B, S, L, L)[:, :, L // 2].contiguous()
# the features of orc.synthetic_batch are drawn per resolution; a partly erased bin needs them binned from ONE signal (else 1 + m' <= 0):
# the promoter is made 400 real finest bins and its coarser features the means of their children
for bs, L in zip(BINS, NB):
    d["promoter_pad_masks"][bs] = torch.zeros_like(d["promoter_pad_masks"][bs])
    if bs != BF:
        m = torch.expm1(d["promoter_feats"][BF].reshape(B, L, LF // L, F).double()).mean(2)
        d["promoter_feats"][bs] = torch.log1p(m).float().reshape(B, 1, L, F).contiguous()
args = tuple(d[k] for k in KEYS)
assert len(fine_window_players("cells", F, WIDTH, NW)[0]) == P
perms = shapley_permutations(P, NP, 0)


def call():
    return model.mark_fine_window_shapley_sampled(*args, players="cells", width=WIDTH, n_windows=NW, start=START, permutations=perms, return_rows=True)


def loop():
    """The same values with public calls: the prefix rows by torch, model(...) per 64 rows, mean and standard error by torch."""
    with torch.no_grad():
        pi = torch.from_numpy(perms.astype("int64")).to(dev)
        rank = torch.empty_like(pi).scatter_(1, pi, torch.arange(P, device=dev).expand(NP, P))      # rank[q, p]: the position of player p
        k = torch.arange(1, P, device=dev)
        present = torch.cat([torch.zeros(1, P, dtype=torch.bool, device=dev), torch.ones(1, P, dtype=torch.bool, device=dev),
                             (rank[:, None, :] < k[None, :, None]).reshape(NP * (P - 1), P)])                # [R, P]
        absent = present.logical_not().reshape(R, NW, F).repeat_interleave(WIDTH, 1)                          # [R, NW * WIDTH, F]: player g * F + f
        table = torch.cat([absent, torch.zeros(R, 1, F, dtype=torch.bool, device=dev)], 1)                    # ... and "no window"
        none = NW * WIDTH
        ext = {}
        for bs, L in zip(BINS, NB):
            real = d["promoter_pad_masks"][bs].logical_not()
            q, e = real.int().argmax(1), L - real.flip(1).int().argmax(1)
            ext[bs] = (q, torch.where(real.any(1), e - q, 0))
        qf, nf = ext[BF]
        kk = torch.arange(LF, device=dev)[None].expand(B, LF)                                                 # genomic finest bin k
        win = torch.where((kk >= START) & (kk < START + none) & (kk < nf[:, None]), kk - START, none)        # [B, LF]: its slot in `table`
        uf = d["promoter_feats"][BF].reshape(B, LF, F)
        mf = torch.expm1(torch.gather(uf, 1, (qf[:, None] + kk).clamp(max=LF - 1)[..., None].expand(B, LF, F))).double()   # by genomic k
        out = torch.empty(B * R, 2, device=dev)
        for g0 in range(0, B * R, B):
            idx = torch.arange(g0, g0 + B, device=dev)
            gene, row = idx // R, idx % R
            gone_k = table[row[:, None], win[gene]]                                                           # [64, LF, F] by genomic k
            pf = {}
            for bs, L in zip(BINS, NB):
                Rr = LF // L
                x = d["promoter_feats"][bs][gene].reshape(B, L, F)
                q, n = ext[bs][0][gene], ext[bs][1][gene]
                j = torch.arange(L, device=dev)[None] - q[:, None]                                            # genomic bin of each row
                ok = (j >= 0) & (j < n[:, None])
                jc = j.clamp(0, L - 1)
                S_ = torch.zeros(B, L, F, dtype=torch.float64, device=dev)
                some = torch.zeros(B, L, F, dtype=torch.bool, device=dev)
                every = torch.ones(B, L, F, dtype=torch.bool, device=dev)
                cnt = torch.zeros(B, L, 1, dtype=torch.float64, device=dev)
                for c in range(Rr):                                                                           # ascending genomic children
                    kc = jc * Rr + c
                    live = (ok & (kc < nf[gene][:, None]))[..., None]
                    kci = kc.clamp(max=LF - 1)[..., None].expand(B, L, F)
                    gk = torch.gather(gone_k, 1, kci) & live
                    S_ = S_ + torch.where(gk, float(BF) * torch.gather(mf[gene], 1, kci), 0.0)
                    some |= gk
                    every &= gk | ~live
                    cnt = cnt + live * float(BF)
                every &= some
                whole = torch.log1p(0.0 * torch.expm1(x))
                part = torch.log1p((torch.expm1(x).double() + (0.0 - 1.0) * S_ / cnt.clamp(min=1.0)).float())
                pf[bs] = torch.where(every, whole, torch.where(some, part, x)).reshape(B, 1, L, F)
            out[g0:g0 + B] = model(pf, {bs: d["promoter_pad_masks"][bs][gene] for bs in BINS}, {bs: d["pcre_feats"][bs][gene] for bs in BINS},
                                   {bs: d["pcre_pad_masks"][bs][gene] for bs in BINS}, {bs: d["interaction_masks"][bs][gene] for bs in BINS},
                                   d["interaction_freq"][gene])
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
    for _ in range(2):
        model.mark_window_shapley_sampled(*args, players="promoter_cells", width=2, permutations=perms)
    torch.cuda.synchronize()
    sys.exit(0)

(phi_c, info), (phi_l, se_l, v_l) = call(), loop()
v_c = info["rows"]
same, worst = bool(torch.equal(v_c, v_l)), float((v_c - v_l).abs().max())
worst_phi, worst_se = float((phi_c - phi_l).abs().max()), float((info["stderr"] - se_l).abs().max())
if not worst < 1e-4:
    raise SystemExit("mark_fine_window_bench: the row logits of the two legs disagree by %.3e; no time is reported" % worst)
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
res["call_median_not_above_loop_median"] = bool(res["call"]["ms_median"] <= res["loop"]["ms_median"])
res["call_median_within_loop_min_max"] = bool(res["call"]["ms_median"] <= res["loop"]["ms_max"])
row_bytes = sum(8 * (1 + S) * L * F + 2 * (1 + S) * L + 2 * T * T for L in NB) + 8 * T * T       # one chunk row, read + written
expand = {"bytes_per_chunk_of_64": 64 * row_bytes, "launches_per_call": B * R // B}
if a.kernel_stats:
    with open(a.kernel_stats) as f:
        rows = list(csv.DictReader(f))
    for name in ("k_mark_fine_expand", "k_mark_window_expand"):
        hit = [r for r in rows if name in r["Name"]]
        if not hit:
            expand[name] = "not measured"
            continue
        us = float(hit[0]["AverageNs"]) / 1e3
        expand[name] = {"us_average": round(us, 2), "calls_in_profile": int(hit[0]["Calls"]), "TB/s": round(64 * row_bytes / us / 1e6, 3),
                        "fraction_of_8_TB/s": round(64 * row_bytes / us / 1e6 / 8.0, 3)}
    expand["source"] = "rocprofv3 --kernel-trace --stats, one run of its own for both kernels (chunks of 64 rows, n_perm = %d)" % NP
else:
    expand["k_mark_fine_expand"] = expand["k_mark_window_expand"] = "not measured"
line = json.dumps({"workload": "B = 64, promoter, one player per (mark, window of 2 finest bins) inside coarse window 9 (P = %d), n_perm = %d, s = 0: "
                               "%d forwards" % (P, NP, B * R),
                   "row_logits_bit_equal": same, "row_logits_max_abs_diff": worst, "phi_max_abs_diff": worst_phi, "stderr_max_abs_diff": worst_se,
                   "stderr_max": float(info["stderr"].max()), "phi_abs_max": float(phi_c.abs().max()),
                   "timing": "HIP events around one call per leg, legs interleaved, two warm-up rounds", "call": res, "expand_kernels": expand})
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(line + "\n")
