"""Exact Shapley values of the histone marks against a donor cell type, against the loop a user would write without the call:
python tools/mark_donor_bench.py [--out profiles/r15_mark_donor.json]

Shape: B = 64 genes (realistic regime), a second draw of 64 as the donor's features, the seven marks as players in every region:
128 coalitions per gene, 8,192 forwards.
  call   one model.mark_donor_shapley call (cf_mark_donor_shapley: rows built by k_mark_donor_expand, 128 chunks of 64, then k_shapley);
  loop   public calls only: the rows of all coalitions built with torch.where on the device, model(...) under no_grad per 64 rows,
         then the Shapley sum with torch.
The two legs are interleaved in one process; HIP events around each; median of --rounds rounds with min and max, two warm-up rounds.
The coalition logits of the two legs must be bit-equal in the same run before a time is reported.

The bytes per second of k_mark_donor_expand and of its sibling k_mark_expand need the kernels' own times: run both call legs alone
under the profiler, in a run of its own, and pass its statistics in,
    rocprofv3 --kernel-trace --stats -d OUT -o run --output-format csv -- python tools/mark_donor_bench.py --call-only
    python tools/mark_donor_bench.py --kernel-stats <the run_kernel_stats.csv written under OUT> --out profiles/r15_mark_donor.json
Algorithmic bytes of one launch over a chunk of 64 rows: every feature element read from the source and written once (4 + 4 B); the
donor's element read (4 B) in the rows whose regions are touched -- with the seven marks as players every region of every word but
the full one, 127 of 128 rows, averaged over the call's launches; the compact pad-mask rows, interaction masks and frequencies read
and written once (1 + 1 B per byte, 4 + 4 B per frequency).  Against 8 TB/s."""
import argparse, csv, json, os, sys
from math import factorial
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from chromoformer_amd import ChromoformerClassifier
from oracle import chromoformer_oracle as orc

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=11)
ap.add_argument("--call-only", action="store_true", help="three mark_donor_shapley and three mark_shapley calls and nothing else (for a profiler run)")
ap.add_argument("--kernel-stats", default=None, help="rocprofv3 --stats CSV of a --call-only run: adds the two expand kernels' times and bytes per second")
ap.add_argument("--out", default=None, help="also write the result line to this file")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("mark_donor_bench: no GPU visible; nothing is measured without one")
dev = torch.device("cuda", 0)
B, F, S, T = 64, 7, 8, 9
P, N = F, 1 << F
BINS, NB = (2000, 500, 100), (20, 80, 400)
batch = orc.synthetic_batch(B, seed=77, regime="realistic")
other = orc.synthetic_batch(B, seed=78, regime="realistic")
model = ChromoformerClassifier(seed=42, max_batch=B).cuda(0)
KEYS = ("promoter_feats", "promoter_pad_masks", "pcre_feats", "pcre_pad_masks", "interaction_masks", "interaction_freq")
d = {k: ({b: t.to(dev) for b, t in v.items()} if isinstance(v, dict) else v.to(dev)) for k, v in batch.items() if k in KEYS}
donor = ({b: t.to(dev).contiguous() for b, t in other["promoter_feats"].items()}, {b: t.to(dev).contiguous() for b, t in other["pcre_feats"].items()})
# compact centre rows of the pad masks (what a resident store holds)
for bs, L in zip(BINS, NB):
    d["promoter_pad_masks"][bs] = d["promoter_pad_masks"][bs].reshape(B, L, L)[:, L // 2].contiguous()
    d["pcre_pad_masks"][bs] = d["pcre_pad_masks"][bs].reshape(B, S, L, L)[:, :, L // 2].contiguous()
args = tuple(d[k] for k in KEYS)
words = torch.arange(N, device=dev)
gone = (words[:, None] >> torch.arange(F, device=dev)[None, :] & 1) == 0                             # [N, F]: mark f absent from word m
size = gone.logical_not().sum(1)                                                                     # |m|
w = torch.tensor([factorial(k) * factorial(P - k - 1) / factorial(P) for k in range(P)], dtype=torch.float32, device=dev)


def call():
    return model.mark_donor_shapley(*args, donor=donor, return_coalitions=True)


def loop():
    """The same values with public calls: all coalitions' rows by torch.where, model(...) per 64 rows, the Shapley sum by torch."""
    with torch.no_grad():
        pf, cf = {}, {}
        for bs, L in zip(BINS, NB):
            x, y = d["promoter_feats"][bs].reshape(B, 1, L, F), donor[0][bs].reshape(B, 1, L, F)
            pf[bs] = torch.where(gone[None, :, None, :], y, x).reshape(B * N, 1, L, F)
            x, y = d["pcre_feats"][bs].reshape(B, 1, S, L, F), donor[1][bs].reshape(B, 1, S, L, F)
            cf[bs] = torch.where(gone[None, :, None, None, :], y, x).reshape(B * N, S, L, F)
        out = torch.empty(B * N, 2, device=dev)
        for g0 in range(0, B * N, B):
            gene = torch.arange(g0, g0 + B, device=dev) // N
            out[g0:g0 + B] = model({bs: pf[bs][g0:g0 + B] for bs in BINS}, {bs: d["promoter_pad_masks"][bs][gene] for bs in BINS},
                                   {bs: cf[bs][g0:g0 + B] for bs in BINS}, {bs: d["pcre_pad_masks"][bs][gene] for bs in BINS},
                                   {bs: d["interaction_masks"][bs][gene] for bs in BINS}, d["interaction_freq"][gene])
        v = out.reshape(B, N, 2)
        phi = torch.empty(B, P, 2, device=dev)
        for p in range(P):
            m = words[(words >> p & 1) == 0]
            phi[:, p] = ((v[:, m | (1 << p)] - v[:, m]) * w[size[m]][None, :, None]).sum(1)
        return phi, v


if a.call_only:
    for _ in range(3):
        call()
        model.mark_shapley(*args)
    torch.cuda.synchronize()
    sys.exit(0)

(phi_c, info), (phi_l, v_l) = call(), loop()
v_c = info["coalitions"]
same, worst = bool(torch.equal(v_c, v_l)), float((v_c - v_l).abs().max())
worst_phi = float((phi_c - phi_l).abs().max())
if not same:
    raise SystemExit("mark_donor_bench: the coalition logits of the two legs are not bit-equal (max difference %.3e); no time is reported" % worst)
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
res["spreads_overlap"] = bool(res["call"]["ms_max"] >= res["loop"]["ms_min"] and res["loop"]["ms_max"] >= res["call"]["ms_min"])
feat_row = sum(4 * (1 + S) * L * F for L in NB)                                                    # one row's feature bytes, once
rest_row = sum(2 * (1 + S) * L + 2 * T * T for L in NB) + 8 * T * T                                 # masks and frequencies, read + written
sib_bytes = 64 * (2 * feat_row + rest_row)                                                          # k_mark_expand, a chunk of 64 rows
don_bytes = sib_bytes + 64 * feat_row * (N - 1) // N                                                # + the donor, 127 of 128 rows
kernels = {"k_mark_donor_expand": {"bytes_per_chunk_of_64": don_bytes, "launches_per_call": N},
           "k_mark_expand": {"bytes_per_chunk_of_64": sib_bytes, "launches_per_call": N}}
if a.kernel_stats:
    with open(a.kernel_stats) as f:
        table = list(csv.DictReader(f))
    for name, k in kernels.items():
        hit = [r for r in table if name in r["Name"]]
        if not hit:
            raise SystemExit("mark_donor_bench: no %s row in %s" % (name, a.kernel_stats))
        us = float(hit[0]["AverageNs"]) / 1e3
        k.update({"us_average": round(us, 2), "calls_in_profile": int(hit[0]["Calls"]), "TB/s": round(k["bytes_per_chunk_of_64"] / us / 1e6, 3),
                  "frac_of_8TBs": round(k["bytes_per_chunk_of_64"] / us / 1e6 / 8, 3), "source": "rocprofv3 --kernel-trace --stats, a run of its own"})
else:
    for k in kernels.values():
        k["TB/s"] = "not measured"
line = json.dumps({"workload": "B = 64, a donor of 64, the seven marks as players: %d forwards" % (B * N), "coalition_logits_bit_equal": same,
                   "coalition_logits_max_abs_diff": worst, "phi_max_abs_diff": worst_phi,
                   "timing": "HIP events around one call per leg, legs interleaved, two warm-up rounds", "call": res, **kernels})
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(line + "\n")
