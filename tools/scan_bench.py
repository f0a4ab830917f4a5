"""The in-silico perturbation scan against the loop a user would write today: python tools/scan_bench.py [--out profiles/r11_scan.json]

Shape: B = 64 genes (realistic regime), the promoter, the default eight mark sets, s = 0: V = 161 variants per gene, 10,304 forwards.
  scan   one model.perturbation_scan call (cf_perturbation_scan: rows built by k_scan_expand, 161 chunks of 64);
  loop   existing public calls only: the perturbed promoter rows of all variants built with torch on the device (the same rule, the
         covered rows from the pad masks), then model(...) under no_grad per 64 rows.
The two legs are interleaved in one process; HIP events around each; median of --rounds rounds with min and max, two warm-up rounds.
Both legs must give the same logits (within 1e-4; whether they are bit-equal is reported) before a time is reported.

k_scan_expand's bytes per second need the kernel's own time: run the scan leg alone under the profiler and pass its statistics in,
    rocprofv3 --kernel-trace --stats -d OUT -o run --output-format csv -- python tools/scan_bench.py --scan-only
    python tools/scan_bench.py --kernel-stats OUT/<host>/run_kernel_stats.csv --out profiles/r11_scan.json
Algorithmic bytes of one launch over a chunk of n rows: every feature element read and written once (4 + 4 B), feats_out not
requested; the compact pad-mask rows, interaction masks and frequencies likewise (1 + 1 B per byte, 4 + 4 B per frequency)."""
import argparse, csv, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from chromoformer_amd import ChromoformerClassifier
from oracle import chromoformer_oracle as orc

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=11)
ap.add_argument("--scan-only", action="store_true", help="three scan calls and nothing else (for a profiler run)")
ap.add_argument("--kernel-stats", default=None, help="rocprofv3 --stats CSV of a --scan-only run: adds k_scan_expand's time and bytes per second")
ap.add_argument("--out", default=None, help="also write the result line to this file")
a = ap.parse_args()
dev = torch.device("cuda", 0)
B, W, F, S, T = 64, 20, 7, 8, 9
BINS, NB = (2000, 500, 100), (20, 80, 400)
batch = orc.synthetic_batch(B, seed=77, regime="realistic")
for bs, m in batch["promoter_pad_masks"].items():          # every other promoter narrowed: its tail fifth is padding
    L = m.shape[-1]
    m[0::2, ..., L - max(1, L // 5):] = True
model = ChromoformerClassifier(seed=42, max_batch=B).cuda(0)
KEYS = ("promoter_feats", "promoter_pad_masks", "pcre_feats", "pcre_pad_masks", "interaction_masks", "interaction_freq")
d = {k: ({b: t.to(dev) for b, t in v.items()} if isinstance(v, dict) else v.to(dev)) for k, v in batch.items() if k in KEYS}
# compact centre rows of the pad masks (what a resident store holds)
for bs, L in zip(BINS, NB):
    d["promoter_pad_masks"][bs] = d["promoter_pad_masks"][bs].reshape(B, L, L)[:, L // 2].contiguous()
    d["pcre_pad_masks"][bs] = d["pcre_pad_masks"][bs].reshape(B, S, L, L)[:, :, L // 2].contiguous()
args = tuple(d[k] for k in KEYS)
SETS = [(f,) for f in range(F)] + [tuple(range(F))]
K = len(SETS)
V = 1 + K * W
marks = torch.zeros(K, F, dtype=torch.bool, device=dev)
for k, ms in enumerate(SETS):
    marks[k, list(ms)] = True


def scan():
    return model.perturbation_scan(*args, region=0, scale=0.0)


def loop():
    """The same scan with existing public calls: all variants' promoter rows by torch, then model(...) per 64 rows."""
    with torch.no_grad():
        rows = {}
        real = ~d["promoter_pad_masks"][2000].bool()
        pos = torch.arange(W, device=dev)
        n_c = (torch.where(real, pos, -1).amax(1) - torch.where(real, pos, W).amin(1) + 1).clamp(min=0)          # [B]
        for bs, L in zip(BINS, NB):
            R = L // W
            real = ~d["promoter_pad_masks"][bs].bool()
            p = torch.arange(L, device=dev)
            q = torch.where(real, p, L).amin(1)
            n = (torch.where(real, p, -1).amax(1) - q + 1).clamp(min=0)
            j = p[None, :] - q[:, None]                                                          # genomic bin of row p   [B, L]
            g = pos[None, :, None]                                                               #                        [1, W, 1]
            hi = torch.minimum(torch.minimum(g + 1, n_c[:, None, None]) * R, n[:, None, None])
            cover = (j[:, None, :] >= g * R) & (j[:, None, :] < hi) & (g < n_c[:, None, None])   # [B, W, L]
            x = d["promoter_feats"][bs].reshape(B, 1, 1, L, F)
            full = cover[:, None, :, :, None] & marks[None, :, None, None, :]                    # [B, K, W, L, F]
            pert = torch.where(full, torch.log1p(0.0 * torch.expm1(x)), x).reshape(B, K * W, L, F)
            rows[bs] = torch.cat([x.reshape(B, 1, L, F), pert], 1).reshape(B * V, 1, L, F)
        out = torch.empty(B * V, 2, device=dev)
        for g0 in range(0, B * V, B):
            gene = torch.arange(g0, min(g0 + B, B * V), device=dev) // V
            out[g0:g0 + gene.numel()] = model({bs: rows[bs][g0:g0 + B] for bs in BINS}, {bs: d["promoter_pad_masks"][bs][gene] for bs in BINS},
                                              {bs: d["pcre_feats"][bs][gene] for bs in BINS}, {bs: d["pcre_pad_masks"][bs][gene] for bs in BINS},
                                              {bs: d["interaction_masks"][bs][gene] for bs in BINS}, d["interaction_freq"][gene])
        return out.reshape(B, V, 2)


if a.scan_only:
    for _ in range(3):
        scan()
    torch.cuda.synchronize()
    sys.exit(0)

x, y = scan(), loop()
same, worst = bool(torch.equal(x, y)), float((x - y).abs().max())
if not worst < 1e-4:
    raise SystemExit("scan_bench: the two legs disagree by %.3e; no time is reported" % worst)
legs = {"scan": scan, "loop": loop}
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
res["loop_over_scan"] = round(res["loop"]["ms_median"] / res["scan"]["ms_median"], 3)
row_bytes = sum(8 * (1 + S) * L * F + 2 * (1 + S) * L + 2 * T * T for L in NB) + 8 * T * T       # one chunk row, read + written
expand = {"bytes_per_chunk_of_64": 64 * row_bytes, "launches_per_call": -(-B * V // B)}
if a.kernel_stats:
    with open(a.kernel_stats) as f:
        hit = [r for r in csv.DictReader(f) if "k_scan_expand" in r["Name"]]
    if not hit:
        raise SystemExit("scan_bench: no k_scan_expand row in %s" % a.kernel_stats)
    us = float(hit[0]["AverageNs"]) / 1e3
    expand.update({"us_average": round(us, 2), "calls_in_profile": int(hit[0]["Calls"]), "TB/s": round(64 * row_bytes / us / 1e6, 3),
                   "frac_of_8TBs": round(64 * row_bytes / us / 1e6 / 8, 3), "source": "rocprofv3 --kernel-trace --stats, a run of its own"})
else:
    expand["TB/s"] = "not measured"
line = json.dumps({"workload": "B = 64, promoter, 8 mark sets, s = 0: %d forwards" % (B * V), "legs_bit_equal": same, "legs_max_abs_diff": worst,
                   "timing": "HIP events around one call per leg, legs interleaved, two warm-up rounds", "call": res, "k_scan_expand": expand})
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(line + "\n")
