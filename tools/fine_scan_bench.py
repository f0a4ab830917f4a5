"""The fine-resolution perturbation scan against the loop a user would write with public calls:
    python tools/fine_scan_bench.py [--out profiles/r19_fine_scan.json]

Shape: B = 64 genes (realistic regime; the promoter's coarser features re-binned from its finest so that the three resolutions hold
one signal), the promoter, the default eight mark sets, s = 0, a zoom of two coarse bins at width 1 from a per-gene start: 40 windows,
V = 321 variants per gene, 20,544 forwards.
  fine   one model.perturbation_scan_fine call (cf_perturbation_scan_fine: rows built by k_scan_fine_expand, 321 chunks of 64);
  loop   public calls only: the perturbed promoter rows of all variants built with torch on the device (the same rule, the partly
         covered 500-bp and 2-kb bins recomputed from the finest child in fp64), then model(...) under no_grad per 64 rows.
The two legs are interleaved in one process; HIP events around each; median of --rounds rounds with min and max, two warm-up rounds.
Both legs must give the same logits (within 1e-4; whether they are bit-equal is reported) before a time is reported.

The expand kernels' bytes per second need the kernels' own times: run the profile leg alone under the profiler and pass its statistics in,
    rocprofv3 --kernel-trace --stats -d OUT -o run --output-format csv -- python tools/fine_scan_bench.py --profile-only
    python tools/fine_scan_bench.py --kernel-stats OUT/<host>/run_kernel_stats.csv --out profiles/r19_fine_scan.json
(--profile-only: three fine scans and three coarse scans, so that k_scan_fine_expand and k_scan_expand come from one run).  Algorithmic
bytes of one launch over a chunk of n rows: those of tools/scan_bench.py -- every feature element, mask byte and frequency read and
written once; the <= 2 x 7 x 19 finest children a row re-reads are 0.1 % of that and are not counted."""
import argparse, csv, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from chromoformer_amd import ChromoformerClassifier
from oracle import chromoformer_oracle as orc

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=11)
ap.add_argument("--profile-only", action="store_true", help="three fine scans, three coarse scans and nothing else (for a profiler run)")
ap.add_argument("--kernel-stats", default=None, help="rocprofv3 --stats CSV of a --profile-only run: adds the expand kernels' times and bytes per second")
ap.add_argument("--out", default=None, help="also write the result line to this file")
a = ap.parse_args()
dev = torch.device("cuda", 0)
B, W, F, S, T = 64, 20, 7, 8, 9
BINS, NB = (2000, 500, 100), (20, 80, 400)
NW, SCALE = 40, 0.0
batch = orc.synthetic_batch(B, seed=77, regime="realistic")
for bs, m in batch["promoter_pad_masks"].items():          # every other promoter narrowed: its tail fifth is padding
    L = m.shape[-1]
    m[0::2, ..., L - max(1, L // 5):] = True
fine = batch["promoter_feats"][100].reshape(B, 400, F)
for bs, L in zip(BINS[:2], NB[:2]):                        # one signal at the three resolutions
    batch["promoter_feats"][bs] = torch.log1p(torch.expm1(fine.double()).reshape(B, L, 400 // L, F).mean(2)).float().reshape(B, 1, L, F)
model = ChromoformerClassifier(seed=42, max_batch=B).cuda(0)
KEYS = ("promoter_feats", "promoter_pad_masks", "pcre_feats", "pcre_pad_masks", "interaction_masks", "interaction_freq")
d = {k: ({b: t.to(dev) for b, t in v.items()} if isinstance(v, dict) else v.to(dev)) for k, v in batch.items() if k in KEYS}
for bs, L in zip(BINS, NB):                                # compact centre rows of the pad masks (what a resident store holds)
    d["promoter_pad_masks"][bs] = d["promoter_pad_masks"][bs].reshape(B, L, L)[:, L // 2].contiguous()
    d["pcre_pad_masks"][bs] = d["pcre_pad_masks"][bs].reshape(B, S, L, L)[:, :, L // 2].contiguous()
args = tuple(d[k] for k in KEYS)
SETS = [(f,) for f in range(F)] + [tuple(range(F))]
K = len(SETS)
V = 1 + K * NW
START = [20 * (b % 14) for b in range(B)]                  # each gene zooms into its own pair of coarse bins
marks = torch.zeros(K, F, dtype=torch.bool, device=dev)
for k, ms in enumerate(SETS):
    marks[k, list(ms)] = True


def scan_fine():
    return model.perturbation_scan_fine(*args, region=0, scale=SCALE, width=1, start=START, n_windows=NW)


def extent(mask, L):
    real = ~mask.bool()
    p = torch.arange(L, device=dev)
    q = torch.where(real, p, L).amin(1)
    return q, (torch.where(real, p, -1).amax(1) - q + 1).clamp(min=0)


def loop():
    """The same scan with public calls: all variants' promoter rows by torch, then model(...) per 64 rows."""
    with torch.no_grad():
        rows = {}
        qf, nf = extent(d["promoter_pad_masks"][100], 400)
        lo = torch.tensor(START, device=dev)[:, None] + torch.arange(NW, device=dev)[None, :]             # [B, NW], width 1
        live = lo < nf[:, None]
        xf = d["promoter_feats"][100].reshape(B, 400, F)
        uk = torch.gather(xf, 1, (qf[:, None] + lo).clamp(max=399)[:, :, None].expand(B, NW, F))          # the window's finest bin
        for bs, L in zip(BINS, NB):
            R = 400 // L
            q, n = extent(d["promoter_pad_masks"][bs], L)
            j = lo // R
            row = (q[:, None] + j).clamp(max=L - 1)
            x = d["promoter_feats"][bs].reshape(B, L, F)
            uj = torch.gather(x, 1, row[:, :, None].expand(B, NW, F))
            kids = (torch.minimum((j + 1) * R, nf[:, None]) - j * R).clamp(min=1)                         # children of bin j
            whole = torch.log1p(SCALE * torch.expm1(uj))
            part = torch.log1p((torch.expm1(uj).double() + ((SCALE - 1.0) * (100.0 * torch.expm1(uk).double())) / (kids * 100.0)[:, :, None]).float())
            new = torch.where((kids == 1)[:, :, None], whole, part)                                       # [B, NW, F]
            hit = (torch.arange(L, device=dev)[None, None, :] == row[:, :, None]) & (live & (j < n[:, None]))[:, :, None]      # [B, NW, L]
            full = hit[:, None, :, :, None] & marks[None, :, None, None, :]                               # [B, K, NW, L, F]
            pert = torch.where(full, new[:, None, :, None, :], x[:, None, None]).reshape(B, K * NW, L, F)
            rows[bs] = torch.cat([x.reshape(B, 1, L, F), pert], 1).reshape(B * V, 1, L, F)
        out = torch.empty(B * V, 2, device=dev)
        for g0 in range(0, B * V, B):
            gene = torch.arange(g0, min(g0 + B, B * V), device=dev) // V
            out[g0:g0 + gene.numel()] = model({bs: rows[bs][g0:g0 + B] for bs in BINS}, {bs: d["promoter_pad_masks"][bs][gene] for bs in BINS},
                                              {bs: d["pcre_feats"][bs][gene] for bs in BINS}, {bs: d["pcre_pad_masks"][bs][gene] for bs in BINS},
                                              {bs: d["interaction_masks"][bs][gene] for bs in BINS}, d["interaction_freq"][gene])
        return out.reshape(B, V, 2)


if a.profile_only:
    for _ in range(3):
        scan_fine()
        model.perturbation_scan(*args, region=0, scale=SCALE)
    torch.cuda.synchronize()
    sys.exit(0)

x, y = scan_fine(), loop()
same, worst = bool(torch.equal(x, y)), float((x - y).abs().max())
if not worst < 1e-4:
    raise SystemExit("fine_scan_bench: the two legs disagree by %.3e; no time is reported" % worst)
legs = {"fine": scan_fine, "loop": loop}
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
res["loop_over_fine"] = round(res["loop"]["ms_median"] / res["fine"]["ms_median"], 3)
row_bytes = sum(8 * (1 + S) * L * F + 2 * (1 + S) * L + 2 * T * T for L in NB) + 8 * T * T       # one chunk row, read + written
expand = {"bytes_per_chunk_of_64": 64 * row_bytes, "launches_per_call": -(-B * V // B)}
if a.kernel_stats:
    with open(a.kernel_stats) as f:
        table = list(csv.DictReader(f))
    for name in ("k_scan_fine_expand", "k_scan_expand"):
        hit = [r for r in table if name in r["Name"]]
        if not hit:
            raise SystemExit("fine_scan_bench: no %s row in %s" % (name, a.kernel_stats))
        us = float(hit[0]["AverageNs"]) / 1e3
        expand[name] = {"us_average": round(us, 2), "calls_in_profile": int(hit[0]["Calls"]), "TB/s": round(64 * row_bytes / us / 1e6, 3),
                        "frac_of_8TBs": round(64 * row_bytes / us / 1e6 / 8, 3)}
    expand["source"] = "rocprofv3 --kernel-trace --stats, a run of its own"
else:
    expand["k_scan_fine_expand"] = expand["k_scan_expand"] = "not measured"
line = json.dumps({"workload": "B = 64, promoter, 8 mark sets, s = 0, 40 windows of one finest bin from a per-gene start: %d forwards" % (B * V),
                   "legs_bit_equal": same, "legs_max_abs_diff": worst,
                   "timing": "HIP events around one call per leg, legs interleaved, two warm-up rounds", "call": res, "expand": expand})
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(line + "\n")
