"""The multi-region perturbation scan against the loop of single-region calls: python tools/scan_regions_bench.py [--out profiles/r13_scan_regions.json]

Shape: B = 64 genes (realistic regime), the default model, the default eight mark sets, s = 0: V = 161 variants per gene and region.
  regions_all     one model.perturbation_scan_regions call over all nine regions (the promoter through the whole forward per row, the
                  eight pCRE slots slot-packed: 20 trunk passes per slot instead of 161);
  loop_all        nine model.perturbation_scan calls, one per region (what the dataset generator and the CLI ran before);
  regions_pcres / loop_pcres   the same over the eight pCRE slots alone.
The legs are interleaved in one process; HIP events around each; median of --rounds rounds with min and max, two warm-up rounds.
The logits of the packed call and of the loop are compared for bit-equality in the same run, before a time is reported.
The new kernels' bytes per second are not measured here."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from chromoformer_amd import ChromoformerClassifier
from oracle import chromoformer_oracle as orc

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=11)
ap.add_argument("--out", default=None, help="also write the result line to this file")
a = ap.parse_args()
dev = torch.device("cuda", 0)
B, W, F, S = 64, 20, 7, 8
BINS, NB = (2000, 500, 100), (20, 80, 400)
batch = orc.synthetic_batch(B, seed=77, regime="realistic")
model = ChromoformerClassifier(seed=42, max_batch=B).cuda(0)
KEYS = ("promoter_feats", "promoter_pad_masks", "pcre_feats", "pcre_pad_masks", "interaction_masks", "interaction_freq")
d = {k: ({b: t.to(dev) for b, t in v.items()} if isinstance(v, dict) else v.to(dev)) for k, v in batch.items() if k in KEYS}
for bs, L in zip(BINS, NB):      # compact centre rows of the pad masks (what a resident store holds)
    d["promoter_pad_masks"][bs] = d["promoter_pad_masks"][bs].reshape(B, L, L)[:, L // 2].contiguous()
    d["pcre_pad_masks"][bs] = d["pcre_pad_masks"][bs].reshape(B, S, L, L)[:, :, L // 2].contiguous()
args = tuple(d[k] for k in KEYS)
flip = torch.arange(B, device=dev) % 2
V = 1 + (F + 1) * W
ALL, PCRES = list(range(S + 1)), list(range(1, S + 1))


def packed(regions):
    return model.perturbation_scan_regions(*args, regions=regions, scale=0.0, flip=flip)[0]


def loop(regions):
    return torch.stack([model.perturbation_scan(*args, region=r, scale=0.0, flip=flip if r == 0 else None) for r in regions])


x, y = packed(ALL), loop(ALL)
same = bool(torch.equal(x, y)) and bool(torch.equal(packed(PCRES), y[1:]))
if not same:
    raise SystemExit("scan_regions_bench: the packed call and the loop differ by %.3e; no time is reported" % float((x - y).abs().max()))
del x, y
legs = {"regions_all": lambda: packed(ALL), "loop_all": lambda: loop(ALL), "regions_pcres": lambda: packed(PCRES), "loop_pcres": lambda: loop(PCRES)}
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
res["loop_over_regions_all"] = round(res["loop_all"]["ms_median"] / res["regions_all"]["ms_median"], 3)
res["loop_over_regions_pcres"] = round(res["loop_pcres"]["ms_median"] / res["regions_pcres"]["ms_median"], 3)
U = -(-(V - 1) // S)
packed(ALL)
n_launches = model.launch_counts()[0]      # of the call just made
line = json.dumps({"workload": "B = 64, default model, 8 mark sets, s = 0: %d rows per region, 9 regions" % (B * V), "legs_bit_equal": same,
                   "timing": "HIP events around one call (or one loop) per leg, legs interleaved, two warm-up rounds", "call": res,
                   "trunk_passes_per_pcre_region": {"packed": -(-B * U // B), "loop": -(-B * V // B)},
                   "launch_counts_fwd_regions_all": n_launches,
                   "k_scan_pack / k_scan_unpack / k_scan_rows TB/s": "not measured"})
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(line + "\n")
