"""The pCRE transplant screen against the loop a user would write: python tools/transplant_bench.py [--out profiles/r28_transplant.json]

Shape: B = 64 genes (realistic regime), the default model, C = 64 candidates (U = 8 pseudo-genes per gene), Q = 4 contact
frequencies: 16,448 Regulation + head rows against 512 pseudo-genes through the trunk.  Every gene takes its first free slot, a gene
without one its last slot (replaced), so that every row is a real transplant.
  transplant      one transplant.pcre_transplant call;
  loop            the loop a user would write today: the six tensors edited with torch on the device and model(...) per 64 rows, 257
                  full forwards (the unedited batch, then one per candidate and frequency);
  pcre_shapley    model.pcre_shapley on the same batch, 16,384 Regulation + head rows from one trunk pass: the second yardstick, the
                  cost per Regulation + head row the call should approach.
The legs are interleaved in one process; HIP events around each; median of --rounds rounds with min and max, two warm-up rounds.
The rows of the call and of the loop are compared for bit-equality in the same run, before a time is reported.
The new kernels' bytes per second are not measured here."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from chromoformer_amd import ChromoformerClassifier
from chromoformer_amd import transplant as tp
from oracle import chromoformer_oracle as orc

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=11)
ap.add_argument("--out", default=None, help="also write the result line to this file")
a = ap.parse_args()
dev = torch.device("cuda", 0)
B, S, T, Cn, Q = 64, 8, 9, 64, 4
BINS, NB = (2000, 500, 100), (20, 80, 400)
batch = orc.synthetic_batch(B, seed=77, regime="realistic")
model = ChromoformerClassifier(seed=42, max_batch=B).cuda(0)
KEYS = ("promoter_feats", "promoter_pad_masks", "pcre_feats", "pcre_pad_masks", "interaction_masks", "interaction_freq")
d = {k: ({b: t.to(dev) for b, t in v.items()} if isinstance(v, dict) else v.to(dev)) for k, v in batch.items() if k in KEYS}
for bs, L in zip(BINS, NB):      # compact centre rows of the pad masks (what a resident store holds)
    d["promoter_pad_masks"][bs] = d["promoter_pad_masks"][bs].reshape(B, L, L)[:, L // 2].contiguous()
    d["pcre_pad_masks"][bs] = d["pcre_pad_masks"][bs].reshape(B, S, L, L)[:, :, L // 2].contiguous()
args = tuple(d[k] for k in KEYS)
src = orc.synthetic_batch(32, seed=78, regime="realistic")      # the candidates: the first 64 live pCREs of other genes
live = ~src["interaction_masks"][2000].reshape(32, T, T).diagonal(dim1=1, dim2=2).bool()
lib = tp.library_from_batch(src, [(g, s) for g in range(32) for s in range(S) if bool(live[g, s + 1])][:Cn])
assert len(lib) == Cn
lib = tp.Library({b: t.to(dev) for b, t in lib.feats.items()}, {b: t.to(dev) for b, t in lib.mask_rows.items()}, lib.names)
freqs = torch.tensor([1.0, 2.0, 5.0, 10.0])
dead = d["interaction_masks"][2000].reshape(B, T, T).diagonal(dim1=1, dim2=2).bool()
slots = [int(torch.nonzero(dead[b, 1:])[0]) if bool(dead[b, 1:].any()) else S - 1 for b in range(B)]
ar, sl = torch.arange(B, device=dev), torch.tensor(slots, device=dev)
J = sl + 1


def call():
    lg, info = tp.pcre_transplant(model, *args, library=lib, freq=freqs, slot=slots)
    return torch.cat([info["logits"][:, None], lg.reshape(B, Cn * Q, -1)], 1)


def loop():
    pf, pm, cf0, cm0, im0, fr0 = args
    im = {}
    for bs in BINS:      # the interaction masks do not depend on the candidate
        m = im0[bs].clone().reshape(B, T, T)
        dd = m.diagonal(dim1=1, dim2=2).clone()
        m[ar, J, :] = dd
        m[ar, :, J] = dd
        m[ar, J, J] = 0
        im[bs] = m.reshape(im0[bs].shape)
    with torch.no_grad():
        out = [model(*args)]
        for c in range(Cn):
            cf, cm = {}, {}
            for bs in BINS:
                cf[bs], cm[bs] = cf0[bs].clone(), cm0[bs].clone()
                cf[bs][ar, sl] = lib.feats[bs][c]
                cm[bs][ar, sl] = lib.mask_rows[bs][c].to(cm[bs].dtype)
            for q in range(Q):
                fr = fr0.clone()
                fr[ar, J, :] = 0
                fr[ar, :, J] = 0
                fr[ar, 0, J] = freqs[q]
                out.append(model(pf, pm, cf, cm, im, fr))
    return torch.stack(out, 1)


def shapley():
    return model.pcre_shapley(*args)[0]


x, y = call(), loop()
same = bool(torch.equal(x, y))
if not same:
    raise SystemExit("transplant_bench: the call and the loop differ by %.3e; no time is reported" % float((x - y).abs().max()))
moved = float((x[:, 1:] - x[:, :1]).abs().max())
print("transplant_bench: the call and the loop are bit-equal; timing %d rounds" % a.rounds, file=sys.stderr, flush=True)
del x, y
legs = {"transplant": call, "loop": loop, "pcre_shapley": shapley}
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
rows_t, rows_s = B * (1 + Cn * Q), B * (1 << S)
res["loop_over_transplant"] = round(res["loop"]["ms_median"] / res["transplant"]["ms_median"], 3)
res["transplant_over_pcre_shapley"] = round(res["transplant"]["ms_median"] / res["pcre_shapley"]["ms_median"], 3)
res["us_per_row"] = {"transplant": round(1e3 * res["transplant"]["ms_median"] / rows_t, 3), "pcre_shapley": round(1e3 * res["pcre_shapley"]["ms_median"] / rows_s, 3)}
call()
n_launches = model.launch_counts()[0]      # of the call just made
line = json.dumps({"workload": "B = 64, default model, C = 64 candidates, Q = 4 frequencies: %d Regulation + head rows, %d pseudo-genes" % (rows_t, B * Cn // S),
                   "legs_bit_equal": same, "largest_logit_change": moved,
                   "timing": "HIP events around one call (or one loop) per leg, legs interleaved, two warm-up rounds", "call": res,
                   "rows": {"transplant": rows_t, "pcre_shapley": rows_s}, "trunk_passes": {"transplant": 1 + Cn // S, "loop": 1 + Cn * Q},
                   "launch_counts_fwd_transplant": n_launches,
                   "k_transplant_pack / k_transplant_rows TB/s": "not measured"})
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(line + "\n")
