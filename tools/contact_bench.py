"""Exact Shapley values of the eight contacts against pcre_shapley and against the loop a user could write before:
python tools/contact_bench.py [--out profiles/r27_contact_games.json]

Shape: B = 64 genes (realistic regime), the default model (i_max = 8): 256 coalitions per gene, 16,384 Regulation + head rows.
  contact  one contact.contact_shapley(players="contacts") call (cf_contact_shapley: the trunk once, 256 chunks of 64 rows built by
           k_contact_expand, k_shapley);
  pcre     one model.pcre_shapley call: the same row count through k_coalition_expand -- the yardstick: the new call should cost what
           this one costs;
  loop     existing public calls only: per coalition word interaction_freq edited with torch on the device (rows and columns of the
           absent contacts scaled by 0), model(...) under no_grad on the 64 genes: 256 full forwards, each re-running the trunk.
The three legs alternate in one process; HIP events around each; median of --rounds rounds with min and max, two warm-up rounds.  The
table of the contact leg and the logits of the loop must be bit-equal before a time is reported.  Per ratio the line says whether it
lies outside both legs' min-max spread (the slower leg's fastest round above the faster leg's slowest)."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from chromoformer_amd import ChromoformerClassifier, contact
from oracle import chromoformer_oracle as orc

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=11)
ap.add_argument("--out", default=None, help="also write the result line to this file")
a = ap.parse_args()
dev = torch.device("cuda", 0)
B, S = 64, 8
N = 1 << S
batch = orc.synthetic_batch(B, seed=77, regime="realistic")
model = ChromoformerClassifier(seed=42, max_batch=B).cuda(0)
KEYS = ("promoter_feats", "promoter_pad_masks", "pcre_feats", "pcre_pad_masks", "interaction_masks", "interaction_freq")
d = {k: ({b: t.to(dev) for b, t in v.items()} if isinstance(v, dict) else v.to(dev)) for k, v in batch.items() if k in KEYS}
args = tuple(d[k] for k in KEYS)
zero = torch.zeros((), device=dev)


def contact_leg():
    return contact.contact_shapley(model, *args, players="contacts", scale=0.0, return_coalitions=True)


def pcre_leg():
    return model.pcre_shapley(*args, return_coalitions=True)


def loop_leg():
    """The same table with existing public calls: 256 model(...) calls on frequencies edited with torch."""
    with torch.no_grad():
        v = torch.empty(B, N, 2, device=dev)
        for m in range(N):
            gone = [j + 1 for j in range(S) if not m >> j & 1]
            f = d["interaction_freq"].clone()
            f[:, gone, :] = zero * d["interaction_freq"][:, gone, :]      # (from the gene's own entries both times: an entry named twice
            f[:, :, gone] = zero * d["interaction_freq"][:, :, gone]      # is edited once)
            v[:, m] = model(d["promoter_feats"], d["promoter_pad_masks"], d["pcre_feats"], d["pcre_pad_masks"], d["interaction_masks"], f)
        return v


px, ix = contact_leg()
n_launch = model.launch_counts()[0]
pp, ip = pcre_leg()
n_launch_pcre = model.launch_counts()[0]
vy = loop_leg()
same = bool(torch.equal(ix["coalitions"], vy))
worst = float((ix["coalitions"] - vy).abs().max())
if not same:
    raise SystemExit("contact_bench: the contact call's table and the loop's logits differ (max %.3e); no time is reported" % worst)
legs = {"contact": contact_leg, "pcre": pcre_leg, "loop": loop_leg}
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
for k, t in times.items():
    t = sorted(t)
    res[k] = {"ms_median": round(t[len(t) // 2], 3), "ms_min": round(t[0], 3), "ms_max": round(t[-1], 3), "rounds": len(t)}


def ratio(num, den):
    r = res[num]["ms_median"] / res[den]["ms_median"]
    slow, fast = (num, den) if r >= 1 else (den, num)
    return {"ratio": round(r, 3), "outside_both_spreads": bool(res[slow]["ms_min"] > res[fast]["ms_max"])}


res["contact_over_pcre"] = ratio("contact", "pcre")
res["loop_over_contact"] = ratio("loop", "contact")
line = json.dumps({"workload": "B = 64, default model, realistic regime: exact Shapley values of the 8 contacts (scale 0), %d Regulation + head rows" % (B * N),
                   "table_bit_equal_to_the_loop": same, "launches_per_contact_call": n_launch, "launches_per_pcre_call": n_launch_pcre,
                   "k_contact_expand_time_and_bytes_per_second": "not measured",
                   "timing": "HIP events around one call per leg, legs alternating, two warm-up rounds", "call": res})
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(line + "\n")
