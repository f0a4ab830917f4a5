"""The six golden cases of the pCRE transplant screen (tests/golden/transplant.npz), chosen from the metadata of
tests.scan_oracle.scan_dataset, and what the golden script and the tests share around them: the metadata with a gene's partner list
edited, and a candidate binned by the dataset's own code in the form tests/transplant_oracle.py takes."""
import torch

from chromoformer_amd.data import bin_log1p, centred


def choose_cases(ds):
    """-> [(name, gene id, slot, (chrom, start, end) of the candidate, f, regression)]."""
    ids = list(ds.target_genes)
    part = {g: ds.genes[g]["pcres"] for g in ids}
    donor = next(g for g in ids[3:] if part[g])                                      # another gene's enhancer
    two = next(g for g in ids if len(part[g]) == 2)
    none = next(g for g in ids if not part[g])
    minus = next(g for g in ids if ds.genes[g]["tss"][2] == "-" and g != ids[1] and 1 <= len(part[g]) < ds.i_max)
    short = next(p for g in ids for p in part[g] if p[2] - p[1] == 1800)
    assert part[ids[1]] and donor != ids[1] and two != donor
    cand = tuple(part[donor][0])
    return [("replace", ids[1], 0, cand, 2.5, False),
            ("append2", two, 2, cand, 1.75, False),
            ("append0", none, 0, cand, 3.0, False),
            ("minus", minus, len(part[minus]), tuple(part[ids[1]][0]), 2.25, False),
            ("short", two, 1, tuple(short), 2.0, False),
            ("regressor", ids[1], 0, cand, 2.5, True)]


def edited_meta(table, gid, slot, cand, f):
    """The metadata table with partner `slot` of gene `gid` replaced by `cand` at score f, or appended if the gene has `slot` partners."""
    out = table.copy()
    out["neighbors"] = out["neighbors"].astype(object)
    out["scores"] = out["scores"].astype(object)
    i = out.index[out.gene_id == gid][0]
    has = isinstance(out.at[i, "neighbors"], str) and out.at[i, "neighbors"] != ""
    names = out.at[i, "neighbors"].split(";") if has else []
    scores = str(out.at[i, "scores"]).split(";") if has else []
    assert 0 <= slot <= len(names)
    name, score = "%s:%d-%d" % tuple(cand), repr(float(f))
    if slot == len(names):
        names.append(name)
        scores.append(score)
    else:
        names[slot], scores[slot] = name, score
    out.at[i, "neighbors"], out.at[i, "scores"] = ";".join(names), ";".join(scores)
    return out


def oracle_candidate(ds, cand):
    """The raw region `cand` binned as the dataset bins a partner -> (feats {binsize: [L, F]}, cols {binsize: [L] bool})."""
    raw = torch.as_tensor(ds._load(*cand)).to(torch.float32)
    feats, cols = {}, {}
    for b in ds.binsizes:
        L = ds.w_max // b
        x, lo, n = centred(bin_log1p(raw, b), L)
        c = torch.ones(L, dtype=torch.bool)
        c[lo:lo + n] = False
        feats[b], cols[b] = x.t().contiguous(), c
    return feats, cols
