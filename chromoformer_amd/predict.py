"""`python -m chromoformer_amd.predict` -- the inference entrypoint (reference: demo/run_demo.py and
demo/run_demo_regression.py, same -m / -d / -o / -w options plus --regression instead of a second script).

    prediction column = sigmoid(logits)[:, 1]   (classifier, demo/run_demo.py:116)
                      = logits[:, 0]            (regressor,  demo/run_demo_regression.py:117)

Forward only (`cf_forward(..., save_for_backward=0)`) on batches staged from a GeneStore.  Checkpoints in the
reference's `.pt` layout load directly; checkpoints written before the reference renamed its modules
(`embed2000_a`, `transformer500`, `lin_proj_c`, ... -- the mapping of misc/convert_weight.py:19-88) are renamed
on the fly.

Every further output file and every option that tunes one is declared once, in TABLE: the parser, the defaults, the value checks,
the "option without its output" refusals, predict()'s keyword arguments and the calls of the writers (predict_writers.py) are read
from it.  A new output is one Out row and one writer."""
from __future__ import annotations

import argparse
import inspect
import re
from collections import namedtuple

import numpy as np
import pandas as pd
import torch

from . import attribution as A
from . import predict_writers as W
from .engine import Trainer
from .net import ChromoformerClassifier, ChromoformerRegressor
from .util import seed_everything

_LEGACY = [  # (pattern, replacement), applied in order; first match of the second group wins (convert_weight.py)
    (r"transformer(2000|500|100)", r"regulation.\1.transformer"),
    (r"embed(2000|500|100)_a", r"embed.\1"),
    (r"embed(2000|500|100)_b", r"pairwise_interaction.\1"),
    (r"^embed(?=\d)", "embed."),
    (r"^pw_int", "pairwise_interaction."),
    (r"^reg(?=\d)", "regulation."),
]


def modernise_keys(state):
    """Legacy checkpoint keys -> current `state_dict` keys (no-op for current checkpoints)."""
    out = {}
    for k, v in state.items():
        k = k.replace("lin_proj_c.", "lin_proj_pcre.") if "lin_proj_c." in k else k
        for pat, rep in _LEGACY:
            k2 = re.sub(pat, rep, k, count=1)
            if k2 != k:
                k = k2
                break
        out[k] = v
    return out


# the table's rows
# Arg: an argument of main() itself, an input path or a switch.  flags: its spellings, the long one last.
Arg = namedtuple("Arg", "flags help required switch", defaults=(False, False))
# Opt: an option that tunes outputs.  default: what predict() takes when it is not given (a tuple: comma-separated on the command line);
# type / choices: the parser's; rule: its value rule (_RULES); plain: a path or a switch -- given when set, with nothing to fill in.
Opt = namedtuple("Opt", "dest help default type choices rule plain switch", defaults=(None, None, None, None, False, False))
# Out: an output.  writer(run, **fixed, <arg> = the path, **{name: the option's value}) serves it; rows with the same writer and the
# same `fixed` share one call.  options: {option dest: the writer's name for it} -- the options that apply to THIS output.  donor: it
# reads the donor cell type; raw: it reads the raw .npy files.  needs: what must be given with it (_needs adds the donor's directory).
# precheck(options, geometry): refusals before anything is computed, given the outputs and options of every row that names the
# precheck, by the writer's names, raising in predict()'s words; main() runs it at predict()'s default geometry and puts `prefix`
# in front of the error (or of its `cli` words, predict_writers.Refusal).
Out = namedtuple("Out", "dest help writer arg fixed options donor raw needs precheck prefix", defaults=("path", {}, {}, False, False, (), None, ""))


def _flag(dest):
    return "--" + dest.replace("_", "-")


def _must(ok, o, what):
    if not ok:
        raise ValueError("%s must be %s" % (_flag(o.dest), what))


def _slot(o, v, args):      # the option's default word ("promoter" / "append") or a pCRE slot, which becomes an int
    _must(v == o.default or v.isdigit() and int(v) < _GEOMETRY["i_max"], o, "%s or a pCRE slot in [0, %d)" % (o.default, _GEOMETRY["i_max"]))
    return v if v == o.default else int(v)


def _frequencies(o, v, args):      # numbers separated by commas, which become a list of floats
    try:
        freqs = [float(s) for s in v.split(",")]
    except ValueError:
        freqs = [np.nan]
    _must(np.isfinite(freqs).all(), o, "a comma-separated list of finite frequencies")
    return freqs


def _focal(o, v, args):      # a number K, which becomes an int, or player names separated by commas, which become a list
    if not isinstance(v, str):
        return v
    if not v.strip().lstrip("+-").isdigit():
        return [s.strip() for s in v.split(",")]
    _must(int(v) >= 1, o, "at least 1 player (or a list of player names)")
    return int(v)


def _checked(ok, what):
    """A value rule that converts nothing: ok(value, args) or main() refuses with "<flag> must be <what(args)>"."""
    def rule(o, v, args):
        _must(ok(v, args), o, what(o, args))
        return v
    return rule


_n_out = lambda args: 1 if args.regression else 2      # noqa: E731
_least = lambda args: 2 if args.ig_method == "riemann_trapezoid" else 1      # noqa: E731
_RULES = dict(      # the value rules of the options' command-line values, rule(option row, value, args) -> value, in the order main() applies them
    column=_checked(lambda v, a: v is None or 0 <= v < _n_out(a), lambda o, a: "in [0, %d)" % _n_out(a)),
    steps=_checked(lambda v, a: v >= _least(a), lambda o, a: "at least %d" % _least(a)),
    factor=_checked(lambda v, a: v >= 0 and np.isfinite(v), lambda o, a: "a finite factor >= 0"),
    finite=_checked(lambda v, a: np.isfinite(v), lambda o, a: "a finite %s" % ("factor" if o.dest.endswith("scale") else "number")),
    at_least_1=_checked(lambda v, a: v is None or v >= 1, lambda o, a: "at least 1"),
    slot=_slot, frequencies=_frequencies, focal=_focal)


def _check_contact(o, g):
    names = A.contact_players(o["players"], g["i_max"])[2]
    if o["interactions_out"] and len(names) < 2:
        raise W.Refusal("predict: contact_interactions_out needs at least 2 players; contact_players = %r has 1" % (o["players"],),
                        "--contact-interactions-out needs at least 2 players; --contact-players %s has 1" % (o["players"],))
    if not np.isfinite(o["scale"]):
        raise ValueError("predict: contact_scale = %r: a finite factor" % (o["scale"],))
    if o["marks"] not in ("own", "donor"):
        raise ValueError("predict: contact_donor_marks = %r: 'own' or 'donor'" % (o["marks"],))


def _check_backselect(o, g):
    A.mark_players_wide(o["players"], g["n_feats"], g["i_max"])
    if o["mode"] not in ("backward", "forward") or not np.isfinite(o["frac"]):
        raise ValueError("predict: backselect_mode = %r ('backward' / 'forward'), backselect_frac = %r (finite)" % (o["mode"], o["frac"]))


def _check_focal(o, g):
    W.focal_argument(o["focal"], o["players"], g["n_feats"], g["i_max"])


def _check_window(o, g):      # (too many players for the geometry)
    A.window_players(o["players"], g["n_feats"], g["i_max"], g["w_max"] // max(g["binsizes"]), o["width"])


def _check_fine_window(o, g):
    A.fine_window_players(o["players"], g["n_feats"], o["width"], -(-(max(g["binsizes"]) // min(g["binsizes"])) // max(int(o["width"]), 1)))


def _check_transplant(o, g):
    from .transplant import broadcast_freq, read_bed, slot_argument
    read_bed(o["bed"])
    broadcast_freq(W.transplant_freqs(o["freqs"]), 1, 1, "predict")
    if not isinstance(o["slot"], (str, int, np.integer)):
        raise ValueError("predict: transplant_slot = %r: 'append' or a slot" % (o["slot"],))
    slot_argument(o["slot"], 1, g["i_max"], "predict")


_IG = dict(ig_steps="n_steps", ig_method="method", ig_target="target")
_SAMPLED = dict(mark_sampled_players="players", mark_perms="n_perm", mark_seed="seed")
_PAIRS = dict(_SAMPLED, mark_focal="focal", interaction_index="index")
_BACKSELECT = dict(mark_backselect_players="players", backselect_mode="mode", backselect_frac="frac")
_WINDOW = dict(window_players="players", window_width="width", window_perms="n_perm", window_seed="seed")
_FINE_WINDOW = dict(fine_window_region="region", fine_window_width="width", fine_window_players="players", fine_window_zoom="zoom",
                    fine_window_perms="n_perm", fine_window_seed="seed")
_EXACT = dict(writer=W.write_exact_values, fixed=dict(game="pcre"))
_EXACT_MARK = dict(writer=W.write_exact_values, fixed=dict(game="mark"))
_EXACT_DONOR = dict(writer=W.write_exact_values, fixed=dict(game="mark_donor"), donor=True)
_DONOR_RULE = dict(fixed=dict(donor=True), donor=True)      # (the same writer against the donor cell type)
_CONTACT = dict(writer=W.write_contact_values, precheck=_check_contact)
_PAIRS_CALL = dict(writer=W.write_mark_sampled_interactions, precheck=_check_focal, prefix="--mark-focal: ")
_WINDOW_CALL = dict(writer=W.write_mark_window_values, precheck=_check_window)
_FINE_WINDOW_CALL = dict(writer=W.write_mark_fine_window_values, precheck=_check_fine_window)
_MARK = dict(mark_players="players", mark_scale="scale")
_CONTACT_OPTS = dict(contact_players="players", contact_scale="scale")

TABLE = [      # in the order of --help
    Arg(("-m", "--meta"), "Path to input metadata file.", required=True),
    Arg(("-d", "--npy-dir"), "Path to directory containing histone signals in .npy files.", required=True),
    Arg(("-o", "--output"), "Path to output expression prediction.", required=True),
    Arg(("-w", "--weights"), "Path to pretrained Chromoformer weights in .pt format."),
    Arg(("--regression",), "ChromoformerRegressor (run_demo_regression.py)", switch=True),
    Arg(("--store",), "packed store of `python -m chromoformer_amd.pack` (default: <npy-dir>/chromoformer.cfstore if present)"),
    Out("attention_dir", "also write DIR/{embed,pairwise_interaction,regulation}_{binsize}.npy: the "
        "attention maps of every gene, in metadata order (model.attention_maps)", W.write_attention_maps, "attention_dir"),
    Out("embeddings_out", "also write the regulatory embedding of every gene (the fc_head input, "
        "[n_genes, 3 * d_emb]) to this .npy file, in metadata order", W.write_attention_maps, "embeddings_out"),
    Out("pcre_ablation_out", "also write in-silico pCRE deletion to this .npy file: [n_genes, i_max + 2] "
        "predictions in metadata order, column 0 as --output, column 1 + j with pCRE j deleted, the last with the promoter "
        "alone (model.pcre_ablation)", W.write_pcre_ablation),
    Out("pcre_shapley_out", "also write the exact Shapley values of the pCREs to this .npz file, in metadata "
        "order and in LOGIT space of the prediction's column (efficiency holds there, not after the sigmoid): phi [n_genes, i_max] "
        "(0 for dummy slots), logits, promoter_only (phi sums to their difference) and n_pcres (model.pcre_shapley)", arg="shapley_out", **_EXACT),
    Out("pcre_epistasis_out", "also write the pair-deletion epistasis of the pCREs to this .npy file: "
        "[n_genes, i_max, i_max] in logit space, symmetric, the leave-one-out effects on the diagonal (model.pcre_epistasis)", arg="epistasis_out", **_EXACT),
    Out("pcre_interactions_out", "also write the pairwise Shapley interaction index of the pCREs to this .npy "
        "file: [n_genes, i_max, i_max] in logit space, symmetric, how much one pCRE's marginal contribution changes with the other "
        "present, averaged over every coalition of the rest (negative: redundant, positive: cooperating); the diagonal as "
        "--interaction-index says (model.pcre_shapley_interactions)", arg="interactions_out", options=dict(interaction_index="index"), **_EXACT),
    Opt("interaction_index", "the index of --pcre-interactions-out / "
        "--mark-interactions-out / --mark-donor-interactions-out: sii, the Shapley interaction index, the Shapley values on the "
        "diagonal (default), or sti, Shapley-Taylor of order 2, v({i}) - v(nobody) on the diagonal (diagonal and upper triangle then "
        "sum to the prediction's logit minus every player absent)", "sii", choices=A.INTERACTION_INDICES),
    Out("ig_dir", "also write integrated gradients (zero baseline, every float input) of every gene, in "
        "metadata order, as DIR/promoter_feats_{binsize}.npy [n, L, F], DIR/pcre_feats_{binsize}.npy [n, i_max, L, F], "
        "DIR/interaction_freq.npy [n, T, T] and DIR/delta.npy [n] (model.integrated_gradients).  About 126 KB per gene at the "
        "default configuration: 2.4 GB for 18,955 genes", W.write_integrated_gradients, "ig_dir", options=_IG),
    Opt("ig_steps", "quadrature nodes of --ig-dir (default 50)", 50, int, rule="steps"),
    Opt("ig_method", "quadrature of --ig-dir (default gausslegendre)", "gausslegendre", choices=A.METHODS),
    Opt("ig_target", "logit column of --ig-dir (default 1 for the classifier, 0 with --regression)", None, int, rule="column"),
    Out("raw_ig_dir", "also write integrated gradients in raw-signal space (zero-signal baseline, path a * x): "
        "DIR/<gene_id>.npz with the keys of --raw-saliency-dir, the tracks holding the per-sample attributions, plus "
        "baseline_logits and delta (model.raw_integrated_gradients).  Takes --ig-steps, --ig-method and --ig-target; needs the "
        "raw .npy files, also next to a packed store", W.write_raw_integrated_gradients, "ig_dir", options=_IG, raw=True),
    Out("raw_saliency_dir", "also write raw-signal saliency: DIR/<gene_id>.npz with the gradient of the "
        "prediction's logit with respect to the raw .npy signals (promoter [7, window], pcre_<s> [7, len], genomic orientation, "
        "regions, logits; model.raw_signal_gradients).  Needs the raw .npy files, also next to a packed store", W.write_raw_saliency,
        "saliency_dir", options=dict(raw_saliency_target="target", raw_saliency_times_input="times_input"), raw=True),
    Opt("raw_saliency_target", "logit column of --raw-saliency-dir (default 1 for the classifier, 0 with --regression)", None, int, rule="column"),
    Opt("raw_saliency_times_input", "--raw-saliency-dir writes gradient x input", False, plain=True, switch=True),
    Out("scan_out", "also write the in-silico perturbation scan to this .npz file: gene_ids, mark_sets "
        "[n_sets, 7], prediction [n] (as --output) and promoter [n, n_sets, W]: the prediction with each mark alone, then all "
        "marks, scaled by --scan-scale in raw-signal space over each window of the promoter, genomic order, NaN where a window "
        "holds no real bin (model.perturbation_scan)", W.write_perturbation_scan, options=dict(scan_scale="scale", scan_width="width", scan_regions="regions")),
    Opt("scan_scale", "scale factor of --scan-out: 0 erases the marks (default), 2 doubles them", 0.0, float, rule="factor"),
    Opt("scan_width", "window width of --scan-out in coarsest bins (default 1)", 1, int, rule="at_least_1"),
    Opt("scan_regions", "--scan-out scans the promoter (default) or also every pCRE slot: pcres [n, i_max, n_sets, W]", "promoter", choices=("promoter", "all")),
    Out("fine_scan_out", "also write the FINE-resolution perturbation scan to this .npz file: gene_ids, "
        "mark_sets [n_sets, 7], prediction [n] (as --output), chroms [n], windows [n, n_win, 2] (genomic start and end, -1 padding) and "
        "scan [n, n_sets, n_win]: the prediction with each mark alone, then all marks, scaled by --fine-scan-scale in raw-signal space "
        "over windows of --fine-scan-width finest bins (100 bp), NaN padding (model.perturbation_scan_fine)", W.write_perturbation_scan_fine,
        options=dict(fine_scan_region="region", fine_scan_width="width", fine_scan_stride="stride", fine_scan_zoom="zoom", fine_scan_scale="scale")),
    Opt("fine_scan_region", "the region --fine-scan-out scans: promoter (default) or a pCRE slot 0 .. 7", "promoter", rule="slot"),
    Opt("fine_scan_width", "window width of --fine-scan-out in finest bins (default 1)", 1, int, rule="at_least_1"),
    Opt("fine_scan_stride", "distance between windows of --fine-scan-out in finest bins (default: the width)", None, int, rule="at_least_1"),
    Opt("fine_scan_zoom", "--fine-scan-out first runs the coarse scan and fine-scans, per gene, the K coarse windows that move the prediction's logit "
        "most; also writes zoom [n, K], coarse_windows and coarse (default: the whole region)", None, int, rule="at_least_1"),
    Opt("fine_scan_scale", "scale factor of --fine-scan-out: 0 erases the marks (default), 2 doubles them", 0.0, float, rule="factor"),
    Out("mark_shapley_out", "also write the exact Shapley values of the histone marks to this .npz file, in "
        "metadata order and in LOGIT space of the prediction's column: gene_ids, players (names), phi [n_genes, P], logits and "
        "erased (every player absent; phi sums to their difference) (model.mark_shapley)", arg="shapley_out", options=_MARK, **_EXACT_MARK),
    Out("mark_epistasis_out", "also write the pair epistasis of the histone marks to this .npy file: [n_genes, P, P] in logit space, "
        "symmetric, the leave-one-out effects on the diagonal (model.mark_epistasis)", arg="epistasis_out", options=_MARK, **_EXACT_MARK),
    Out("mark_interactions_out", "also write the pairwise Shapley interaction index of the histone marks to "
        "this .npy file: [n_genes, P, P] in logit space, symmetric (model.mark_shapley_interactions).  --mark-players, --mark-scale "
        "and --interaction-index apply", arg="interactions_out", options=dict(_MARK, interaction_index="index"), **_EXACT_MARK),
    Opt("mark_players", "the players of --mark-shapley-out / --mark-epistasis-out: "
        "each mark in every region (marks, the default), each mark in the promoter and in the pCREs (compartments), or all marks "
        "per region (regions)", "marks", choices=A.MARK_PLAYER_SPECS),
    Opt("mark_scale", "what an absent mark's raw signal is scaled by: 0 erases it (default)", 0.0, float, rule="factor"),
    Out("raw_donor_ig_dir", "also write integrated gradients in raw-signal space against the DONOR cell type of "
        "--donor-npy-dir (path xd + a * (x - xd) between the two raw signals): DIR/<gene_id>.npz with the keys of --raw-ig-dir plus "
        "donor_prediction; baseline_logits is the donor's signal under the gene's masks and frequencies "
        "(model.raw_integrated_gradients(donor_dataset=...)).  Takes --ig-steps, --ig-method and --ig-target; needs the raw .npy "
        "files of both cell types", W.write_raw_integrated_gradients, "ig_dir", options=_IG, raw=True, **_DONOR_RULE),
    Arg(("--donor-npy-dir",), "directory of the .npy histone signals of a DONOR cell type over the same regions: "
        "what an absent mark becomes in --mark-donor-shapley-out / --mark-donor-epistasis-out"),
    Arg(("--donor-meta",), "metadata file of the donor cell type (default: --meta); TSS, strand and pCREs of every gene must equal those of --meta"),
    Arg(("--donor-store",), "packed store of the donor cell type (default: <donor-npy-dir>/chromoformer.cfstore if present)"),
    Out("mark_donor_shapley_out", "also write the exact Shapley values of the histone marks against the donor "
        "cell type to this .npz file, in metadata order and in LOGIT space of the prediction's column: gene_ids, players (names), "
        "phi [n_genes, P], logits, donor (every player's marks from the donor, the gene's masks and frequencies; phi sums to logits "
        "- donor) and donor_prediction (the donor's own prediction) (model.mark_donor_shapley).  --mark-players applies", arg="shapley_out",
        options=dict(mark_players="players"), **_EXACT_DONOR),
    Out("mark_donor_epistasis_out", "also write the pair epistasis of the histone marks against the donor cell "
        "type to this .npy file: [n_genes, P, P] in logit space, symmetric, the leave-one-out effects on the diagonal "
        "(model.mark_donor_epistasis).  --mark-players applies", arg="epistasis_out", options=dict(mark_players="players"), **_EXACT_DONOR),
    Out("mark_donor_interactions_out", "also write the pairwise Shapley interaction index of the histone marks "
        "against the donor cell type to this .npy file: [n_genes, P, P] in logit space, symmetric "
        "(model.mark_donor_shapley_interactions).  --mark-players and --interaction-index apply", arg="interactions_out",
        options=dict(mark_players="players", interaction_index="index"), **_EXACT_DONOR),
    Out("mark_sampled_shapley_out", "also write permutation-SAMPLED Shapley values of up to 128 histone-mark "
        "players to this .npz file, in metadata order and in LOGIT space of the prediction's column: gene_ids, players (names), "
        "permutations [n_perm, P], phi [n_genes, P], stderr [n_genes, P] (the standard error over the sampled orders: the sampling "
        "error is reported, not bounded), logits and absent (every player absent; phi sums to their difference) "
        "(model.mark_shapley_sampled).  --mark-scale applies", W.write_mark_sampled_values, options=dict(_SAMPLED, mark_scale="scale")),
    Out("mark_donor_sampled_shapley_out", "the same against the donor cell type of --donor-npy-dir: an absent "
        "player takes the donor's signal", W.write_mark_sampled_values, options=_SAMPLED, **_DONOR_RULE),
    Opt("mark_sampled_players", "the players of --mark-sampled-shapley-out / "
        "--mark-donor-sampled-shapley-out: one per (mark, region) pair (cells, the default: 63 players, phi reshapes to "
        "[n_genes, i_max + 1, 7]), or the specs of --mark-players", "cells", choices=A.MARK_WIDE_PLAYER_SPECS),
    Opt("mark_perms", "sampled orders of adding the players (default 64); each costs P - 1 forwards per gene", 64, int, rule="at_least_1"),
    Opt("mark_seed", "seed of the sampled orders (default 0)", 0, int),
    Out("mark_backselect_out", "also write the greedy player selection of up to 128 histone-mark players to "
        "this .npz file, in metadata order, on the prediction's logit column: gene_ids, players (names), mode, frac, order "
        "[n_genes, P] (the player of each move), curve [n_genes, P + 1] (the logit after t moves: the deletion curve), size and "
        "subset [n_genes, P] (the smallest sufficient set on the path: which few cells are enough on their own), threshold, "
        "direction, logits and absent (chromoformer_amd.backselect.mark_backselect; deterministic, P (P + 1) / 2 + 1 forwards per gene).  "
        "--mark-scale applies", W.write_mark_backselect, options=dict(_BACKSELECT, mark_scale="scale"), precheck=_check_backselect),
    Out("mark_donor_backselect_out", "the same against the donor cell type of --donor-npy-dir: an absent "
        "player takes the donor's signal", W.write_mark_backselect, options=_BACKSELECT, precheck=_check_backselect, **_DONOR_RULE),
    Opt("mark_backselect_players", "the players of --mark-backselect-out / "
        "--mark-donor-backselect-out: one per (mark, region) pair (cells, the default), or the specs of --mark-players", "cells", choices=A.MARK_WIDE_PLAYER_SPECS),
    Opt("backselect_mode", "backward (default): start from every player and "
        "remove the least needed one per round; forward: start from none and add the most useful one", "backward", choices=("backward", "forward")),
    Opt("backselect_frac", "a set is sufficient when it keeps this share of logits - absent (default 0.9)", 0.9, float, rule="finite"),
    Out("mark_sampled_interactions_out", "also write the SAMPLED pairwise Shapley interaction index of each gene's "
        "focal mark players with every player to this .npz file, in metadata order and in LOGIT space of the prediction's column: "
        "gene_ids, players (names), index, permutations, focal [n_genes, n_focal], interactions and stderr [n_genes, n_focal, P] (the "
        "standard error over the sampled orders: the sampling error is reported, not bounded), phi and phi_stderr [n_genes, P], "
        "logits and absent (model.mark_shapley_interactions_sampled).  --mark-focal, --mark-sampled-players, --mark-perms, "
        "--mark-seed, --mark-scale and --interaction-index apply", options=dict(_PAIRS, mark_scale="scale"), **_PAIRS_CALL),
    Out("mark_donor_sampled_interactions_out", "the same against the donor cell type of --donor-npy-dir: an "
        "absent player takes the donor's signal", options=_PAIRS, **_PAIRS_CALL, **_DONOR_RULE),
    Opt("mark_focal", "the focal players of --mark-sampled-interactions-out / "
        "--mark-donor-sampled-interactions-out: a number K (default 4): each gene's K strongest players by |phi| of a sampled Shapley "
        "estimate on the same orders; or player names separated by commas (mark3@pcre0,mark0@promoter): those for every gene", 4, rule="focal"),
    Out("pcre_dividends_out", "also write the Harsanyi dividends (the Moebius transform of the coalition "
        "table) of every set of pCRE slots to this .npz file, in metadata order and in LOGIT space of the prediction's column: "
        "gene_ids, players (names), sets [2^P] (set names by word), dividends [n_genes, 2^P] (they add up to the logit of every "
        "coalition: which pCREs act alone, which together, in which combinations) and mass (the scale of a dividend's rounding "
        "error) (model.pcre_dividends)", W.write_dividends, fixed=dict(game="pcre")),
    Out("mark_dividends_out", "the same for the histone marks (model.mark_dividends).  --mark-players and "
        "--mark-scale apply", W.write_dividends, fixed=dict(game="mark"), options=_MARK),
    Out("mark_donor_dividends_out", "the same against the donor cell type of --donor-npy-dir: an absent mark "
        "takes the donor's signal (model.mark_donor_dividends).  --mark-players applies", W.write_dividends, fixed=dict(game="mark_donor"),
        options=dict(mark_players="players"), donor=True),
    Out("contact_shapley_out", "also write the exact Shapley values of CONTACT players -- the promoter-pCRE "
        "contact frequencies of the pCRE slots, and / or the slots themselves -- to this .npz file, in metadata order and in LOGIT "
        "space of the prediction's column: gene_ids, players (names), phi [n_genes, P] (0 for dummy slots), logits, erased (every "
        "player absent; phi sums to their difference), freq [n_genes, i_max] and n_pcres (contact.contact_shapley): does a pCRE matter "
        "through its chromatin state or through its contact with the promoter?", arg="shapley_out", options=_CONTACT_OPTS, **_CONTACT),
    Opt("contact_players", "the players of the --contact-* outputs: each slot's "
        "contact (contacts, the default), each slot deleted (pcres: the pCRE game), both, slot by slot (pcres_and_contacts: 16 "
        "players) or one player holding every contact (all: the model without Hi-C)", "contacts", choices=A.CONTACT_PLAYER_SPECS),
    Opt("contact_scale", "what an absent contact's frequency is scaled by: 0 erases it (default), 2 doubles it; any finite value", 0.0, float, rule="finite"),
    Out("contact_interactions_out", "also write the pairwise Shapley interaction index of the contact players "
        "to this .npy file: [n_genes, P, P] in logit space, symmetric (contact.contact_shapley_interactions).  --contact-players, "
        "--contact-scale and --interaction-index apply", arg="interactions_out", options=dict(_CONTACT_OPTS, interaction_index="index"), **_CONTACT),
    Out("contact_dividends_out", "also write the Harsanyi dividends of every set of contact players to this "
        ".npz file: gene_ids, players, sets [2^P], dividends and mass [n_genes, 2^P] (contact.contact_dividends).  --contact-players "
        "and --contact-scale apply", arg="dividends_out", options=_CONTACT_OPTS, **_CONTACT),
    Out("contact_donor_shapley_out", "the Shapley values of the contact players against the donor cell type of "
        "--donor-npy-dir: an absent contact takes the donor's frequency.  The keys of --contact-shapley-out with donor in place of "
        "erased, plus donor_freq and marks.  --contact-players applies", arg="shapley_out",
        options=dict(contact_players="players", contact_donor_marks="marks"), **_CONTACT, **_DONOR_RULE),
    Opt("contact_donor_marks", "--contact-donor-shapley-out plays on the gene's own "
        "features (own, the default) or on the donor's under the gene's masks (donor: logits is then the donor row of "
        "--mark-donor-shapley-out, and the two games together account for the whole difference between the two cell types)", "own",
        choices=("own", "donor")),
    Out("window_shapley_out", "also write the Shapley values of WINDOW players -- stretches of a region, in coarsest bins -- to this .npz file, "
        "in metadata order and in LOGIT space of the prediction's column: gene_ids, players (names), estimator (exact with at most 16 players, "
        "else sampled), phi [n_genes, P], stderr, logits, absent (every player absent; phi sums to their difference), null (the window holds "
        "no real bin of the gene), chroms and windows [n_genes, P, 2] (genomic start and end) and, sampled, permutations "
        "(model.mark_window_shapley / mark_window_shapley_sampled)", options=dict(_WINDOW, window_scale="scale"), **_WINDOW_CALL),
    Out("window_donor_shapley_out", "the same against the donor cell type of --donor-npy-dir: an absent "
        "player's window takes the donor's signal", options=_WINDOW, **_WINDOW_CALL, **_DONOR_RULE),
    Opt("window_players", "the players of --window-shapley-out / "
        "--window-donor-shapley-out: all marks per promoter window (promoter, the default), each mark per promoter window "
        "(promoter_cells) or all marks per window of every region (regions); at most 128: widen the windows", "promoter", choices=A.WINDOW_PLAYER_SPECS),
    Opt("window_width", "window width in coarsest bins (default 1)", 1, int, rule="at_least_1"),
    Opt("window_perms", "sampled orders when there are more than 16 players (default 64)", 64, int, rule="at_least_1"),
    Opt("window_seed", "seed of the sampled orders (default 0)", 0, int),
    Opt("window_scale", "what an absent player's raw signal is scaled by inside its window: 0 "
        "erases it (default); --window-shapley-out only", 0.0, float, rule="factor"),
    Out("fine_window_shapley_out", "also write the Shapley values of FINE window players -- stretches of "
        "finest bins inside each gene's most important coarse windows (the coarse window game runs first) -- to this .npz file, in "
        "metadata order and in LOGIT space of the prediction's column: gene_ids, players (names), exact, zoom [n_genes, k] (the "
        "chosen coarse windows), coarse_phi, phi and stderr [n_genes, k, P], logits, absent [n_genes, k], null, chroms and "
        "windows [n_genes, k, P, 2] (genomic start and end) (model.mark_fine_window_shapley_dataset)",
        options=dict(_FINE_WINDOW, fine_window_scale="scale"), **_FINE_WINDOW_CALL),
    Out("fine_window_donor_shapley_out", "the same against the donor cell type of --donor-npy-dir: an absent "
        "player's window takes the donor's signal, in the coarse and in the fine game", options=_FINE_WINDOW, **_FINE_WINDOW_CALL, **_DONOR_RULE),
    Opt("fine_window_region", "the region the game plays in: promoter (default) or a pCRE slot 0..7", "promoter", rule="slot"),
    Opt("fine_window_width", "window width in finest bins (default 2)", 2, int, rule="at_least_1"),
    Opt("fine_window_players", "all marks per fine window (windows, the "
        "default) or each mark per fine window (cells); at most 128: widen the windows", "windows", choices=A.FINE_WINDOW_PLAYER_SPECS),
    Opt("fine_window_zoom", "coarse windows to zoom into per gene (default 1)", 1, int, rule="at_least_1"),
    Opt("fine_window_perms", "sampled orders when a game has more than 16 players (default 64)", 64, int, rule="at_least_1"),
    Opt("fine_window_seed", "seed of the sampled orders (default 0)", 0, int),
    Opt("fine_window_scale", "what an absent player's raw signal is scaled by inside its window: 0 "
        "erases it (default); --fine-window-shapley-out only", 0.0, float, rule="factor"),
    Opt("transplant_bed", "pCRE transplant screen: a BED file of candidate regions, `chrom start end [name]` "
        "lines, whose raw chrom:start-end.npy files are in --npy-dir; each is tried in one pCRE slot of every gene "
        "(transplant.pcre_transplant).  Needs --transplant-out", plain=True),
    Out("transplant_out", "write the transplant screen to this .npz file, in metadata order: prediction "
        "[n_genes], transplant [n_genes, C, Q] (the prediction with candidate c in the gene's slot at contact frequency q), slot "
        "(-1: not placed), placed, candidates, freqs.  Needs --transplant-bed", W.write_transplant, "out",
        options=dict(transplant_bed="bed", transplant_freq="freqs", transplant_slot="slot"), needs=("transplant_bed",),
        precheck=_check_transplant, prefix="--transplant-bed: "),
    Opt("transplant_freq", "the contact frequencies of the screen, comma-separated (default 1,5,10)", (1.0, 5.0, 10.0), rule="frequencies"),
    Opt("transplant_slot", "append (default: each gene's first free slot; a gene without one is not "
        "placed) or a slot in [0, 8), whose pCRE is replaced", "append", rule="slot"),
]
OPTS = [r for r in TABLE if isinstance(r, Opt)]
OUTS = [r for r in TABLE if isinstance(r, Out)]
_N_FEATS = 7      # the histone marks of the model and of every dataset here
KEYWORDS = {r.dest: r.default if isinstance(r, Opt) else None for r in TABLE if not isinstance(r, Arg)}      # predict()'s keyword arguments
_DEFAULTS = {o.dest: ",".join("%g" % x for x in o.default) if isinstance(o.default, tuple) else o.default for o in OPTS if not o.plain}      # what main() fills in
# for an option that was not given, as the command line spells it; main() tells "not given" by None until its checks are through


def _needs(out):
    return out.needs or (("donor_npy_dir",) if out.donor else ())


def _prechecks(values):
    """(precheck, its options, the first row that names it) of the requested outputs, in table order, each precheck once.  Its options:
    every output and option of the rows that share it, by the writer's names."""
    found = {}
    for out in OUTS:
        if out.precheck is not None and values[out.dest]:
            found.setdefault(out.precheck, out)
    for check, first in found.items():
        options = {}
        for out in OUTS:
            if out.precheck is check:
                options.update({out.arg: values[out.dest]}, **{name: values[dest] for dest, name in out.options.items()})
        yield check, options, first


def predict(meta_path, npy_dir, weights=None, regression=False, bsz=32, seed=123, i_max=8, w_prom=40000, w_max=40000,
            binsizes=(2000, 500, 100), progress=False, store_path=None, *, donor_npy_dir=None, donor_meta=None, donor_store_path=None, **given):
    """-> (meta DataFrame, predictions float32 [n_genes]) in the order of the metadata file.  **given: the outputs to write as well
    and the options that tune them, by the names and with the defaults of KEYWORDS -- every Out and Opt row of TABLE, whose help texts
    (`--help`) say what each writes and which options apply to it; an unknown name is a TypeError.  A donor output reads the donor cell
    type's signals from donor_npy_dir with the metadata donor_meta (default: meta_path) or the packed store donor_store_path -- both
    cell types must hold the genes' regions at the same coordinates (attribution.same_regions); a raw output needs the raw .npy files
    also when a packed store serves the predictions.  Everything is refused before anything is computed."""
    for name in given:
        if name not in KEYWORDS:
            raise TypeError("predict() got an unexpected keyword argument %r" % name)
    v = dict(KEYWORDS, **given)
    geometry = dict(n_feats=_N_FEATS, i_max=i_max, binsizes=binsizes, w_prom=w_prom, w_max=w_max)
    if bool(v["transplant_bed"]) != bool(v["transplant_out"]):
        raise ValueError("predict: transplant_bed and transplant_out go together")
    A.interaction_index(v["interaction_index"], "predict")
    for check, options, _ in _prechecks(v):
        check(options, geometry)
    seed_everything(seed)
    meta = pd.read_csv(meta_path)
    run = W.Run(meta_path, npy_dir, meta, regression, bsz, geometry, progress, store_path, donor_npy_dir, donor_meta, donor_store_path)
    wanted = [out for out in OUTS if v[out.dest]]
    if any(out.raw for out in wanted):
        W.require_raw_signals(run.dataset(raw=True))
    if v["raw_donor_ig_dir"]:
        if not donor_npy_dir:
            raise ValueError("predict: raw_donor_ig_dir needs donor_npy_dir")
        W.require_raw_signals(run.dataset(donor=True, raw=True))
        A.same_regions(run.dataset(raw=True), run.dataset(donor=True, raw=True))
    if any(out.donor and not out.raw for out in wanted):      # (the readers of the donor store)
        if not donor_npy_dir:
            raise ValueError("predict: %s need donor_npy_dir" % " / ".join(_DONOR_NAMED + ("contact_donor_shapley_out",)))
        A.same_regions(run.dataset(), run.dataset(donor=True))
    run.store = run.find_store()
    Model = ChromoformerRegressor if regression else ChromoformerClassifier
    run.model = Model(_N_FEATS, 128, 128, dict(n_layers=1, n_heads=2, d_model=128, d_ff=128), dict(n_layers=2, n_heads=2, d_model=128, d_ff=256),
                      dict(n_layers=6, n_heads=8, d_model=256, d_ff=256), binsizes=list(binsizes), seed=seed, i_max=i_max, w_max=w_max,
                      max_batch=bsz)
    if weights is not None:
        ckpt = torch.load(weights, map_location="cpu", weights_only=False)
        run.model.load_state_dict(modernise_keys(ckpt["net"] if "net" in ckpt else ckpt))
    run.model.cuda()
    out = Trainer(run.model, use_graph=False).evaluate_store(run.store, bsz).cpu()          # device gather + forward per batch, logits in store order
    pred = out.numpy().reshape(-1) if regression else torch.sigmoid(out).numpy()[:, 1]
    calls = {}      # (writer, fixed) -> (reads the donor store, the call's keyword arguments): rows that share a writer call fill one entry
    for row in wanted:
        _, kw = calls.setdefault((row.writer, tuple(sorted(row.fixed.items()))), (row.donor and not row.raw, dict(row.fixed)))
        kw.update({row.arg: v[row.dest]}, **{name: v[dest] for dest, name in row.options.items()})
    for block in (True, False):      # the readers of the donor store as one block, after which it is released; then the rest, in table order
        for (writer, _), (reads_donor_store, kw) in calls.items():
            if reads_donor_store == block:
                writer(run, **kw)
        run.release_donor()
    return meta, pred.astype(np.float32)


_GEOMETRY = dict(n_feats=_N_FEATS, **{k: p.default for k, p in inspect.signature(predict).parameters.items() if k in ("i_max", "binsizes", "w_prom", "w_max")})


def build_parser():
    ap = argparse.ArgumentParser(description="Chromoformer expression prediction on the MI355X path")
    for r in TABLE:
        if isinstance(r, Arg):
            ap.add_argument(*r.flags, help=r.help, **(dict(action="store_true") if r.switch else dict(required=True) if r.required else dict(default=None)))
        elif isinstance(r, Opt) and r.switch:
            ap.add_argument(_flag(r.dest), action="store_true", help=r.help)
        else:      # (an option's default is None on the command line: main() tells "not given" by it)
            more = {k: getattr(r, k) for k in ("type", "choices") if getattr(r, k, None) is not None}
            ap.add_argument(_flag(r.dest), default=None, help=r.help, **more)
    return ap


def _owners(flag):
    """What one of `flag` must come with: for an output, what it needs; for the donor's inputs, the outputs that read the donor; for an
    option, the outputs it applies to."""
    if flag in ("donor_npy_dir", "donor_meta", "donor_store"):
        return tuple(out.dest for out in OUTS if out.donor)
    return next((_needs(out) for out in OUTS if out.dest == flag), None) or tuple(out.dest for out in OUTS if flag in out.options)


_DONOR_NAMED = ("mark_donor_shapley_out", "mark_donor_epistasis_out", "mark_donor_sampled_shapley_out", "window_donor_shapley_out",
                "fine_window_donor_shapley_out", "mark_donor_interactions_out", "mark_donor_sampled_interactions_out",
                "mark_donor_dividends_out")      # the donor outputs that the two "need donor_npy_dir" refusals list, in their wording's order
_MARK_NEED = ("--mark-players / --mark-scale need --mark-shapley-out, --mark-epistasis-out, --mark-interactions-out or --mark-dividends-out"
              " (--mark-players also applies to --mark-donor-shapley-out / --mark-donor-epistasis-out, --mark-scale to"
              " --mark-sampled-shapley-out)")
_NEEDS = [(flags, tuple(dict.fromkeys(owner for flag in flags for owner in _owners(flag))), message) for flags, message in (
    # (flags, the flags they must come with -- from the table --, the refusal where one of the former is given and none of the latter), in
    # the order checked; the wording is irregular and stays literal
    (("raw_saliency_target", "raw_saliency_times_input"), "--raw-saliency-target / --raw-saliency-times-input need --raw-saliency-dir"),
    (("ig_steps", "ig_method", "ig_target"), "--ig-steps / --ig-method / --ig-target need --ig-dir or --raw-ig-dir (or --raw-donor-ig-dir)"),
    (("scan_scale", "scan_width", "scan_regions"), "--scan-scale / --scan-width / --scan-regions need --scan-out"),
    (("fine_scan_region", "fine_scan_width", "fine_scan_stride", "fine_scan_zoom", "fine_scan_scale"),
     "--fine-scan-region / --fine-scan-width / --fine-scan-stride / --fine-scan-zoom / --fine-scan-scale need --fine-scan-out"),
    (("interaction_index",), "--interaction-index needs --pcre-interactions-out, --mark-interactions-out or --mark-donor-interactions-out"
     " (or --mark-sampled-interactions-out, --mark-donor-sampled-interactions-out)"),
    (("mark_focal",), "--mark-focal needs --mark-sampled-interactions-out or --mark-donor-sampled-interactions-out"),
    (("raw_donor_ig_dir",), "--raw-donor-ig-dir needs --donor-npy-dir"),
    (_DONOR_NAMED, "%s need --donor-npy-dir" % " / ".join("--" + name.replace("_", "-") for name in _DONOR_NAMED)),
    (("mark_donor_backselect_out",), "--mark-donor-backselect-out needs --donor-npy-dir"),
    (("contact_donor_shapley_out",), "--contact-donor-shapley-out needs --donor-npy-dir"),
    (("contact_players",), "--contact-players needs --contact-shapley-out, --contact-interactions-out, --contact-dividends-out or --contact-donor-shapley-out"),
    (("contact_scale",), "--contact-scale needs --contact-shapley-out, --contact-interactions-out or --contact-dividends-out (the donor rule has no scale)"),
    (("contact_donor_marks",), "--contact-donor-marks needs --contact-donor-shapley-out"),
    (("mark_backselect_players", "backselect_mode", "backselect_frac"),
     "--mark-backselect-players / --backselect-mode / --backselect-frac need --mark-backselect-out or --mark-donor-backselect-out"),
    (("donor_npy_dir", "donor_meta", "donor_store"),
     "--donor-npy-dir / --donor-meta / --donor-store need --mark-donor-shapley-out, --mark-donor-epistasis-out or "
     "--mark-donor-sampled-shapley-out (or --window-donor-shapley-out, --fine-window-donor-shapley-out, "
     "--mark-donor-interactions-out, --mark-donor-sampled-interactions-out, --mark-donor-dividends-out)"),
    (("mark_sampled_players", "mark_perms", "mark_seed"),
     "--mark-sampled-players / --mark-perms / --mark-seed need --mark-sampled-shapley-out or --mark-donor-sampled-shapley-out"
     " (or --mark-sampled-interactions-out, --mark-donor-sampled-interactions-out)"),
    (("mark_scale",), _MARK_NEED),
    (("mark_players",), _MARK_NEED),
    (("window_players", "window_width", "window_perms", "window_seed"),
     "--window-players / --window-width / --window-perms / --window-seed need --window-shapley-out or --window-donor-shapley-out"),
    (("window_scale",), "--window-scale needs --window-shapley-out (the donor rule has no scale)"),
    (("fine_window_region", "fine_window_width", "fine_window_players", "fine_window_zoom", "fine_window_perms", "fine_window_seed"),
     "--fine-window-region / --fine-window-width / --fine-window-players / --fine-window-zoom / --fine-window-perms / "
     "--fine-window-seed need --fine-window-shapley-out or --fine-window-donor-shapley-out"),
    (("fine_window_scale",), "--fine-window-scale needs --fine-window-shapley-out (the donor rule has no scale)"),
    (("transplant_bed",), "--transplant-bed needs --transplant-out"),
    (("transplant_out",), "--transplant-out needs --transplant-bed"),
    (("transplant_freq", "transplant_slot"), "--transplant-freq / --transplant-slot need --transplant-out"),
)]


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)

    def given(name):      # (an option of _DEFAULTS: it was given; an output, a directory or a switch: it is set)
        return getattr(args, name) is not None if name in _DEFAULTS else bool(getattr(args, name))

    for flags, owners, message in _NEEDS:
        if any(given(name) for name in flags) and not any(given(name) for name in owners):
            ap.error(message)
    for name, default in _DEFAULTS.items():
        if getattr(args, name) is None:
            setattr(args, name, default)
    for name, rule in _RULES.items():      # (the options' value rules; a rule may convert the value)
        for o in OPTS:
            if o.rule == name:
                try:
                    setattr(args, o.dest, rule(o, getattr(args, o.dest), args))
                except ValueError as e:
                    ap.error(str(e))
    if args.raw_donor_ig_dir and args.donor_store:
        ap.error("--raw-donor-ig-dir reads the donor's raw .npy signals; --donor-store does not serve it")
    for check, options, row in _prechecks(vars(args)):      # (at predict()'s default geometry: a bad count, name or file is a usage error)
        try:
            check(options, _GEOMETRY)
        except (OSError, ValueError) as e:
            ap.error(row.prefix + getattr(e, "cli", str(e)))
    kw = {name: value for name, value in vars(args).items() if name not in ("meta", "npy_dir", "weights", "regression", "output", "store", "donor_store")}
    meta, pred = predict(args.meta, args.npy_dir, args.weights, args.regression, progress=True, store_path=args.store,
                         donor_store_path=args.donor_store, **kw)
    print("Predicting expressions for %d genes." % len(meta))
    meta["prediction"] = pred
    meta.to_csv(args.output, index=False)
    from sklearn import metrics
    if args.regression:
        from scipy.stats import pearsonr
        y = np.log2(meta["expression"] + 1)
        print("R2 : %s" % metrics.r2_score(y, meta["prediction"]))
        print("Pearson's r : %s" % pearsonr(y, meta["prediction"])[0])
    else:
        print("ROC-AUC : %s" % metrics.roc_auc_score(meta["label"], meta["prediction"]))
        print("Average Precision : %s" % metrics.average_precision_score(meta["label"], meta["prediction"]))
        print("Accuracy : %s" % metrics.accuracy_score(meta["label"], (meta["prediction"] > 0.5).astype(int)))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
