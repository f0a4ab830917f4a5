"""The attribution methods of the Chromoformer models: attention maps, pCRE ablation, the coalition games of the pCREs and of the
histone marks (coalitions, exact and sampled Shapley values, epistasis, interaction indices, dividends), integrated gradients and the
perturbation scans.  AttributionMixin is a plain mixin of net.ChromoformerBase, which supplies construction, packing, the forward and
the training methods; every method here runs in the library (csrc/), there is no PyTorch fallback.

The 25 game methods are one runner, _game, over two small tables: _FAMILIES (who the players are) and _KINDS (what is computed); the
functions of chromoformer_amd.backselect run the kind "backselect" through the same runner, those of chromoformer_amd.contact the
family "contact"."""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from . import attribution as A

# The families of games.  Per family: the options struct of the C calls (None: the call takes none and `info` names no players), the
# player parser -> (arrays..., names), the struct fields those arrays go to, the word parser of `keep`, what `keep` holds (for the
# refusal of a call without it), and the key of the every-player-absent row in `info` ("either": "erased", or "donor" where a donor
# is given; "donor": the family needs one).
_WORDS, _WIDE = "the coalition words (bit p set: player p present)", "the coalitions (bit p set: player p present)"
_FAMILIES = {
    "pcre": (None, None, (), A.coalition_words, "the coalition words (bit j set: pCRE slot j kept)", "promoter_only"),
    "contact": (_lib.cf_contact_opts, lambda spec, n_feats, i_max: A.contact_players(spec, i_max), ("player_drop", "player_contact"),
                A.mark_coalition_words, _WORDS, "either"),
    "mark": (_lib.cf_mark_opts, A.mark_players, ("player_marks", "player_regions"), A.mark_coalition_words, _WORDS, "erased"),
    "mark_donor": (_lib.cf_mark_donor_opts, A.mark_players, ("player_marks", "player_regions"), A.mark_coalition_words, _WORDS, "donor"),
    "mark_wide": (_lib.cf_mark_wide_opts, A.mark_players_wide, ("player_marks", "player_regions"), A.mark_wide_words, _WIDE, "either"),
    "mark_window": (_lib.cf_mark_window_opts, A.window_players, ("player_marks", "player_regions", "player_lo", "player_hi"),
                    A.mark_wide_words, _WIDE, "either"),
    "mark_fine_window": (_lib.cf_mark_fine_opts, A.fine_window_players, ("player_marks", "player_lo", "player_hi"), A.mark_wide_words, _WIDE,
                         "either"),
}


def _shapley_info(o, g):
    n = o["rows"].shape[1]
    info = {"logits": o["rows"][:, n - 1].clone(), g.absent: o["rows"][:, 0].clone()}
    if g.names is not None:
        info["players"] = g.names
    info["delta"] = o["phi"].sum(1) - (info["logits"] - info[g.absent])
    if g.table:
        info["coalitions"] = o["rows"]
    return o["phi"], info


def _interactions_info(o, g):
    """rows [B, 2^P, n_out], word m at column m."""
    inter, rows = o["inter"], o["rows"]
    info = {"phi": o["phi"], "logits": rows[:, rows.shape[1] - 1].clone(), g.absent: rows[:, 0].clone(), "index": g.index}
    if g.names is not None:
        info["players"] = g.names
    if g.index == "sti":      # efficiency: the diagonal plus the upper triangle sums to v(N) - v(0)
        upper = torch.triu(torch.ones(g.P, g.P, dtype=torch.bool, device=inter.device))
        info["delta"] = inter[:, upper].sum(1) - (info["logits"] - info[g.absent])
    if g.table:
        info["coalitions"] = rows
    return inter, info


def _epistasis_info(o, g):
    info = {"logits": o["rows"][:, 0].clone(), "single": o["rows"][:, 1:1 + g.P].clone()}
    if g.names is not None:
        info["players"] = g.names
    return o["eps"], info


def _sampled_info(o, g):
    rows = o["rows"]
    info = {"logits": rows[:, 1].clone(), "absent": rows[:, 0].clone(), "stderr": o["se"], "names": g.names, "permutations": g.perms}
    info["delta"] = o["phi"].sum(1) - (info["logits"] - info["absent"])
    if g.table:
        info["rows"] = rows
    return o["phi"], info


def _pairs_sampled_info(o, g):
    """See mark_shapley_interactions_sampled."""
    inter, rows, dev, F = o["inter"], o["rows"], o["inter"].device, len(g.focal)
    at = torch.as_tensor([A.focal_row_count(g.perms, g.focal[:f]) for f in range(F)], device=dev)      # {i} alone; everybody but i follows it
    info = {"stderr": o["se"], "phi": o["phi"], "phi_stderr": o["phi_se"], "logits": rows[:, 1].clone(), "absent": rows[:, 0].clone(),
            "alone": rows[:, at].clone(), "without": rows[:, at + 1].clone(), "index": g.index, "names": g.names,
            "focal": g.focal, "permutations": g.perms, "col": g.col, "delta": None}
    if g.index == "sii":      # every order telescopes: sum_{j != i} d(j) = (v(N) - v(N - i)) - (v({i}) - v(0))
        off = torch.ones(F, g.P, dtype=torch.bool, device=dev)
        off[torch.arange(F, device=dev), torch.as_tensor(g.focal.astype(np.int64), device=dev)] = False
        total = (inter * off[None, :, :, None]).sum(2)
        info["delta"] = total - ((info["logits"][:, None] - info["without"]) - (info["alone"] - info["absent"][:, None]))
    if g.table:
        info["rows"] = rows
    return inter, info


def _backselect_info(o, g):
    """See backselect.mark_backselect.  rows: round-major blocks, views of one buffer."""
    B, P, n_out, flat = o["order"].shape[0], g.P, o["values"].shape[2], o["rows"].view(-1, o["values"].shape[2])
    ends = flat[:2 * B].view(B, 2, n_out)
    info = {"values": o["values"], "size": o["size"], "subset": A.subset_bools(o["subset"], P), "names": g.names, "logits": ends[:, 1].clone(),
            "absent": ends[:, 0].clone(), "threshold": o["thr"], "direction": o["dir"], "mode": g.select.mode, "target": g.select.target}
    if g.table:
        info["rows"], at = [ends], 2 * B
        for t in range(P - 1):
            info["rows"].append(flat[at:at + B * (P - t)].view(B, P - t, n_out))
            at += B * (P - t)
    return o["order"], info


# The kinds of call a family offers.  Per kind: the outputs the library writes in full, each [B, *shape(g), n_out], the first being the
# table of forwards (one row of feats_out each); the C arguments between the options and the stream (an output, a host value of the
# call `g`, or #name: its length); (result, info) from the outputs; and the exact game's refusal of more than 16 players, if it is one.
_KINDS = {
    "coalitions": ((("logits", lambda g: (len(g.words),)),), "words #words logits", lambda o, g: o["logits"], None),
    "shapley": ((("rows", lambda g: (1 << g.P,)), ("phi", lambda g: (g.P,))), "phi rows", _shapley_info,
                "%(who)s: %(P)d players; the exact game takes 1..16: choose a larger width or %(who)s_sampled"),
    "epistasis": ((("rows", lambda g: (1 + g.P + g.P * (g.P - 1) // 2,)), ("eps", lambda g: (g.P, g.P))), "eps rows", _epistasis_info, None),
    "shapley_interactions": ((("rows", lambda g: (1 << g.P,)), ("inter", lambda g: (g.P, g.P)), ("phi", lambda g: (g.P,))),
                             "code inter phi rows", _interactions_info,
                             "%(who)s: %(P)d players; the exact game takes 2..16 and the index has no sampled estimator: choose a larger width"),
    "shapley_sampled": ((("rows", lambda g: (2 + len(g.perms) * (g.P - 1),)), ("phi", lambda g: (g.P,)), ("se", lambda g: (g.P,))),
                        "perms #perms phi se rows", _sampled_info, None),
    "shapley_interactions_sampled": ((("rows", lambda g: (len(g.words),)), ("inter", lambda g: (len(g.focal), g.P)),
                                      ("se", lambda g: (len(g.focal), g.P)), ("phi", lambda g: (g.P,)), ("phi_se", lambda g: (g.P,))),
                                     "perms #perms focal #focal code inter se phi phi_se rows", _pairs_sampled_info, None),
    # (an output with a dtype is [B, *shape(g)] of that dtype, no n_out; the two structs are filled once the outputs exist)
    "backselect": ((("rows", lambda g: (A.backselect_row_count(g.P),)), ("values", lambda g: (g.P + 1,)), ("order", lambda g: (g.P,), torch.int32),
                    ("size", lambda g: (), torch.int32), ("subset", lambda g: ((g.P + 31) // 32,), torch.int32), ("thr", lambda g: (), torch.float32),
                    ("dir", lambda g: (), torch.int32)), "bopts bout", _backselect_info, None),
}

# What five docstrings say about `inter`, filled per method with the absent key, the sibling method and the line about the players
# (contact.contact_shapley_interactions fills it too).
_INTER_DOC = """inter               [B, P, P, n_out], exactly symmetric.  Off the diagonal, with S over the coalitions that hold neither player,
                              I_ij = sum_S w(|S|) ((v(S + i + j) - v(S + j)) - (v(S + i) - v(S))): how much i's marginal contribution
                              changes with j present, averaged over every context -- negative for redundant players, positive for
                              cooperating ones, also where a third player hides the effect from the full-coalition *_epistasis.  index "sii"
                              (Shapley interaction index): w(s) = s! (P - s - 2)! / (P - 1)!, the diagonal is phi.  index "sti"
                              (Shapley-Taylor, order 2): w(s) = (2 / P) / C(P - 1, s), the diagonal is v({i}) - v(nobody), and the
                              diagonal plus the upper triangle sums to logits - %(absent)s.  A null player's row and column are exactly 0
          info["phi"]         [B, P, n_out]: the Shapley values of %(sibling)s on the same rows, bit for bit
          info["logits"]      [B, n_out]: the prediction;  info["%(absent)s"]  [B, n_out]: every player absent
          info["index"]       the index name;  info["delta"]  [B, n_out], "sti" only: the efficiency gap (rounding only)%(players)s
          info["coalitions"]  [B, 2^P, n_out], with return_coalitions: the logits of every coalition, word m at column m

        SHAP's interaction values follow from the sii result: Phi_ij = I_ij / 2 off the diagonal and Phi_ii = phi_i - sum_{j != i} I_ij / 2."""


class AttributionMixin:
    MAP_KEYS = ("embed", "pairwise_interaction", "regulation", "regulatory_embedding")

    def _attrib_call(self, who, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                     interaction_freq=None):
        """What the attribution methods share -> (batch struct, book).  The six tensors of forward(), or a packed batch (an engine.Slot,
        a pack_batch result or a batch struct) with nothing after it.  book() -> stream, called directly in front of the library call,
        once the arguments are accepted: it brings the tiled weights up to date on the stream and books the call as `who` (a pending
        backward of an earlier forward then refuses to run).  book keeps what the batch struct points to alive."""
        if promoter_pad_masks is None:
            p = promoter_feats
            bs, keep = (p if isinstance(p, _lib.cf_batch) else p.struct if hasattr(p, "struct") else p[0]), p
        else:
            bs, keep = self._pack(promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq)
        if self._handle is None:
            raise RuntimeError("call .cuda() first: the Chromoformer HIP path needs device buffers")

        def book(_alive=keep):
            st = torch.cuda.current_stream(self._device).cuda_stream
            self._sync_tiled(st)
            self._maps_gen += 1
            self._maps_by = who
            return st

        return bs, book

    def _game(self, who, family, kind, batch, keep=None, index=None, focal=None, perms=None, table=False, feats=False, players=None, width=1,
              scale=0.0, donor=None, flip=None, fine=None, select=None):
        """The one body of the game methods: method `who` is call `kind` (_KINDS) of `family` (_FAMILIES) on `batch`, the six arguments
        of forward().  keep / index / focal / perms = (n_perm, seed, permutations): the kind's arguments; table: return_coalitions or
        return_rows; feats: return_feats; players .. flip: the family's options; fine = (region, n_windows, start, lengths) of the fine
        game; select = (mode, frac, threshold, target, direction) of a back-selection.  What can be refused without the batch is refused before the device is asked for (the fine game needs `start` to know its
        players); book() runs once every argument has been accepted, directly in front of the library call."""
        struct, parse, fields, parse_words, keep_what, absent = _FAMILIES[family]
        outputs, c_args, result, too_many = _KINDS[kind]
        stem = "cf_" + who.replace("mark_fine_window_", "mark_fine_")
        g = SimpleNamespace(P=self.i_max, names=None, index=index, table=table, focal=focal)      # the host values of the call
        if kind == "coalitions" and keep is None:
            raise ValueError("%s: keep is required: %s" % (who, keep_what))
        if kind == "backselect":
            g.select = self._backselect_args(who, *select)
        if "interactions" in kind:
            g.code = A.interaction_index(index, stem[3:])
        if kind == "shapley_interactions_sampled" and focal is None:
            raise ValueError("%s: focal is required: the players whose interactions are asked for (indices or names)" % stem[3:])

        def play(*arrays):
            """Once the players are known: the exact game's limit, the words of `keep`, the orders and the focal players -> arrays."""
            if struct is not None:
                g.P, g.names = len(arrays[0]), arrays[-1]
            if too_many and g.P > 16:
                raise ValueError(too_many % {"who": who, "P": g.P})
            if kind == "coalitions":
                g.words = parse_words(keep, g.P, who)
            if perms is not None:
                g.perms = self._permutations(who, g.P, *perms)
            if kind == "shapley_interactions_sampled":
                if g.P < 2:
                    raise ValueError("%s: %d player; a pair needs at least 2" % (stem[3:], g.P))
                g.focal = A.focal_players(focal, g.names, g.P)
                g.words, g.col = A.focal_words(g.perms, g.focal)      # (the rows of the table)
            return arrays[:-1]

        if family == "mark_window":
            arrays = play(*parse(players, self.n_feats, self.i_max, min(self.n_bins), width))
        elif family != "mark_fine_window":
            arrays = play(*parse(players, self.n_feats, self.i_max)) if parse else play()
        bs, book = self._attrib_call(who, *batch)
        head = [self._handle, C.byref(bs)]
        if struct is not None:
            opts, alive = struct(), ()
            if family == "mark_fine_window":
                region, n_windows, start, lengths = fine
                opts.region = int(region)
                n_windows, alive = self._fine_args(who, opts, bs.B, start, lengths, n_windows, int(width))
                arrays = play(*parse(players, self.n_feats, int(width), n_windows))
            alive += self._game_opts(who, opts, fields, arrays, scale, flip, donor, absent == "donor", bs.B)      # (kept until the call is issued)
            head.append(C.byref(opts))
            if absent == "either":
                absent = "erased" if donor is None else "donor"
        g.absent = absent
        out = {o[0]: torch.empty(bs.B, *o[1](g), self.n_out, device=self._device) if len(o) == 2 else
               torch.empty(bs.B, *o[1](g), dtype=o[2], device=self._device) for o in outputs}      # (written in full by the library)
        if kind == "backselect":
            g.bopts, g.bout, kept = self._backselect_structs(who, g.select, bs.B, out)
            alive += kept
        feats = self._feats_out(opts, bs.B, out[outputs[0][0]].shape[1]) if feats else None

        def c_arg(a):
            if a in out:
                return out[a].data_ptr()
            v = len(getattr(g, a[1:])) if a[0] == "#" else getattr(g, a)
            return v.ctypes.data if isinstance(v, np.ndarray) else v

        args = [c_arg(a) for a in c_args.split()]
        st = book()
        _lib.check(getattr(_lib.lib(), stem)(*head, *args, st), stem)
        res = result(out, g)
        if feats is None:
            return res
        if kind == "coalitions":
            return res, feats
        res[1]["feats"] = feats
        return res

    def _backselect_args(self, who, mode, frac, threshold, target, direction):
        """The options of a back-selection, checked on the host -> namespace(mode, code, frac, threshold, target, direction)."""
        if mode not in _lib.BACKSELECT_MODE:
            raise ValueError("%s: mode = %r: 'backward' (remove players from everybody) or 'forward' (add players to nobody)" % (who, mode))
        if direction not in ("auto", 1, -1):
            raise ValueError("%s: direction = %r: 'auto' (from the two end rows), 1 or -1" % (who, direction))
        target = (1 if self.n_out == 2 else 0) if target is None else int(target)
        if not 0 <= target < self.n_out:
            raise ValueError("%s: target = %d outside [0, n_out = %d)" % (who, target, self.n_out))
        frac = float(frac)
        if not np.isfinite(frac):
            raise ValueError("%s: frac = %r: a finite number (the share of logits - absent a sufficient set keeps)" % (who, frac))
        return SimpleNamespace(mode=mode, code=_lib.BACKSELECT_MODE[mode], frac=frac, threshold=threshold, target=target,
                               direction=0 if direction == "auto" else int(direction))

    def _backselect_structs(self, who, s, B, out):
        """cf_backselect_opts and cf_backselect_out of a call on B genes -> (byref opts, byref out, what they point to besides `out`)."""
        o, w, thr = _lib.cf_backselect_opts(), _lib.cf_backselect_out(), None
        o.mode, o.target, o.direction, o.frac = s.code, s.target, s.direction, s.frac
        if s.threshold is not None:
            thr = torch.as_tensor(s.threshold, dtype=torch.float32).to(self._device).contiguous()
            if thr.shape != (B,):
                raise ValueError("%s: threshold has shape %s; expected [B = %d] floats, one per gene" % (who, tuple(thr.shape), B))
            o.threshold = thr.data_ptr()
        for field, name in (("order", "order"), ("values", "values"), ("size", "size"), ("subset", "subset"), ("rows", "rows"),
                            ("threshold", "thr"), ("direction", "dir")):
            if name in out:
                setattr(w, field, out[name].data_ptr())
        return C.byref(o), C.byref(w), (o, w, thr)

    def _backselect_table(self, coalitions, mode, frac, threshold, target, direction, names):
        """The body of backselect.backselect: cf_backselect_from_rows on a kept coalition table."""
        who = "backselect"
        s = self._backselect_args(who, mode, frac, threshold, target, direction)
        rows, B, P = self._table_check(who, "coalitions", coalitions)
        g = SimpleNamespace(P=P, names=names, select=s, table=False)
        out = {"values": torch.empty(B, P + 1, self.n_out, device=self._device), "order": torch.empty(B, P, dtype=torch.int32, device=self._device),
               "size": torch.empty(B, dtype=torch.int32, device=self._device), "subset": torch.empty(B, 1, dtype=torch.int32, device=self._device),
               "thr": torch.empty(B, device=self._device), "dir": torch.empty(B, dtype=torch.int32, device=self._device)}
        bopts, bout, _alive = self._backselect_structs(who, s, B, out)
        st = torch.cuda.current_stream(self._device).cuda_stream
        _lib.check(_lib.lib().cf_backselect_from_rows(self._handle, rows.data_ptr(), B, P, self.n_out, bopts, bout, st), "cf_backselect_from_rows")
        full = (1 << P) - 1
        out["rows"] = torch.stack((rows[:, 0], rows[:, full]), 1)      # nobody, everybody: what _backselect_info reads of a game's rows
        return _backselect_info(out, g)

    def _game_opts(self, who, opts, fields, arrays, scale, flip, donor, need_donor, B):
        """The fields the options structs of the mark games share, filled for a batch of B genes -> what they point to besides `arrays`.
        donor: None (the scale rule, unless the family needs one) or one of the forms of _donor_feats."""
        opts.n_players = len(arrays[0])
        for field, a in zip(fields, arrays):
            setattr(opts, field, a.ctypes.data)
        if hasattr(opts, "scale"):
            opts.scale = float(scale)
        alive = (self._set_flip(who, opts, flip, B),) if hasattr(opts, "flip") else ()
        if hasattr(opts, "donor_freq"):      # (the contact games: the donor is a frequency tensor)
            return alive + self._donor_freq(who, opts, donor, B)
        if need_donor or donor is not None:
            alive += self._donor_feats(who, donor, B, opts)
        return alive

    @torch.no_grad()
    def attention_maps(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                       interaction_freq=None, which=MAP_KEYS):
        """Logits and what a user of the reference reads off its attention modules (modules.py:73, 184) and fc_head input, from one
        forward pass (cf_attention_maps) -> (logits [B, n_out], maps), tensors on the model's device.  Per binsize b, L = n_bins[b],
        T = i_max + 1:

          maps["embed"][b]                 [B, embed.n_heads, L]                       centre query's softmax row of the Embedding layer
          maps["pairwise_interaction"][b]  [B, pw.n_layers, i_max, pw.n_heads, L]     promoter centre row over each pCRE's bins, per layer
          maps["regulation"][b]            [B, reg.n_layers, reg.n_heads, T]           row 0 (promoter token) over [promoter, pCRE slots]
          maps["regulatory_embedding"]     [B, 3 * d_emb]                              cat(x_out[b][:, 0]) + cat(x_in[b][:, 0])

        Masked keys are 0, fully masked rows (dummy pCRE slots) uniform, as with the reference.  `which` selects the outputs (the others
        are not copied).  The first argument may also be a packed batch (an engine.Slot or a pack_batch result), with nothing after it.
        The pass overwrites the activations a grad-enabled model(...) keeps for its backward: such a pending backward() raises."""
        bs, book = self._attrib_call("attention_maps", promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks,
                                     interaction_freq)
        which = (which,) if isinstance(which, str) else tuple(which)
        bad = [k for k in which if k not in self.MAP_KEYS]
        if bad:
            raise ValueError("attention_maps: unknown output(s) %s; choose from %s" % (bad, self.MAP_KEYS))
        B, S, T, dev = bs.B, self.i_max, self.i_max + 1, self._device
        embed, pair, reg = self._kws
        want = _lib.cf_attn_maps()
        maps = {k: {} for k in which if k != "regulatory_embedding"}
        for r, b in enumerate(self.binsizes):
            L = self.n_bins[r]
            for key, field, shape in (("embed", "embed", (B, embed["n_heads"], L)),
                                      ("pairwise_interaction", "pairwise", (B, pair["n_layers"], S, pair["n_heads"], L)),
                                      ("regulation", "regulation", (B, reg["n_layers"], reg["n_heads"], T))):
                if key in maps:
                    t = maps[key][b] = torch.empty(shape, device=dev)      # (written in full by the library)
                    getattr(want, field)[r] = t.data_ptr()
        if "regulatory_embedding" in which:
            maps["regulatory_embedding"] = t = torch.empty(B, len(self.binsizes) * self.d_emb, device=dev)
            want.embedding = t.data_ptr()
        logits = torch.empty(B, self.n_out, device=dev)
        st = book()
        _lib.check(_lib.lib().cf_attention_maps(self._handle, C.byref(bs), logits.data_ptr(), C.byref(want), st), "cf_attention_maps")
        return logits, maps

    @torch.no_grad()
    def pcre_ablation(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                      interaction_freq=None):
        """In-silico pCRE deletion (cf_pcre_ablation) -> logits [B, i_max + 2, n_out] on the model's device, no autograd graph:

          [:, 0]          the prediction (model(...) under no_grad, bit-equal)
          [:, 1 + j]      with pCRE slot j deleted: interaction_masks row and column j + 1 set at every resolution (= the slot made a
                          dataset dummy, data.py); a slot that is already a dummy gives [:, 0]
          [:, i_max + 1]  the promoter alone: rows and columns 1..i_max set

        The Embedding + Pairwise stage runs once, the Regulation stack and the head on the B * (i_max + 2) gene-variants.  The first
        argument may also be a packed batch (an engine.Slot or a pack_batch result), with nothing after it.  The pass overwrites the
        activations a grad-enabled model(...) keeps for its backward: such a pending backward() raises."""
        bs, book = self._attrib_call("pcre_ablation", promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks,
                                     interaction_freq)
        logits = torch.empty(bs.B, self.i_max + 2, self.n_out, device=self._device)      # (written in full by the library)
        st = book()
        _lib.check(_lib.lib().cf_pcre_ablation(self._handle, C.byref(bs), logits.data_ptr(), st), "cf_pcre_ablation")
        return logits

    @torch.no_grad()
    def pcre_coalitions(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                        interaction_freq=None, keep=None):
        """The prediction under pCRE coalitions (cf_pcre_coalitions) -> logits [B, n_coal, n_out] on the model's device, no autograd
        graph.  `keep`: a sequence / array of ints, bit j set = pCRE slot j kept, or a bool array [n_coal, i_max].  Column c is the
        inference forward with interaction_masks row and column j + 1 set, at every resolution, for every slot j that keep[c] drops
        (model(...) under no_grad on those masks, bit-equal): 2^i_max - 1 is the prediction, 0 the promoter alone; a bit of a slot
        that is already a dummy changes nothing; a bit >= i_max raises ValueError.  The Embedding + Pairwise stage runs once, the
        Regulation stack and the head on the B * n_coal rows.  The first argument may also be a packed batch (an engine.Slot or a
        pack_batch result), with nothing after it.  The pass overwrites the activations a grad-enabled model(...) keeps for its
        backward: such a pending backward() raises."""
        batch = (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq)
        return self._game("pcre_coalitions", "pcre", "coalitions", batch, keep=keep)

    @torch.no_grad()
    def pcre_shapley(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                     interaction_freq=None, return_coalitions=False):
        """Exact Shapley values of the pCRE slots (cf_pcre_shapley) -> (phi, info), tensors on the model's device, no autograd graph:

          phi                    [B, i_max, n_out]: slot j's average marginal contribution to each logit over all orders of adding
                                 the pCREs to the promoter; exactly 0 for a dummy slot
          info["logits"]         [B, n_out]: the prediction (all pCREs kept; model(...) under no_grad, bit-equal)
          info["promoter_only"]  [B, n_out]: the promoter alone
          info["delta"]          [B, n_out]: phi.sum(1) - (logits - promoter_only), the efficiency gap (rounding only)
          info["coalitions"]     [B, 2^i_max, n_out], with return_coalitions: the logits of every coalition, word m at column m

        All 2^i_max coalitions run from one trunk pass (pcre_coalitions); the values are in logit space, where efficiency holds.
        The first argument may also be a packed batch (an engine.Slot or a pack_batch result), with nothing after it.  The pass
        overwrites the activations a grad-enabled model(...) keeps for its backward: such a pending backward() raises."""
        batch = (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq)
        return self._game("pcre_shapley", "pcre", "shapley", batch, table=return_coalitions)

    @torch.no_grad()
    def pcre_shapley_interactions(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                                  interaction_freq=None, index="sii", return_coalitions=False):
        """Pairwise Shapley interaction indices of the pCRE slots (cf_pcre_shapley_interactions) -> (inter, info), tensors on the
        model's device, no autograd graph.  P = i_max (at least 2); the 2^i_max coalitions run once, as in pcre_shapley:

          %(inter)s
        The packed forms of the first argument and the effect on a pending backward() are those of pcre_shapley."""
        batch = (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq)
        return self._game("pcre_shapley_interactions", "pcre", "shapley_interactions", batch, index=index, table=return_coalitions)

    @torch.no_grad()
    def shapley_interactions(self, coalitions, index="sii"):
        """Pairwise Shapley interaction indices from a kept coalition table (cf_shapley_interactions_from_rows) -> inter
        [B, P, P, n_out] on the model's device: `coalitions` is info["coalitions"] of any exact *_shapley call, [B, 2^P, n_out] with
        word m at column m, 2 <= P <= 16 (a float32 tensor; moved to the model's device and made contiguous if it is not).  The bits
        are those of the *_shapley_interactions call on the same table (index as there); no forward runs and a pending backward() is
        left alone.
        SHAP's interaction values follow from the sii result: Phi_ij = I_ij / 2 off the diagonal and Phi_ii = phi_i - sum_{j != i} I_ij / 2."""
        code = A.interaction_index(index, "shapley_interactions")
        rows, B, P = self._table_check("shapley_interactions", "coalitions", coalitions, least=2)
        inter = torch.empty(B, P, P, self.n_out, device=self._device)      # (written in full by the library)
        st = torch.cuda.current_stream(self._device).cuda_stream
        _lib.check(_lib.lib().cf_shapley_interactions_from_rows(self._handle, rows.data_ptr(), B, P, code, inter.data_ptr(), st),
                   "cf_shapley_interactions_from_rows")
        return inter

    def _table_check(self, who, what, table, least=1):
        """A [B, 2^P, n_out] float32 table, least <= P <= 16, on the model's device, contiguous -> (table, B, P)."""
        if not torch.is_tensor(table) or table.dim() != 3 or table.dtype != torch.float32:
            raise ValueError("%s: %s must be a float32 tensor [B, 2^P, n_out]" % (who, what))
        B, n, n_out = table.shape
        P = n.bit_length() - 1
        if B < 1 or n != 1 << P or not least <= P <= 16 or n_out != self.n_out:
            raise ValueError("%s: %s has shape %s; expected [B >= 1, 2^P with P in %d..16, n_out = %d]"
                             % (who, what, tuple(table.shape), least, self.n_out))
        if self._handle is None:
            raise RuntimeError("%s: the model is not on a GPU (model.cuda() first); there is no CPU fallback" % who)
        return table.to(self._device).contiguous(), B, P

    @torch.no_grad()
    def shapley_dividends(self, coalitions, return_mass=False):
        """Harsanyi dividends (the Moebius transform) of a kept coalition table (cf_dividends_from_rows) -> div [B, 2^P, n_out] on the
        model's device, or (div, mass) with return_mass.  `coalitions` is info["coalitions"] of any exact *_shapley call, word m at
        column m, 1 <= P <= 16.  div[b, S] = sum over T <= S of (-1)^(|S| - |T|) v(T): what the players of S contribute TOGETHER beyond
        every smaller group of them; the dividends of all subsets of S add back up to v(S).  The fp32 result is the in-place
        butterfly (for k < P, for S with bit k: a[S] -= a[S ^ 1 << k]), bit for bit; the dividends of a set that holds a null player
        are exactly 0.  mass[b, S] = sum over T <= S of |v(T)| scales the rounding error (attribution.dividend_bound): a high-order
        dividend smaller than its bound is noise.  No forward runs and a pending backward() is left alone."""
        rows, B, P = self._table_check("shapley_dividends", "coalitions", coalitions)
        div = torch.empty_like(rows)      # (written in full by the library)
        mass = torch.empty_like(rows) if return_mass else None
        st = torch.cuda.current_stream(self._device).cuda_stream
        _lib.check(_lib.lib().cf_dividends_from_rows(self._handle, rows.data_ptr(), B, P, div.data_ptr(), mass.data_ptr() if return_mass else None, st),
                   "cf_dividends_from_rows")
        return (div, mass) if return_mass else div

    @torch.no_grad()
    def set_interactions(self, dividends, order=2, index="sii", sets=None):
        """An interaction index of sets of up to `order` players from the dividends (cf_set_interactions_from_dividends) -> (inter
        [B, n_sets, n_out] on the model's device, sets uint32 [n_sets]).  dividends: shapley_dividends' result; sets: words (bit p =
        player p), each with 1..order players; default attribution.interaction_sets(P, order), every such set by size and word.
        index "sii": the Shapley interaction index of any order (order 1 the Shapley values, order 2 the pairwise sii of
        shapley_interactions, within rounding); "sti": Shapley-Taylor of top order `order` -- sets below it carry their dividend's
        bits, and all sets together sum to logits - absent.  Weights: attribution.set_interaction_weights.  No forward runs."""
        who = "set_interactions"
        code = A.interaction_index(index, who)
        div, B, P = self._table_check(who, "dividends", dividends)
        order = int(order)
        if not 1 <= order <= P:
            raise ValueError("%s: order = %d outside 1..P = %d" % (who, order, P))
        if sets is None:
            words = A.interaction_sets(P, order)
        else:
            raw = np.asarray(sets.cpu() if hasattr(sets, "cpu") else sets)
            if raw.ndim != 1 or raw.size < 1 or raw.dtype.kind not in "iu" or raw.min() < 0 or raw.max() >= 1 << P:
                raise ValueError("%s: sets must be a non-empty 1-D integer array of words below 2^P = %d" % (who, 1 << P))
            words = np.ascontiguousarray(raw.astype(np.uint32))
        inter = torch.empty(B, len(words), self.n_out, device=self._device)      # (written in full by the library)
        st = torch.cuda.current_stream(self._device).cuda_stream
        _lib.check(_lib.lib().cf_set_interactions_from_dividends(self._handle, div.data_ptr(), B, P, words.ctypes.data, len(words), code, order,
                                                                 inter.data_ptr(), st), "cf_set_interactions_from_dividends")
        return inter, words

    def _dividends_info(self, phi, info, names):
        """(div, info) of a *_dividends call from its sibling's (phi, info with the coalitions)."""
        div, mass = self.shapley_dividends(info["coalitions"], return_mass=True)
        info = dict(info, phi=phi, mass=mass, names=list(names))
        info["sets"] = A.set_names(np.arange(div.shape[1], dtype=np.uint32), names)
        return div, info

    @torch.no_grad()
    def pcre_dividends(self, *args, **kwargs):
        """pcre_shapley(..., return_coalitions=True) with the same arguments, then shapley_dividends on its table -> (div, info): div
        [B, 2^i_max, n_out], word m at column m; info is pcre_shapley's (logits, promoter_only, delta, coalitions) plus phi (its
        Shapley values, bit for bit), mass (shapley_dividends), names ("pcre0", ...) and sets (the 2^P set names by word, "" for the
        empty set).  A dummy slot is a null player: every set that holds it has dividend exactly 0."""
        phi, info = self.pcre_shapley(*args, **dict(kwargs, return_coalitions=True))
        return self._dividends_info(phi, info, ["pcre%d" % j for j in range(self.i_max)])

    @torch.no_grad()
    def mark_dividends(self, *args, **kwargs):
        """mark_shapley(..., return_coalitions=True) with the same arguments, then shapley_dividends -> (div, info) as pcre_dividends;
        info is mark_shapley's (logits, erased, players, delta, coalitions) plus phi, mass, names and sets."""
        phi, info = self.mark_shapley(*args, **dict(kwargs, return_coalitions=True))
        return self._dividends_info(phi, info, info["players"])

    @torch.no_grad()
    def mark_donor_dividends(self, *args, **kwargs):
        """mark_donor_shapley(..., return_coalitions=True) with the same arguments, then shapley_dividends -> (div, info) as
        mark_dividends; the absent key is "donor"."""
        phi, info = self.mark_donor_shapley(*args, **dict(kwargs, return_coalitions=True))
        return self._dividends_info(phi, info, info["players"])

    @torch.no_grad()
    def mark_window_dividends(self, *args, **kwargs):
        """mark_window_shapley(..., return_coalitions=True) with the same arguments (at most 16 window players), then
        shapley_dividends -> (div, info) as mark_dividends."""
        phi, info = self.mark_window_shapley(*args, **dict(kwargs, return_coalitions=True))
        return self._dividends_info(phi, info, info["players"])

    @torch.no_grad()
    def mark_fine_window_dividends(self, *args, **kwargs):
        """mark_fine_window_shapley(..., return_coalitions=True) with the same arguments (at most 16 fine window players), then
        shapley_dividends -> (div, info) as mark_dividends."""
        phi, info = self.mark_fine_window_shapley(*args, **dict(kwargs, return_coalitions=True))
        return self._dividends_info(phi, info, info["players"])

    @torch.no_grad()
    def pcre_epistasis(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                       interaction_freq=None):
        """Pair-deletion epistasis of the pCRE slots (cf_pcre_epistasis) -> (eps, info), tensors on the model's device, no autograd graph.
        With v(...) the logits after deleting the named slots from the full gene:

          eps[:, i, j]    [B, i_max, i_max, n_out]: ((v() - v(i)) - v(j)) + v(i, j) for i != j, exactly symmetric: 0 when the two
                          deletions add up, non-zero when the pCREs are redundant or cooperate; eps[:, i, i] = v() - v(i), the
                          leave-one-out effect; rows and columns of dummy slots are exactly 0
          info["logits"]  [B, n_out]: v(), the prediction;  info["single"]  [B, i_max, n_out]: v(i)

        The 1 + i_max + i_max (i_max - 1) / 2 rows (attribution.coalition_table("pairs", i_max)) run from one trunk pass.  The first
        argument may also be a packed batch (an engine.Slot or a pack_batch result), with nothing after it.  The pass overwrites the
        activations a grad-enabled model(...) keeps for its backward: such a pending backward() raises."""
        batch = (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq)
        return self._game("pcre_epistasis", "pcre", "epistasis", batch)

    @torch.no_grad()
    def integrated_gradients(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                             interaction_freq=None, target=None, n_steps=50, method="gausslegendre", baselines=None,
                             inputs=("promoter_feats", "pcre_feats", "interaction_freq"), path="linear", donor=None):
        """Integrated gradients of logit column `target` (default: 1 for the classifier, 0 for the regressor) with respect to the float
        inputs named in `inputs` (cf_integrated_gradients) -> (attr, info), tensors on the model's device, no autograd graph:

          attr["promoter_feats"][b], attr["pcre_feats"][b], attr["interaction_freq"]   the caller's shapes (inputs not named: absent)
          info["logits"], info["baseline_logits"]   [B, n_out]: the forward of x and of the baseline
          info["delta"]                             [B]: sum of a gene's attributions - (logits - baseline_logits)[:, target]

        With nodes a_k and weights w_k of chromoformer_amd.attribution.ig_quadrature(method, n_steps): x_k = xb + a_k (x - xb),
        g_k = d(w_k logits[:, target]) / d x_k, attr = (x - xb) * (g_0 + g_1 + ... + g_{n-1}) -- what a hand-written loop of
        grad-enabled model(...) calls and backward()s gives, bit for bit.  `baselines`: None (zeros, the binned value of an empty
        signal) or a dict with some of the three keys ({binsize: tensor} for the features), each with a leading dimension of B or 1.
        Masks are never interpolated.  The first argument may also be a packed batch (an engine.Slot or a pack_batch result), with
        nothing after it.  Parameter gradients and optimiser state are left as they are; the pass overwrites the activations a
        grad-enabled model(...) keeps for its backward: such a pending backward() raises.

        path="signal" (cf_integrated_gradients_raw): the features are u = log(1 + m), m the mean of a bin of the raw signal, and the
        path is a * m from the empty signal -- straight in the raw signal, curved in the features: u_k = log1p(a_k expm1(u)),
        C = sum_k g_k / (1 + a_k m).  attr of the features is m * C, integrated gradients with respect to the bin means (still
        complete: delta as above), and info gains "coeff": {"promoter_feats": {b: ...}, "pcre_feats": {b: ...}} = (1 + m) * C, the dfeat
        that cf_bin_regions_multi_backward(times_input = 1) turns into per-sample attributions (attribution.raw_integrated_gradients).
        interaction_freq, if named, keeps its straight path and baseline.  `inputs` must name a feature input; a feature baseline
        raises ValueError (zero signal only); features must stay below ~80 (expm1 in fp32).

        path="signal" with donor=(donor_promoter_feats, donor_pcre_feats) (cf_integrated_gradients_raw_donor): the baseline is the same
        genes' binned signal in another cell type, in any form mark_donor_shapley's `donor` takes, and the path is the straight line
        xd + a (x - xd) between the two RAW signals: with m, md the bin means of the two, u_k = log1p(md + a_k (m - md)),
        C = sum_k g_k / (1 + md + a_k (m - md)), attr = (m - md) * C.  info["baseline_logits"] is the donor's features under the gene's
        masks and frequencies, info["cmean"] (in place of "coeff") = C per bin, which cf_bin_spread_difference spreads over the
        difference of the two raw signals.  An element with the same bits in both gets exactly 0; a donor of zeros gives the bits of
        the call without donor.  donor= with path="linear", or together with a feature baseline, raises ValueError."""
        if path not in ("linear", "signal"):
            raise ValueError("integrated_gradients: path %r; choose 'linear' or 'signal'" % (path,))
        signal = path == "signal"
        if donor is not None:      # (before anything touches the device)
            if not signal:
                raise ValueError("integrated_gradients: donor= is the baseline of path='signal' (a path between two raw signals); "
                                 "path='linear' takes feature baselines in baselines=")
            given = [k for k in ("promoter_feats", "pcre_feats") if (baselines or {}).get(k) is not None]
            if given:
                raise ValueError("integrated_gradients: donor= and a baseline for %s: the donor is the feature baseline" % given)
            named = (inputs,) if isinstance(inputs, str) else tuple(inputs)
            if not set(named) & {"promoter_feats", "pcre_feats"}:
                raise ValueError("integrated_gradients: path='signal' needs promoter_feats or pcre_feats in inputs, got %s" % (named,))
        elif signal:
            named = (inputs,) if isinstance(inputs, str) else tuple(inputs)
            given = [k for k in ("promoter_feats", "pcre_feats") if (baselines or {}).get(k) is not None]
            if given:
                raise ValueError("integrated_gradients: path='signal' starts at the zero signal; a baseline for %s is not accepted" % given)
            if not set(named) & {"promoter_feats", "pcre_feats"}:
                raise ValueError("integrated_gradients: path='signal' needs promoter_feats or pcre_feats in inputs, got %s" % (named,))
        bs, book = self._attrib_call("integrated_gradients", promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks,
                                     interaction_freq)
        shapes = None
        if promoter_pad_masks is not None:      # (given tensors: the attributions come back in the callers' shapes)
            shapes = {"promoter_feats": {b: promoter_feats[b].shape for b in self.binsizes},
                      "pcre_feats": {b: pcre_feats[b].shape for b in self.binsizes}, "interaction_freq": interaction_freq.shape}
        inputs = (inputs,) if isinstance(inputs, str) else tuple(inputs)
        bad = [k for k in inputs if k not in A.INPUTS]
        if bad or not inputs:
            raise ValueError("integrated_gradients: inputs %s; choose a non-empty subset of %s" % (bad or "()", A.INPUTS))
        target = (1 if self.n_out == 2 else 0) if target is None else int(target)
        alphas, weights = A.ig_quadrature(method, n_steps)
        B, S, T, F, dev = bs.B, self.i_max, self.i_max + 1, self.n_feats, self._device
        canon = {"promoter_feats": {b: (B, L, F) for b, L in zip(self.binsizes, self.n_bins)},
                 "pcre_feats": {b: (B, S, L, F) for b, L in zip(self.binsizes, self.n_bins)}, "interaction_freq": (B, T, T)}
        opts = _lib.cf_ig_opts()
        opts.n_steps, opts.target = len(alphas), target
        opts.interpolate = sum(bit for k, bit in zip(A.INPUTS, (_lib.IG_PROMOTER, _lib.IG_PCRE, _lib.IG_FREQ)) if k in inputs)
        opts.alphas, opts.weights = alphas.ctypes.data, weights.ctypes.data
        keep = []
        baselines = baselines or {}
        extra = [k for k in baselines if k not in A.INPUTS]
        if extra:
            raise ValueError("integrated_gradients: unknown baseline(s) %s; keys are %s" % (extra, A.INPUTS))
        unused = [k for k in baselines if baselines[k] is not None and k not in inputs]
        if unused:
            raise ValueError("integrated_gradients: baseline(s) given for %s, which are not in inputs=%s" % (unused, inputs))
        leads = set()
        for k in inputs:
            if baselines.get(k) is None:
                continue
            for t in (baselines[k].values() if isinstance(baselines[k], dict) else [baselines[k]]):
                leads.add(t.shape[0])
        if leads - {1, B}:
            raise ValueError("integrated_gradients: baselines need a leading dimension of B = %d or 1, got %s" % (B, sorted(leads)))
        bcast = leads == {1}

        def base(t, shape):
            n = 1 if bcast else B
            t = t.to(dev, torch.float32)
            if t.numel() != n * int(np.prod(shape[1:])):
                t = t.expand(B, *t.shape[1:]) if t.shape[0] == 1 else t
                if t.numel() != n * int(np.prod(shape[1:])):
                    raise ValueError("integrated_gradients: a baseline of %d elements does not match the input's shape %s" % (t.numel(), tuple(shape)))
            t = t.contiguous()
            keep.append(t)
            return t.data_ptr()

        for r, b in enumerate(self.binsizes):
            if "promoter_feats" in inputs and baselines.get("promoter_feats") is not None:
                opts.base_promoter_feats[r] = base(baselines["promoter_feats"][b], canon["promoter_feats"][b])
            if "pcre_feats" in inputs and baselines.get("pcre_feats") is not None:
                opts.base_pcre_feats[r] = base(baselines["pcre_feats"][b], canon["pcre_feats"][b])
        if "interaction_freq" in inputs and baselines.get("interaction_freq") is not None:
            opts.base_interaction_freq = base(baselines["interaction_freq"], canon["interaction_freq"])
        opts.base_broadcast = 1 if bcast else 0
        if donor is not None:
            if bcast:
                raise ValueError("integrated_gradients: donor= holds one row per gene; a broadcast baseline (leading dimension 1) cannot go with it")
            dn = _lib.cf_mark_donor_opts()
            keep.append(self._donor_feats("integrated_gradients", donor, B, dn))
            for r in range(len(self.binsizes)):
                if "promoter_feats" in inputs:
                    opts.base_promoter_feats[r] = dn.donor_promoter_feats[r]
                if "pcre_feats" in inputs:
                    opts.base_pcre_feats[r] = dn.donor_pcre_feats[r]
        out = _lib.cf_input_grads()
        attr = {}
        for r, b in enumerate(self.binsizes):
            for k, field in (("promoter_feats", out.promoter_feats), ("pcre_feats", out.pcre_feats)):
                if k in inputs:
                    t = attr.setdefault(k, {})[b] = torch.empty(canon[k][b], device=dev)      # (written in full by the library)
                    field[r] = t.data_ptr()
        if "interaction_freq" in inputs:
            t = attr["interaction_freq"] = torch.empty(canon["interaction_freq"], device=dev)
            out.interaction_freq = t.data_ptr()
        lx = torch.empty(B, self.n_out, device=dev)
        lb = torch.empty(B, self.n_out, device=dev)
        delta = torch.empty(B, device=dev)
        st = book()
        info = {"logits": lx, "baseline_logits": lb, "delta": delta}
        if signal:
            co = _lib.cf_input_grads()
            second = "cmean" if donor is not None else "coeff"
            coeff = info[second] = {}
            for r, b in enumerate(self.binsizes):
                for k, field in (("promoter_feats", co.promoter_feats), ("pcre_feats", co.pcre_feats)):
                    if k in inputs:
                        t = coeff.setdefault(k, {})[b] = torch.empty(canon[k][b], device=dev)      # (written in full by the library)
                        field[r] = t.data_ptr()
            if donor is not None:
                _lib.check(_lib.lib().cf_integrated_gradients_raw_donor(self._handle, C.byref(bs), C.byref(opts), C.byref(out), C.byref(co),
                                                                        lx.data_ptr(), lb.data_ptr(), delta.data_ptr(), st),
                           "cf_integrated_gradients_raw_donor")
            else:
                _lib.check(_lib.lib().cf_integrated_gradients_raw(self._handle, C.byref(bs), C.byref(opts), C.byref(out), C.byref(co), lx.data_ptr(),
                                                                  lb.data_ptr(), delta.data_ptr(), st), "cf_integrated_gradients_raw")
        else:
            _lib.check(_lib.lib().cf_integrated_gradients(self._handle, C.byref(bs), C.byref(opts), C.byref(out), lx.data_ptr(), lb.data_ptr(),
                                                          delta.data_ptr(), st), "cf_integrated_gradients")
        if shapes is not None:
            attr = {k: ({b: t.view(shapes[k][b]) for b, t in v.items()} if isinstance(v, dict) else v.view(shapes[k])) for k, v in attr.items()}
            if signal:
                info[second] = {k: {b: t.view(shapes[k][b]) for b, t in v.items()} for k, v in info[second].items()}
        return attr, info

    def _scan_mark_bits(self, who, mark_sets):
        """mark_sets (None: attribution.scan_mark_sets' default) validated -> uint32 [n_sets], bit f of word k set where set k holds mark f."""
        F = self.n_feats
        mark_sets = A.scan_mark_sets(mark_sets, F)
        bad = [ms for ms in mark_sets if any(not 0 <= f < min(F, 32) for f in ms)]
        if bad or not mark_sets:
            raise ValueError("%s: mark_sets %s: a non-empty list of sets of mark indices in [0, n_feats = %d)" % (who, bad or "()", F))
        return np.array([sum(1 << f for f in set(ms)) for ms in mark_sets], dtype=np.uint32)

    def _set_flip(self, who, opts, flip, B):
        """flip ([B] bools, or None) as opts.flip -> what it points to, to be kept alive until the call has been issued: a uint8 tensor
        of B entries on the model's device, or None."""
        if flip is None:
            return None
        flip = torch.as_tensor(flip).to(self._device).ne(0).to(torch.uint8).contiguous()
        if flip.numel() != B:
            raise ValueError("%s: flip has %d entries for a batch of %d genes" % (who, flip.numel(), B))
        opts.flip = flip.data_ptr()
        return flip

    def _feats_out(self, opts, B, rows):
        """feats_out of a scan or a fine game of `rows` rows per gene, attached to its options -> {binsize: [B, rows, n_bins, n_feats]}."""
        feats = {}
        for r, b in enumerate(self.binsizes):
            t = feats[b] = torch.empty(B, rows, self.n_bins[r], self.n_feats, device=self._device)      # (written in full by the library)
            opts.feats_out[r] = t.data_ptr()
        return feats

    def _fine_args(self, who, opts, B, start, lengths, n_windows, step):
        """What the fine scan and the fine game share: start (an int or B ints) and lengths (B ints or None) as opts.start and
        opts.lengths -> (n_windows, by default the windows `step` finest bins apart that reach the end of the region from the smallest
        start; what opts points to)."""
        Lf = self.n_bins[min(range(len(self.binsizes)), key=lambda r: self.binsizes[r])]
        start = np.asarray(start, dtype=np.int64).reshape(-1)
        if start.size == 1:
            start = np.repeat(start, B)
        if start.size != B:
            raise ValueError("%s: start has %d entries for a batch of %d genes" % (who, start.size, B))
        if start.size and (start.min() < -2 ** 31 or start.max() >= 2 ** 31):
            raise ValueError("%s: start does not fit an int" % who)
        start = start.astype(np.int32)
        if n_windows is None:
            first = max(int(start.min()), 0) if B else 0
            n_windows = max(-(-(Lf - first) // max(step, 1)), 1)
        opts.start = start.ctypes.data
        if lengths is not None:
            lengths = np.ascontiguousarray(np.asarray(lengths, dtype=np.int64).reshape(-1))
            if lengths.size != B:
                raise ValueError("%s: lengths has %d entries for a batch of %d genes" % (who, lengths.size, B))
            lengths = np.clip(lengths, -1, 2 ** 31 - 1).astype(np.int32)      # (out of range either way: refused by the library)
            opts.lengths = lengths.ctypes.data
        return n_windows, (start, lengths)

    @torch.no_grad()
    def perturbation_scan(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                          interaction_freq=None, region=0, scale=0.0, width=1, mark_sets=None, flip=None, return_feats=False):
        """In-silico perturbation scan (cf_perturbation_scan): the prediction with the histone marks of a mark set scaled by `scale`
        (0 erases, 2 doubles) in RAW-SIGNAL space over a window of one region -- the promoter (region 0) or pCRE slot j (region
        1 + j) -- for every window and every mark set, from one call -> logits [B, V, n_out] on the model's device, no autograd graph.
        With W = min(n_bins), the bins of the coarsest resolution, V = 1 + n_sets * W:

          [:, 0]                the prediction (model(...) under no_grad, bit-equal)
          [:, 1 + k * W + g]    mark set k over window g: the coarse genomic bins [g, g + width) of the region and the finer bins inside
                                them; a covered feature u = log(1 + mean) becomes log1p(scale * expm1(u)), exactly what binning the
                                scaled signal gives.  Windows past the region's real bins (a short pCRE, a dummy slot, a narrowed
                                promoter) and empty mark sets give [:, 0], bit for bit.

        mark_sets: iterables of mark indices; default each mark alone, then all marks together (n_feats + 1 sets).  flip: [B] bools,
        True where the region is stored mirrored (the dataset mirrors '-' strand promoters, never pCREs): window g then counts from
        the genomic start.  return_feats: also {binsize: [B, V, n_bins, n_feats]}, the features of the scanned region that row (b, v)
        read.  Features must stay below ~80 (expm1 in fp32).  The first argument may also be a packed batch (an engine.Slot or a
        pack_batch result), with nothing after it.  The pass overwrites the activations a grad-enabled model(...) keeps for its
        backward: such a pending backward() raises."""
        bs, book = self._attrib_call("perturbation_scan", promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks,
                                     interaction_freq)
        bits = self._scan_mark_bits("perturbation_scan", mark_sets)
        V = 1 + len(bits) * min(self.n_bins)
        opts = _lib.cf_scan_opts()
        opts.region, opts.width, opts.n_sets, opts.scale = int(region), int(width), len(bits), float(scale)
        opts.mark_sets = bits.ctypes.data
        flip = self._set_flip("perturbation_scan", opts, flip, bs.B)
        feats = self._feats_out(opts, bs.B, V) if return_feats else None
        logits = torch.empty(bs.B, V, self.n_out, device=self._device)      # (written in full by the library)
        st = book()
        _lib.check(_lib.lib().cf_perturbation_scan(self._handle, C.byref(bs), C.byref(opts), logits.data_ptr(), st), "cf_perturbation_scan")
        return (logits, feats) if return_feats else logits

    @torch.no_grad()
    def perturbation_scan_regions(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                                  interaction_freq=None, regions="all", scale=0.0, width=1, mark_sets=None, flip=None):
        """perturbation_scan of several regions from one call (cf_perturbation_scan_regions) -> (logits [n_reg, B, V, n_out] on the
        model's device, the list of scanned regions in block order).  regions: "all" (0 .. i_max), "pcres" (1 .. i_max) or an iterable
        of region indices (0 the promoter, 1 + j pCRE slot j; sorted, duplicates dropped).  Block q carries the bits of
        perturbation_scan(region=regions[q]) with the same scale, width and mark_sets -- `flip` applies to the promoter block alone
        (pCREs are never stored mirrored).  The promoter block costs what perturbation_scan costs; the variants of a pCRE slot run
        slot-packed: i_max variants share one pass of the Embedding + Pairwise stage, and only the Regulation stack and the head run
        per variant.  mark_sets, the packed forms of the first argument and the effect on a pending backward() are those of
        perturbation_scan; there is no return_feats."""
        bs, book = self._attrib_call("perturbation_scan_regions", promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks,
                                     interaction_freq)
        regions = A.scan_regions_expand(regions, self.i_max, "perturbation_scan_regions")
        bits = self._scan_mark_bits("perturbation_scan_regions", mark_sets)
        V = 1 + len(bits) * min(self.n_bins)
        opts = _lib.cf_scan_regions_opts()
        opts.regions = sum(1 << r for r in regions)
        opts.width, opts.n_sets, opts.scale = int(width), len(bits), float(scale)
        opts.mark_sets = bits.ctypes.data
        flip = self._set_flip("perturbation_scan_regions", opts, flip, bs.B)
        logits = torch.empty(len(regions), bs.B, V, self.n_out, device=self._device)      # (written in full by the library)
        st = book()
        _lib.check(_lib.lib().cf_perturbation_scan_regions(self._handle, C.byref(bs), C.byref(opts), logits.data_ptr(), st),
                   "cf_perturbation_scan_regions")
        return logits, regions

    @torch.no_grad()
    def perturbation_scan_fine(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                               interaction_freq=None, region=0, scale=0.0, width=1, stride=None, start=0, n_windows=None, mark_sets=None,
                               lengths=None, flip=None, return_feats=False):
        """perturbation_scan with windows in bins of the FINEST resolution (cf_perturbation_scan_fine) -> logits [B, V, n_out] on the
        model's device, no autograd graph; V = 1 + n_sets * n_windows:

          [:, 0]                        the prediction (model(...) under no_grad, bit-equal)
          [:, 1 + k * n_windows + g]    mark set k over the finest genomic bins [start[b] + g * stride, start[b] + g * stride + width) of
                                        the region.  A coarser bin the window covers wholly follows perturbation_scan's rule; one it
                                        covers in part is recomputed from its finest children, weighted by their sample counts -- what
                                        binning the scaled signal gives, up to the rounding of the stored features.  Windows past the
                                        region's real bins and empty mark sets give [:, 0], bit for bit.

        width, stride (default: width) in finest bins; start: an int or B ints, the first finest genomic bin per gene (zoom into a
        different coarse window per gene); n_windows: default the windows that reach the end of the region from the smallest start.
        lengths: B ints, the scanned region's length in samples, so that the short last bin of a region is weighted by what it holds
        (None: every real finest bin is full -- exact for promoters and whenever the length is a multiple of the finest bin size;
        giving it costs one read-back of the pad-mask rows and a stream synchronisation).  mark_sets, flip, return_feats, the packed
        forms of the first argument and the effect on a pending backward() are those of perturbation_scan."""
        who = "perturbation_scan_fine"
        bs, book = self._attrib_call(who, promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq)
        bits = self._scan_mark_bits(who, mark_sets)
        opts = _lib.cf_scan_fine_opts()
        opts.width = int(width)
        opts.stride = opts.width if stride is None else int(stride)
        n_windows, _alive = self._fine_args(who, opts, bs.B, start, lengths, n_windows, opts.stride)
        opts.n_windows = int(n_windows)
        V = 1 + len(bits) * max(opts.n_windows, 0)
        opts.region, opts.n_sets, opts.scale = int(region), len(bits), float(scale)
        opts.mark_sets = bits.ctypes.data
        flip = self._set_flip(who, opts, flip, bs.B)
        feats = self._feats_out(opts, bs.B, V) if return_feats else None
        logits = torch.empty(bs.B, V, self.n_out, device=self._device)      # (written in full by the library)
        st = book()
        _lib.check(_lib.lib().cf_perturbation_scan_fine(self._handle, C.byref(bs), C.byref(opts), logits.data_ptr(), st), "cf_perturbation_scan_fine")
        return (logits, feats) if return_feats else logits

    def perturbation_scan_fine_dataset(self, dataset, genes=None, region="promoter", zoom=None, scale=0.0, width=1, stride=None, mark_sets=None,
                                       target=None, bsz=None, store=None):
        """perturbation_scan_fine over the genes of a ChromoformerDataset with windows in genomic coordinates
        (chromoformer_amd.attribution.perturbation_scan_fine, a generator of per-gene dicts)."""
        return A.perturbation_scan_fine(self, dataset, genes=genes, region=region, zoom=zoom, scale=scale, width=width, stride=stride,
                                        mark_sets=mark_sets, target=target, bsz=bsz, store=store)

    def perturbation_scan_dataset(self, dataset, genes=None, regions="promoter", scale=0.0, width=1, mark_sets=None, bsz=None, store=None):
        """perturbation_scan over the genes of a ChromoformerDataset with windows in genomic coordinates
        (chromoformer_amd.attribution.perturbation_scan, a generator of per-gene dicts)."""
        return A.perturbation_scan(self, dataset, genes=genes, regions=regions, scale=scale, width=width, mark_sets=mark_sets, bsz=bsz, store=store)

    def _permutations(self, who, P, n_perm, seed, permutations):
        """The orders of a sampled game of P players -> uint8 [n_perm, P]: shapley_permutations, or `permutations` checked."""
        if permutations is None:
            return A.shapley_permutations(P, n_perm, seed)
        given = np.asarray(permutations.cpu() if hasattr(permutations, "cpu") else permutations)
        if given.ndim != 2 or given.shape[0] < 1 or given.shape[1] != P or given.dtype.kind not in "iu" or given.min() < 0 or given.max() >= P:
            raise ValueError("%s: permutations must be an integer array [n_perm >= 1, P = %d] with entries in [0, P)" % (who, P))
        return np.ascontiguousarray(given, dtype=np.uint8)

    @torch.no_grad()
    def perm_interactions_from_rows(self, rows, permutations, focal, index="sii"):
        """The reducers of the sampled interactions calls on a table (cf_perm_interactions_from_rows) -> (inter, stderr, phi,
        phi_stderr).  rows: a float32 tensor [B, R, n] on the model's device in the layout of attribution.focal_words(permutations,
        focal) (any n >= 1); permutations: integer [n_perm, P], 2 <= P <= 128; focal: distinct player indices.  inter, stderr
        [B, n_focal, P, n]; phi, phi_stderr [B, P, n].  No forward runs and no activation is written."""
        who = "perm_interactions_from_rows"
        code = A.interaction_index(index, who)
        if self._handle is None:
            raise RuntimeError("call .cuda() first: the Chromoformer HIP path needs device buffers")
        perms = np.ascontiguousarray(np.asarray(permutations.cpu() if hasattr(permutations, "cpu") else permutations))
        if perms.ndim != 2 or perms.dtype.kind not in "iu" or not 2 <= perms.shape[1] <= 128 or perms.min() < 0 or perms.max() >= perms.shape[1]:
            raise ValueError("%s: permutations must be an integer array [n_perm >= 1, 2 <= P <= 128] with entries in [0, P)" % who)
        perms = np.ascontiguousarray(perms, dtype=np.uint8)
        n, P = perms.shape
        focal = A.focal_players(focal, None, P)
        R = A.focal_row_count(perms, focal)
        if not torch.is_tensor(rows) or rows.dtype != torch.float32 or rows.dim() != 3 or rows.shape[1] != R or rows.device != self._device:
            raise ValueError("%s: rows must be a float32 tensor [B, R = %d, n] on %s" % (who, R, self._device))
        rows = rows.contiguous()
        B, n_out, F, dev = rows.shape[0], rows.shape[2], len(focal), self._device
        inter, se = torch.empty(B, F, P, n_out, device=dev), torch.empty(B, F, P, n_out, device=dev)
        phi, phi_se = torch.empty(B, P, n_out, device=dev), torch.empty(B, P, n_out, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(_lib.lib().cf_perm_interactions_from_rows(self._handle, rows.data_ptr(), B, P, n_out, perms.ctypes.data, n, focal.ctypes.data, F,
                                                             code, inter.data_ptr(), se.data_ptr(), phi.data_ptr(), phi_se.data_ptr(), st),
                   "cf_perm_interactions_from_rows")
        return inter, se, phi, phi_se

    @torch.no_grad()
    def mark_coalitions(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                        interaction_freq=None, keep=None, players="marks", scale=0.0):
        """The prediction under histone-mark coalitions (cf_mark_coalitions) -> logits [B, n_coal, n_out] on the model's device, no
        autograd graph.  The players are marks, each optionally restricted to regions (attribution.mark_players: "marks",
        "compartments", "regions" or a list of (marks, regions) pairs).  `keep`: a sequence / array of ints, bit p set = player p
        present, or a bool array [n_coal, P].  Column c is the inference forward with the raw signal of every ABSENT player's marks
        scaled by `scale` (0 erases, the default) over the player's regions: a feature u = log(1 + mean) becomes
        log1p(scale * expm1(u)), exactly what binning the scaled signal gives; an element covered by several absent players is scaled
        once.  The full word 2^P - 1 is the prediction (model(...) under no_grad, bit-equal).  Features must stay below ~80 (expm1 in
        fp32).  The first argument may also be a packed batch (an engine.Slot or a pack_batch result), with nothing after it.  The
        pass overwrites the activations a grad-enabled model(...) keeps for its backward: such a pending backward() raises."""
        batch = (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq)
        return self._game("mark_coalitions", "mark", "coalitions", batch, keep=keep, players=players, scale=scale)

    @torch.no_grad()
    def mark_shapley(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                     interaction_freq=None, players="marks", scale=0.0, return_coalitions=False):
        """Exact Shapley values of the histone marks (cf_mark_shapley) -> (phi, info), tensors on the model's device, no autograd graph:

          phi                 [B, P, n_out]: player p's average marginal contribution to each logit over all orders of adding the
                              players to the gene with every player absent; exactly 0 for a player whose elements are all zeros
          info["logits"]      [B, n_out]: the prediction (every player present; model(...) under no_grad, bit-equal)
          info["erased"]      [B, n_out]: every player absent
          info["delta"]       [B, n_out]: phi.sum(1) - (logits - erased), the efficiency gap (rounding only)
          info["players"]     the players' names
          info["coalitions"]  [B, 2^P, n_out], with return_coalitions: the logits of every coalition, word m at column m

        players and scale as in mark_coalitions; all 2^P coalitions (128 for the seven marks) run from one call, in logit space, where
        efficiency holds.  The packed forms of the first argument and the effect on a pending backward() are those of mark_coalitions."""
        batch = (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq)
        return self._game("mark_shapley", "mark", "shapley", batch, players=players, scale=scale, table=return_coalitions)

    @torch.no_grad()
    def mark_epistasis(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                       interaction_freq=None, players="marks", scale=0.0):
        """Pair epistasis of the histone-mark players (cf_mark_epistasis) -> (eps, info), tensors on the model's device, no autograd
        graph.  With v(...) the logits with the named players absent:

          eps[:, i, j]    [B, P, P, n_out]: ((v() - v(i)) - v(j)) + v(i, j) for i != j, exactly symmetric: 0 when the two marks add
                          up, non-zero when they are redundant or cooperate; eps[:, i, i] = v() - v(i), the leave-one-out effect
          info["logits"]  [B, n_out]: v(), the prediction;  info["single"]  [B, P, n_out]: v(i);  info["players"]  the names

        The 1 + P + P (P - 1) / 2 rows (attribution.coalition_table("pairs", P)) run from one call.  players, scale, the packed forms
        of the first argument and the effect on a pending backward() are those of mark_coalitions."""
        batch = (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq)
        return self._game("mark_epistasis", "mark", "epistasis", batch, players=players, scale=scale)

    @torch.no_grad()
    def mark_shapley_interactions(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                                  interaction_freq=None, players="marks", scale=0.0, index="sii", return_coalitions=False):
        """Pairwise Shapley interaction indices of the histone-mark players (cf_mark_shapley_interactions) -> (inter, info), tensors on
        the model's device, no autograd graph.  At least 2 players; the 2^P coalitions run once, as in mark_shapley:

          %(inter)s
        players and scale as in mark_coalitions.  The packed forms of the first argument and the effect on a pending backward() are
        those of mark_coalitions."""
        batch = (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq)
        return self._game("mark_shapley_interactions", "mark", "shapley_interactions", batch, players=players, scale=scale, index=index,
                          table=return_coalitions)

    def _donor_freq(self, who, opts, donor_freq, B):
        """The donor rule of the contact games: donor_freq (None: the scale rule) checked, its pointer written into opts.donor_freq ->
        what it points to.  A contiguous float32 tensor [B, T, T] (or [B, 1, T, T]) on the model's device, T = i_max + 1."""
        if donor_freq is None:
            return ()
        T, t = self.i_max + 1, donor_freq
        what = "%s: donor_freq" % who
        if not torch.is_tensor(t):
            raise ValueError("%s is not a tensor" % what)
        if t.dtype != torch.float32:
            raise ValueError("%s is %s; the donor's bits are taken as they are: float32 is required" % (what, t.dtype))
        if t.device != self._device:
            raise ValueError("%s is on %s, the model on %s" % (what, t.device, self._device))
        if t.numel() != B * T * T or t.dim() < 3 or t.shape[0] != B or tuple(t.shape[-2:]) != (T, T):
            raise ValueError("%s has shape %s; expected %s" % (what, tuple(t.shape), (B, T, T)))
        if not t.is_contiguous():
            raise ValueError("%s is not contiguous" % what)
        opts.donor_freq = t.data_ptr()
        return (t,)

    def mark_shapley_dataset(self, dataset, genes=None, players="marks", scale=0.0, epistasis=False, bsz=None, store=None, interactions=None,
                             dividends=False):
        """mark_shapley (and optionally mark_epistasis, or mark_shapley_interactions in its place; with dividends=True the Harsanyi
        dividends of the same table too) over the genes of a ChromoformerDataset (chromoformer_amd.attribution.mark_shapley, a generator
        of per-gene dicts)."""
        return A.mark_shapley(self, dataset, genes=genes, players=players, scale=scale, epistasis=epistasis, bsz=bsz, store=store,
                              interactions=interactions, dividends=dividends)

    def _donor_feats(self, who, donor, B, opts):
        """The donor of a batch of B genes checked, its feature pointers written into opts.donor_promoter_feats / donor_pcre_feats ->
        what they point to.  donor: a (promoter_feats, pcre_feats) pair of dicts by bin size (or lists in binsizes order) of contiguous
        float32 tensors on the model's device, [B, 1, L, F] and [B, i_max, L, F]; or a packed batch (an engine.Slot, a pack_batch result
        or a batch struct), whose features are used and the rest ignored.  Anything else raises ValueError naming `who`."""
        if donor is None:
            raise ValueError("%s: donor is required: the same genes' features in the other cell type, a (promoter_feats, pcre_feats) "
                             "pair or a packed batch" % who)
        S, F = self.i_max, self.n_feats
        packed = donor if isinstance(donor, _lib.cf_batch) else getattr(donor, "struct", None)
        if packed is None and isinstance(donor, (tuple, list)) and len(donor) == 2 and isinstance(donor[0], _lib.cf_batch):
            packed = donor[0]
        if packed is not None:
            if packed.B != B:
                raise ValueError("%s: the donor holds %d genes, the batch %d" % (who, packed.B, B))
            for r in range(len(self.binsizes)):
                opts.donor_promoter_feats[r], opts.donor_pcre_feats[r] = packed.promoter_feats[r], packed.pcre_feats[r]
            return (donor,)
        try:
            pfs, cfs = donor
            pfs = [pfs[b] for b in self.binsizes] if isinstance(pfs, dict) else list(pfs)
            cfs = [cfs[b] for b in self.binsizes] if isinstance(cfs, dict) else list(cfs)
        except (TypeError, ValueError, KeyError):
            raise ValueError("%s: donor must be a (promoter_feats, pcre_feats) pair of dicts by bin size %s (or lists in that order) or a "
                             "packed batch" % (who, list(self.binsizes))) from None
        if len(pfs) != len(self.binsizes) or len(cfs) != len(self.binsizes):
            raise ValueError("%s: donor has %d / %d feature tensors, the model %d resolutions" % (who, len(pfs), len(cfs), len(self.binsizes)))
        for r, b in enumerate(self.binsizes):
            L = self.n_bins[r]
            for name, t, lead in (("promoter_feats", pfs[r], 1), ("pcre_feats", cfs[r], S)):
                what = "%s: donor %s[%d]" % (who, name, b)
                if not torch.is_tensor(t):
                    raise ValueError("%s is not a tensor" % what)
                if t.dtype != torch.float32:
                    raise ValueError("%s is %s; the donor's bits are selected as they are: float32 is required" % (what, t.dtype))
                if t.device != self._device:
                    raise ValueError("%s is on %s, the model on %s" % (what, t.device, self._device))
                if t.numel() != B * lead * L * F or t.dim() < 3 or t.shape[0] != B or tuple(t.shape[-2:]) != (L, F):
                    raise ValueError("%s has shape %s; expected %s" % (what, tuple(t.shape), (B, lead, L, F)))
                if not t.is_contiguous():
                    raise ValueError("%s is not contiguous" % what)
            opts.donor_promoter_feats[r], opts.donor_pcre_feats[r] = pfs[r].data_ptr(), cfs[r].data_ptr()
        return (pfs, cfs)

    @torch.no_grad()
    def mark_donor_coalitions(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                              interaction_freq=None, donor=None, keep=None, players="marks"):
        """The prediction under histone-mark coalitions against a donor cell type (cf_mark_donor_coalitions) -> logits
        [B, n_coal, n_out] on the model's device, no autograd graph.  Players and `keep` as in mark_coalitions.  `donor`: the same B
        genes' features in the other cell type -- a (promoter_feats, pcre_feats) pair of dicts by bin size (or lists in binsizes
        order) of contiguous float32 tensors on the model's device, or a packed batch (an engine.Slot or a pack_batch result), whose
        features are used and the rest ignored.  Column c is the inference forward with every ABSENT player's marks taken from the
        donor over the player's regions, bit for bit, at every resolution and in every row; masks and interaction_freq stay the
        gene's own.  Where the two cell types share a region's coordinates this is exactly what binning the raw region with those
        marks' rows replaced gives.  The full word 2^P - 1 is the prediction (model(...) under no_grad, bit-equal).  The first
        argument may also be a packed batch, with nothing after it.  The pass overwrites the activations a grad-enabled model(...)
        keeps for its backward: such a pending backward() raises."""
        batch = (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq)
        return self._game("mark_donor_coalitions", "mark_donor", "coalitions", batch, keep=keep, players=players, donor=donor)

    @torch.no_grad()
    def mark_donor_shapley(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                           interaction_freq=None, donor=None, players="marks", return_coalitions=False):
        """Exact Shapley values of the histone marks against a donor cell type (cf_mark_donor_shapley) -> (phi, info), tensors on the
        model's device, no autograd graph: which mark changes account for the difference between the two predictions?

          phi                 [B, P, n_out]: player p's average marginal contribution to each logit over all orders of switching the
                              players from the donor's signal to the gene's; exactly 0 for a player whose elements are the same in both
          info["logits"]      [B, n_out]: the prediction (every player present; model(...) under no_grad, bit-equal)
          info["donor"]       [B, n_out]: every player absent: the donor's marks under the gene's masks and frequencies
          info["delta"]       [B, n_out]: phi.sum(1) - (logits - donor), the efficiency gap (rounding only)
          info["players"]     the players' names
          info["coalitions"]  [B, 2^P, n_out], with return_coalitions: the logits of every coalition, word m at column m

        donor and players as in mark_donor_coalitions; all 2^P coalitions run from one call.  The packed forms of the first argument
        and the effect on a pending backward() are those of mark_coalitions."""
        batch = (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq)
        return self._game("mark_donor_shapley", "mark_donor", "shapley", batch, players=players, donor=donor, table=return_coalitions)

    @torch.no_grad()
    def mark_donor_epistasis(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                             interaction_freq=None, donor=None, players="marks"):
        """Pair epistasis of the histone-mark players against a donor cell type (cf_mark_donor_epistasis) -> (eps, info) as
        mark_epistasis returns them, with v(...) the logits with the named players' marks taken from the donor.  donor and players as
        in mark_donor_coalitions."""
        batch = (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq)
        return self._game("mark_donor_epistasis", "mark_donor", "epistasis", batch, players=players, donor=donor)

    @torch.no_grad()
    def mark_donor_shapley_interactions(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                                        interaction_freq=None, donor=None, players="marks", index="sii", return_coalitions=False):
        """Pairwise Shapley interaction indices of the histone-mark players against a donor cell type
        (cf_mark_donor_shapley_interactions) -> (inter, info), tensors on the model's device, no autograd graph.  At least 2 players;
        the 2^P coalitions run once, as in mark_donor_shapley:

          %(inter)s
        donor and players as in mark_donor_coalitions; a player whose elements are the same in both cell types is a null player."""
        batch = (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq)
        return self._game("mark_donor_shapley_interactions", "mark_donor", "shapley_interactions", batch, players=players, donor=donor, index=index,
                          table=return_coalitions)

    def mark_donor_shapley_dataset(self, dataset, donor_dataset, genes=None, players="marks", epistasis=False, bsz=None, store=None, donor_store=None,
                                   interactions=None, dividends=False):
        """mark_donor_shapley (and optionally mark_donor_epistasis, the interaction index, the dividends) over the genes of two
        ChromoformerDatasets, the gene's cell type and the donor's (chromoformer_amd.attribution.mark_donor_shapley, a generator of
        per-gene dicts)."""
        return A.mark_donor_shapley(self, dataset, donor_dataset, genes=genes, players=players, epistasis=epistasis, bsz=bsz, store=store,
                                    donor_store=donor_store, interactions=interactions, dividends=dividends)

    @torch.no_grad()
    def mark_coalitions_wide(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                             interaction_freq=None, keep=None, players="cells", scale=0.0, donor=None):
        """The prediction under histone-mark coalitions of up to 128 players (cf_mark_coalitions_wide) -> logits [B, n_coal, n_out] on
        the model's device, no autograd graph.  players: attribution.mark_players_wide -- what mark_coalitions takes, or "cells", one
        player per (mark, region) pair: n_feats (i_max + 1) of them.  `keep`: a bool array [n_coal, P], or a sequence of Python ints
        (bit p set = player p present; attribution.mark_wide_words).  donor None: an ABSENT player's raw signal is scaled by `scale`
        (0 erases) as in mark_coalitions; a donor (the forms of mark_donor_coalitions): its elements take the donor's bits and `scale`
        is not read.  With at most 16 players the rows carry the bits of mark_coalitions / mark_donor_coalitions.  The packed forms
        of the first argument and the effect on a pending backward() are those of mark_coalitions."""
        batch = (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq)
        return self._game("mark_coalitions_wide", "mark_wide", "coalitions", batch, keep=keep, players=players, scale=scale, donor=donor)

    @torch.no_grad()
    def mark_shapley_sampled(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                             interaction_freq=None, players="cells", n_perm=64, seed=0, permutations=None, scale=0.0, donor=None,
                             return_rows=False):
        """Permutation-sampled Shapley values of up to 128 histone-mark players (cf_mark_shapley_sampled) -> (phi, info), tensors on the
        model's device, no autograd graph: which mark matters at which region?

          phi                   [B, P, n_out]: the mean, over the sampled orders of adding the players, of player p's marginal
                                contribution to each logit; exactly 0 for a player whose elements are the same present and absent.
                                With players="cells", phi.view(B, i_max + 1, n_feats, n_out)[:, rho, f] is mark f in region rho
          info["stderr"]        [B, P, n_out]: the standard error of that mean over the orders (0 with one order).  phi is an
                                ESTIMATE: this is the only statement about its sampling error, nothing bounds it
          info["logits"]        [B, n_out]: the prediction (every player present; model(...) under no_grad, bit-equal)
          info["absent"]        [B, n_out]: every player absent (erased, scaled, or the donor's marks)
          info["delta"]         [B, n_out]: phi.sum(1) - (logits - absent), the efficiency gap (rounding only: every order telescopes)
          info["names"]         the players' names
          info["permutations"]  uint8 [n_perm, P]: the orders used
          info["rows"]          [B, 2 + n_perm (P - 1), n_out], with return_rows: nobody, everybody, then per order q its first
                                k = 1 .. P - 1 players at column 2 + q (P - 1) + (k - 1)

        The orders are attribution.shapley_permutations(P, n_perm, seed), or `permutations` (an integer array [n_perm, P], each row a
        permutation; stderr then still assumes independent orders).  players, scale and donor as in mark_coalitions_wide.  The packed
        forms of the first argument and the effect on a pending backward() are those of mark_coalitions."""
        batch = (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq)
        return self._game("mark_shapley_sampled", "mark_wide", "shapley_sampled", batch, players=players, scale=scale, donor=donor,
                          perms=(n_perm, seed, permutations), table=return_rows)

    def mark_shapley_sampled_dataset(self, dataset, donor_dataset=None, genes=None, players="cells", n_perm=64, seed=0, scale=0.0, bsz=None,
                                     store=None, donor_store=None):
        """mark_shapley_sampled over the genes of a ChromoformerDataset, against a donor cell type's dataset if one is given
        (chromoformer_amd.attribution.mark_shapley_sampled, a generator of per-gene dicts)."""
        return A.mark_shapley_sampled(self, dataset, donor_dataset, genes=genes, players=players, n_perm=n_perm, seed=seed, scale=scale, bsz=bsz,
                                      store=store, donor_store=donor_store)

    @torch.no_grad()
    def mark_shapley_interactions_sampled(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None,
                                          interaction_masks=None, interaction_freq=None, players="cells", focal=None, index="sii", n_perm=64,
                                          seed=0, permutations=None, scale=0.0, donor=None, return_rows=False):
        """Permutation-sampled pairwise Shapley interaction indices of a few FOCAL players of up to 128 histone-mark players
        (cf_mark_shapley_interactions_sampled) -> (inter, info), tensors on the model's device, no autograd graph: for the cells that
        carry the prediction (mark_shapley_sampled finds them), which other cells are redundant with them, which cooperate?

          inter                 [B, n_focal, P, n_out]: inter[b, f, j] estimates the interaction index of focal player i = focal[f] with
                                player j -- how much i's marginal contribution changes with j present: per order, with the players
                                that precede j among the others as context, (i's marginal with j) - (i's marginal without j); the mean
                                over the orders.  index "sii": unbiased for the Shapley interaction index; the diagonal j = i is
                                info["phi"][b, i], bit for bit.  index "sti": each sample weighted by 2 (P - 1 - a) / P, a the size of
                                the context: unbiased for Shapley-Taylor of order 2; the diagonal is v({i}) - v(nobody).  Exactly 0
                                where i or j is a null player.  NOT symmetric: inter[b, f, j] from focal i and the entry of focal j at
                                player i are different samples of the same quantity
          info["stderr"]        [B, n_focal, P, n_out]: the standard error of that mean over the orders (0 with one order; 0 on the
                                "sti" diagonal).  inter is an ESTIMATE: this is the only statement about its sampling error
          info["phi"], info["phi_stderr"]   [B, P, n_out]: mark_shapley_sampled's estimate of every player on the same orders, from the
                                same forwards, bit for bit
          info["logits"], info["absent"]    [B, n_out]: everybody present (the prediction), nobody present
          info["alone"], info["without"]    [B, n_focal, n_out]: the focal player alone present; everybody but the focal player
          info["delta"]         [B, n_focal, n_out], "sii": sum_{j != i} inter - ((logits - without) - (alone - absent)), rounding only
                                (every order telescopes); None for "sti"
          info["names"], info["focal"], info["index"], info["permutations"]   the players' names, the focal indices (int32), the index
                                name, the orders (uint8 [n_perm, P])
          info["col"]           uint32 [n_focal, n_perm, P, 2]: the rows the reducer reads (attribution.focal_words)
          info["rows"]          [B, R, n_out], with return_rows: mark_shapley_sampled's table, then the focal players' own rows
                                (attribution.focal_words) -- about as many forwards again as the Shapley estimate per focal player

        focal: player indices or names (attribution.focal_players), distinct.  players, n_perm, seed, permutations, scale and donor as
        in mark_shapley_sampled.  The packed forms of the first argument and the effect on a pending backward() are those of
        mark_coalitions."""
        batch = (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq)
        return self._game("mark_shapley_interactions_sampled", "mark_wide", "shapley_interactions_sampled", batch, players=players, scale=scale,
                          donor=donor, focal=focal, index=index, perms=(n_perm, seed, permutations), table=return_rows)

    def mark_shapley_interactions_sampled_dataset(self, dataset, donor_dataset=None, genes=None, players="cells", top=4, focal=None, index="sii",
                                                  n_perm=64, seed=0, scale=0.0, bsz=None, store=None, donor_store=None):
        """mark_shapley_interactions_sampled over the genes of a ChromoformerDataset, the focal players chosen per gene
        (chromoformer_amd.attribution.mark_shapley_interactions_sampled, a generator of per-gene dicts)."""
        return A.mark_shapley_interactions_sampled(self, dataset, donor_dataset, genes=genes, players=players, top=top, focal=focal, index=index,
                                                   n_perm=n_perm, seed=seed, scale=scale, bsz=bsz, store=store, donor_store=donor_store)

    @torch.no_grad()
    def mark_window_coalitions(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                               interaction_freq=None, keep=None, players="promoter", width=1, scale=0.0, donor=None, flip=None):
        """The prediction under coalitions of WINDOW players (cf_mark_window_coalitions) -> logits [B, n_coal, n_out] on the model's
        device, no autograd graph.  A player is a set of marks in a set of regions over a window of bins of the coarsest resolution
        (attribution.window_players: "promoter", "promoter_cells", "regions" at `width` bins per window, or (marks, regions, (lo, hi))
        triples; at most 128).  `keep` as in mark_coalitions_wide.  Column c is the inference forward with the marks of every ABSENT
        player, inside its window of its regions, scaled by `scale` in raw-signal space (0 erases; donor None) or taken from the donor
        (the forms of mark_donor_coalitions), at every resolution; an element covered by several absent players changes once.  flip:
        [B] bools, True where the promoter is stored mirrored ('-' strand): windows count from the genomic start, as in
        perturbation_scan.  One absent single-region player gives the row of perturbation_scan(width=hi - lo) at window lo, bit for bit; a
        window past a region's real bins changes nothing.  The packed forms of the first argument and the effect on a pending
        backward() are those of mark_coalitions."""
        batch = (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq)
        return self._game("mark_window_coalitions", "mark_window", "coalitions", batch, keep=keep, players=players, width=width, scale=scale,
                          donor=donor, flip=flip)

    @torch.no_grad()
    def mark_window_shapley(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                            interaction_freq=None, players="promoter", width=1, scale=0.0, donor=None, flip=None, return_coalitions=False):
        """Exact Shapley values of at most 16 window players (cf_mark_window_shapley) -> (phi, info), tensors on the model's device, no
        autograd graph: which stretch of the region carries the prediction?  Two redundant stretches share the credit here, where a
        leave-one-out scan scores both near zero.

          phi                 [B, P, n_out]: player p's average marginal contribution over all orders; exactly 0 for a null player
                              (a window past the region's real bins, a dummy slot)
          info["logits"]      [B, n_out]: the prediction (every player present; model(...) under no_grad, bit-equal)
          info["erased"]      [B, n_out]: every player absent (donor None); info["donor"] with a donor
          info["delta"]       [B, n_out]: phi.sum(1) - (logits - erased), the efficiency gap (rounding only)
          info["players"]     the players' names
          info["coalitions"]  [B, 2^P, n_out], with return_coalitions: the logits of every coalition, word m at column m

        players, width, scale, donor and flip as in mark_window_coalitions."""
        batch = (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq)
        return self._game("mark_window_shapley", "mark_window", "shapley", batch, players=players, width=width, scale=scale, donor=donor, flip=flip,
                          table=return_coalitions)

    @torch.no_grad()
    def mark_window_shapley_interactions(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                                         interaction_freq=None, players="promoter", width=1, scale=0.0, donor=None, flip=None, index="sii",
                                         return_coalitions=False):
        """Pairwise Shapley interaction indices of 2..16 window players (cf_mark_window_shapley_interactions) -> (inter, info),
        tensors on the model's device, no autograd graph: which stretches are redundant, which cooperate?  The 2^P coalitions run once,
        as in mark_window_shapley:

          %(inter)s
        info["donor"] takes the place of info["erased"] with a donor.  players, width, scale, donor and flip as in
        mark_window_coalitions; a window past the region's real bins and a player in a dummy slot are null players."""
        batch = (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq)
        return self._game("mark_window_shapley_interactions", "mark_window", "shapley_interactions", batch, players=players, width=width, scale=scale,
                          donor=donor, flip=flip, index=index, table=return_coalitions)

    @torch.no_grad()
    def mark_window_shapley_sampled(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                                    interaction_freq=None, players="promoter", width=1, n_perm=64, seed=0, permutations=None, scale=0.0,
                                    donor=None, flip=None, return_rows=False):
        """Permutation-sampled Shapley values of up to 128 window players (cf_mark_window_shapley_sampled) -> (phi, info) with the keys,
        the row layout and the estimator of mark_shapley_sampled: which mark in which stretch?  players, width, scale, donor and flip
        as in mark_window_coalitions; n_perm, seed and permutations as in mark_shapley_sampled.  A null player (a window past the
        region's real bins, a dummy slot) has phi and stderr exactly 0."""
        batch = (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq)
        return self._game("mark_window_shapley_sampled", "mark_window", "shapley_sampled", batch, players=players, width=width, scale=scale,
                          donor=donor, flip=flip, perms=(n_perm, seed, permutations), table=return_rows)

    @torch.no_grad()
    def mark_window_shapley_interactions_sampled(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None,
                                                 interaction_masks=None, interaction_freq=None, players="promoter", width=1, focal=None,
                                                 index="sii", n_perm=64, seed=0, permutations=None, scale=0.0, donor=None, flip=None,
                                                 return_rows=False):
        """Permutation-sampled pairwise Shapley interaction indices of focal players among up to 128 window players
        (cf_mark_window_shapley_interactions_sampled) -> (inter, info) with the keys, the row layout and the estimator of
        mark_shapley_interactions_sampled: which stretches are redundant with the ones that carry the prediction?  players, width,
        scale, donor and flip as in mark_window_coalitions; focal, index, n_perm, seed and permutations as in
        mark_shapley_interactions_sampled.  The estimate is not symmetric; a null player (a window past the region's real bins, a
        dummy slot) has its row and column exactly 0."""
        batch = (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq)
        return self._game("mark_window_shapley_interactions_sampled", "mark_window", "shapley_interactions_sampled", batch, players=players,
                          width=width, scale=scale, donor=donor, flip=flip, focal=focal, index=index,
                          perms=(n_perm, seed, permutations), table=return_rows)

    def mark_window_shapley_dataset(self, dataset, donor_dataset=None, genes=None, players="promoter", width=1, n_perm=64, seed=0, scale=0.0,
                                    bsz=None, store=None, donor_store=None, interactions=None, dividends=False):
        """Shapley values of window players over the genes of a ChromoformerDataset, against a donor cell type's dataset if one is
        given, windows in genomic coordinates (chromoformer_amd.attribution.mark_window_shapley, a generator of per-gene dicts)."""
        return A.mark_window_shapley(self, dataset, donor_dataset, genes=genes, players=players, width=width, n_perm=n_perm, seed=seed,
                                     scale=scale, bsz=bsz, store=store, donor_store=donor_store, interactions=interactions, dividends=dividends)

    @torch.no_grad()
    def mark_fine_window_coalitions(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                                    interaction_freq=None, keep=None, region=0, players="windows", width=1, n_windows=None, start=0,
                                    lengths=None, scale=0.0, donor=None, flip=None, return_feats=False):
        """The prediction under coalitions of FINE window players (cf_mark_fine_coalitions) -> logits [B, n_coal, n_out] on the model's
        device, no autograd graph.  The game plays in one region (0 the promoter, 1 + j pCRE slot j); a player is a set of marks over a
        window of bins of the FINEST resolution, relative to the gene's `start` (attribution.fine_window_players: "windows", "cells" at
        `width` bins per window and `n_windows` windows, or (marks, (lo, hi)) pairs; at most 128).  `keep` as in mark_coalitions_wide.
        Column c is the inference forward with the marks of every ABSENT player, inside its window, scaled by `scale` in raw-signal
        space (0 erases; donor None) or taken from the donor (the forms of mark_donor_coalitions), at every resolution: a coarser bin
        the absent windows cover wholly follows mark_window_coalitions' rule, one they cover in part is recomputed from its finest
        children, weighted by their sample counts, as in perturbation_scan_fine; an element covered by several absent players changes
        once.  start: an int or B ints, the first finest genomic bin per gene; n_windows: default the windows that reach the end of
        the region from the smallest start; lengths, flip, return_feats ({binsize: [B, n_coal, n_bins, n_feats]}, the region's
        features that row (b, c) read; returned as (logits, feats)): as in perturbation_scan_fine.  One absent player gives the row of
        perturbation_scan_fine at that window, bit for bit; a window past the region's real bins changes nothing.  The packed forms of
        the first argument and the effect on a pending backward() are those of mark_coalitions."""
        batch = (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq)
        return self._game("mark_fine_window_coalitions", "mark_fine_window", "coalitions", batch, keep=keep, players=players, width=width,
                          scale=scale, donor=donor, flip=flip, fine=(region, n_windows, start, lengths), feats=return_feats)

    @torch.no_grad()
    def mark_fine_window_shapley(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                                 interaction_freq=None, region=0, players="windows", width=1, n_windows=None, start=0, lengths=None, scale=0.0,
                                 donor=None, flip=None, return_coalitions=False, return_feats=False):
        """Exact Shapley values of at most 16 fine window players (cf_mark_fine_shapley) -> (phi, info) with the keys of
        mark_window_shapley (info["feats"] with return_feats): which 200 bp of the peak carries the prediction?  Neighbouring fine windows
        share the credit here, where the leave-one-out perturbation_scan_fine scores redundant ones near zero.  Everything else as in
        mark_fine_window_coalitions; a null player (a window past the region's real bins, a dummy slot, a donor that agrees with the gene
        inside the window) has phi exactly 0."""
        batch = (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq)
        return self._game("mark_fine_window_shapley", "mark_fine_window", "shapley", batch, players=players, width=width, scale=scale, donor=donor,
                          flip=flip, fine=(region, n_windows, start, lengths), table=return_coalitions, feats=return_feats)

    @torch.no_grad()
    def mark_fine_window_shapley_interactions(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None,
                                              interaction_masks=None, interaction_freq=None, region=0, players="windows", width=1, n_windows=None,
                                              start=0, lengths=None, scale=0.0, donor=None, flip=None, index="sii", return_coalitions=False,
                                              return_feats=False):
        """Pairwise Shapley interaction indices of 2..16 fine window players (cf_mark_fine_shapley_interactions) -> (inter, info),
        tensors on the model's device, no autograd graph: which 200 bp stretches of the peak are redundant, which cooperate?  The 2^P
        coalitions run once, as in mark_fine_window_shapley:

          %(inter)s
        info["donor"] takes the place of info["erased"] with a donor; info["feats"] with return_feats.  Everything else as in
        mark_fine_window_shapley; a null player (a window past the region's real bins, a dummy slot, a donor that agrees with the gene
        inside the window) has its row and column exactly 0."""
        batch = (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq)
        return self._game("mark_fine_window_shapley_interactions", "mark_fine_window", "shapley_interactions", batch, players=players, width=width,
                          scale=scale, donor=donor, flip=flip,
                          fine=(region, n_windows, start, lengths), index=index, table=return_coalitions, feats=return_feats)

    @torch.no_grad()
    def mark_fine_window_shapley_sampled(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                                         interaction_freq=None, region=0, players="windows", width=1, n_windows=None, start=0, lengths=None,
                                         n_perm=64, seed=0, permutations=None, scale=0.0, donor=None, flip=None, return_rows=False,
                                         return_feats=False):
        """Permutation-sampled Shapley values of up to 128 fine window players (cf_mark_fine_shapley_sampled) -> (phi, info) with the
        keys, the row layout and the estimator of mark_shapley_sampled (info["feats"] with return_feats): which mark in which 200 bp?
        region, players, width, n_windows, start, lengths, scale, donor and flip as in mark_fine_window_coalitions; n_perm, seed and
        permutations as in mark_shapley_sampled.  A null player has phi and stderr exactly 0."""
        batch = (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq)
        return self._game("mark_fine_window_shapley_sampled", "mark_fine_window", "shapley_sampled", batch, players=players, width=width, scale=scale,
                          donor=donor, flip=flip, fine=(region, n_windows, start, lengths),
                          perms=(n_perm, seed, permutations), table=return_rows, feats=return_feats)

    @torch.no_grad()
    def mark_fine_window_shapley_interactions_sampled(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None,
                                                      interaction_masks=None, interaction_freq=None, region=0, players="windows", width=1,
                                                      n_windows=None, start=0, lengths=None, focal=None, index="sii", n_perm=64, seed=0,
                                                      permutations=None, scale=0.0, donor=None, flip=None, return_rows=False):
        """Permutation-sampled pairwise Shapley interaction indices of focal players among up to 128 fine window players
        (cf_mark_fine_shapley_interactions_sampled) -> (inter, info) with the keys, the row layout and the estimator of
        mark_shapley_interactions_sampled: which 200 bp stretches are redundant with the ones that carry the prediction?  region,
        players, width, n_windows, start, lengths, scale, donor and flip as in mark_fine_window_coalitions; focal, index, n_perm, seed
        and permutations as in mark_shapley_interactions_sampled.  The estimate is not symmetric; a null player has its row and column
        exactly 0."""
        batch = (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq)
        return self._game("mark_fine_window_shapley_interactions_sampled", "mark_fine_window", "shapley_interactions_sampled", batch, players=players,
                          width=width, scale=scale, donor=donor, flip=flip, fine=(region, n_windows, start, lengths), focal=focal, index=index,
                          perms=(n_perm, seed, permutations), table=return_rows)

    def mark_fine_window_shapley_dataset(self, dataset, donor_dataset=None, genes=None, region="promoter", zoom=1, coarse_width=1, width=2,
                                         players="windows", n_perm=64, seed=0, scale=0.0, target=None, bsz=None, store=None, donor_store=None,
                                         interactions=None, dividends=False):
        """Shapley values of fine window players over the genes of a ChromoformerDataset, zooming from the coarse window game, against a
        donor cell type's dataset if one is given, windows in genomic coordinates (chromoformer_amd.attribution.mark_fine_window_shapley,
        a generator of per-gene dicts)."""
        return A.mark_fine_window_shapley(self, dataset, donor_dataset, genes=genes, region=region, zoom=zoom, coarse_width=coarse_width, width=width,
                                          players=players, n_perm=n_perm, seed=seed, scale=scale, target=target, bsz=bsz, store=store,
                                          donor_store=donor_store, interactions=interactions, dividends=dividends)

    def raw_signal_gradients(self, dataset, genes=None, target=None, times_input=False, bsz=None):
        """Raw-signal saliency of the genes of a ChromoformerDataset: the gradient (or gradient x input) of logit column `target` with
        respect to the raw fp16 signals, per gene one track per histone mark for the promoter window and every pCRE, in genomic
        orientation (chromoformer_amd.attribution.raw_signal_gradients, a generator of per-gene dicts)."""
        return A.raw_signal_gradients(self, dataset, genes=genes, target=target, times_input=times_input, bsz=bsz)

    def raw_integrated_gradients(self, dataset, genes=None, target=None, n_steps=50, method="gausslegendre", bsz=None, donor_dataset=None):
        """Integrated gradients of logit column `target` with respect to the raw fp16 signals of the genes of a ChromoformerDataset, from
        the zero signal along a * x: per gene one track per histone mark for the promoter window and every pCRE, in genomic
        orientation, summing to logits - baseline_logits up to the quadrature error.  donor_dataset: another cell type's dataset over
        the same regions; the baseline is then its signal xd and the path xd + a * (x - xd)
        (chromoformer_amd.attribution.raw_integrated_gradients, a generator of per-gene dicts)."""
        return A.raw_integrated_gradients(self, dataset, genes=genes, target=target, n_steps=n_steps, method=method, bsz=bsz,
                                          donor_dataset=donor_dataset)

    # the paragraph about `inter` in five docstrings: (method, absent key, sibling method, does info name the players)
    for _f, _absent, _sibling, _players in ((pcre_shapley_interactions, "promoter_only", "pcre_shapley", False),
                                            (mark_shapley_interactions, "erased", "mark_shapley", True),
                                            (mark_donor_shapley_interactions, "donor", "mark_donor_shapley", True),
                                            (mark_window_shapley_interactions, "erased", "mark_window_shapley", True),
                                            (mark_fine_window_shapley_interactions, "erased", "mark_fine_window_shapley", True)):
        _f.__doc__ %= {"inter": _INTER_DOC % {"absent": _absent, "sibling": _sibling,
                                              "players": "\n          info[\"players\"]     the players' names" if _players else ""}}
    del _f, _absent, _sibling, _players
