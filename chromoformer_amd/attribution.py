"""Integrated gradients (ChromoformerBase.integrated_gradients): the quadrature table shared by the library call, its tests and users.

IG integrates the input gradient along the straight path from a baseline x' to the input x,
    attr = (x - x') * integral_0^1 dF(x' + a (x - x')) / dx da  ~  (x - x') * sum_k w_k g(x' + a_k (x - x')),
and satisfies completeness: the attributions of one gene sum to F(x) - F(x') up to the quadrature error.  The methods are Captum's
(IntegratedGradients(method=...)): Gauss-Legendre (default) and the four Riemann sums.  The trapezoid rule here is the composite one
on n equally spaced nodes including both ends (step 1 / (n - 1), half weights at the ends), so that every method's weights sum to 1.
"""
import ctypes as C

import numpy as np

METHODS = ("gausslegendre", "riemann_trapezoid", "riemann_middle", "riemann_left", "riemann_right")
INPUTS = ("promoter_feats", "pcre_feats", "interaction_freq")


def ig_quadrature64(method="gausslegendre", n_steps=50):
    """-> (alphas, weights), float64 [n_steps]: nodes and weights on [0, 1]."""
    if method not in METHODS:
        raise ValueError("integrated gradients: unknown method %r; choose from %s" % (method, METHODS))
    n = int(n_steps)
    if n != n_steps or n < 1:
        raise ValueError("integrated gradients: n_steps must be a positive integer, got %r" % (n_steps,))
    if method == "gausslegendre":
        x, w = np.polynomial.legendre.leggauss(n)
        return 0.5 * (x + 1.0), 0.5 * w
    if method == "riemann_trapezoid":
        if n < 2:
            raise ValueError("integrated gradients: riemann_trapezoid needs n_steps >= 2 (both ends of the path)")
        w = np.full(n, 1.0 / (n - 1))
        w[0] *= 0.5
        w[-1] *= 0.5
        return np.linspace(0.0, 1.0, n), w
    k = np.arange(n, dtype=np.float64)
    a = {"riemann_left": k / n, "riemann_middle": (k + 0.5) / n, "riemann_right": (k + 1.0) / n}[method]
    return a, np.full(n, 1.0 / n)


def ig_quadrature(method="gausslegendre", n_steps=50):
    """-> (alphas, weights), float32 [n_steps]: ig_quadrature64 cast to fp32 -- the table the library call uses."""
    a, w = ig_quadrature64(method, n_steps)
    return a.astype(np.float32), w.astype(np.float32)


def coalition_table(kind, i_max):
    """The pCRE coalition words (bit j set: slot j kept) of ChromoformerBase.pcre_shapley / pcre_epistasis -> uint32 array.
    "all": every word 0 .. 2^i_max - 1 in ascending order (word m at position m).  "pairs", with N = 2^i_max - 1: N; N without i for
    i = 0 .. i_max - 1; then N without i and j for the pairs i < j in lexicographic order (1 + S + S (S - 1) / 2 words)."""
    S = int(i_max)
    if S != i_max or not 1 <= S <= 31:
        raise ValueError("coalition_table: i_max = %r; an integer in 1..31" % (i_max,))
    if kind == "all":
        return np.arange(1 << S, dtype=np.uint32)
    if kind == "pairs":
        N = (1 << S) - 1
        words = [N] + [N & ~(1 << i) for i in range(S)] + [N & ~(1 << i) & ~(1 << j) for i in range(S) for j in range(i + 1, S)]
        return np.array(words, dtype=np.uint32)
    raise ValueError("coalition_table: kind %r; choose 'all' or 'pairs'" % (kind,))


def coalition_words(keep, i_max, who="pcre_coalitions", item="pCRE slot", limit="i_max"):
    """`keep` as the uint32 words the library reads: a sequence / array of ints (bit j set: slot j kept), or a bool array
    [n_coal, i_max] (column j: slot j kept).  Empty input, a negative word or a bit >= i_max raise ValueError naming `who`.
    (`item` / `limit`: what a bit and its bound are called in the messages; mark_coalition_words passes the players'.)"""
    S = int(i_max)
    a = np.asarray(keep.cpu() if hasattr(keep, "cpu") else keep)
    if a.size < 1:
        raise ValueError("%s: keep is empty: at least 1 coalition" % who)
    if a.dtype == np.bool_:
        if a.ndim != 2 or a.shape[1] != S:
            raise ValueError("%s: a bool keep must be [n_coal, %s = %d], got %s" % (who, limit, S, tuple(a.shape)))
        a = (a.astype(np.int64) << np.arange(S, dtype=np.int64)).sum(1)
    elif a.ndim != 1 or a.dtype.kind not in "iu":
        raise ValueError("%s: keep must be a sequence of ints or a bool array [n_coal, %s], got dtype %s with shape %s"
                         % (who, limit, a.dtype, tuple(a.shape)))
    a = a.astype(np.int64) if a.dtype != np.uint64 else a
    bad = [int(m) for m in a if int(m) < 0 or int(m) >> S]
    if bad:
        raise ValueError("%s: keep word(s) %s name a %s >= %s = %d (or are negative)" % (who, [hex(m) for m in bad[:4]], item, limit, S))
    return np.ascontiguousarray(a, dtype=np.uint32)


MARK_PLAYER_SPECS = ("marks", "compartments", "regions")


def mark_players(spec, n_feats, i_max):
    """The players of the histone-mark game (ChromoformerBase.mark_coalitions / mark_shapley / mark_epistasis) ->
    (marks uint32 [P], regions uint32 [P], names): bit f of marks[p] set = player p holds mark f; bit 0 of regions[p] = in the
    promoter, bit 1 + j = in pCRE slot j.  spec:

      "marks"          P = n_feats: player f is mark f in every region ("mark0", ...)
      "compartments"   P = 2 n_feats: mark f in the promoter ("mark0@promoter", ...), then mark f in all pCRE slots ("mark0@pcres", ...)
      "regions"        P = i_max + 1: all marks in region rho ("promoter", "pcre0", ...)
      a list of (marks, regions) pairs of index iterables (regions: 0 the promoter, 1 + j pCRE slot j); players may overlap

    More than 16 players, an empty player or an index out of range raise ValueError naming mark_players."""
    return _mark_players(spec, n_feats, i_max, "mark_players", MARK_PLAYER_SPECS, 16, "the exact game takes 1..16")


def _mark_players(spec, n_feats, i_max, who, specs, limit, limit_text):
    """mark_players / mark_players_wide: `specs` the named specs offered, `limit` the most players, `who` the name in the messages."""
    F, S = int(n_feats), int(i_max)
    every_mark, every_region = list(range(F)), list(range(S + 1))
    if isinstance(spec, str):
        if spec == "marks":
            pairs = [([f], every_region) for f in every_mark]
            names = ["mark%d" % f for f in every_mark]
        elif spec == "compartments":
            pairs = [([f], [0]) for f in every_mark] + [([f], every_region[1:]) for f in every_mark]
            names = ["mark%d@promoter" % f for f in every_mark] + ["mark%d@pcres" % f for f in every_mark]
        elif spec == "regions":
            pairs = [(every_mark, [rho]) for rho in every_region]
            names = ["promoter"] + ["pcre%d" % j for j in range(S)]
        elif spec == "cells" and spec in specs:
            pairs = [([f], [rho]) for rho in every_region for f in every_mark]
            names = ["mark%d@%s" % (f, "promoter" if rho == 0 else "pcre%d" % (rho - 1)) for rho in every_region for f in every_mark]
        else:
            raise ValueError("%s: players %r; choose from %s or give a list of (marks, regions) pairs" % (who, spec, specs))
    else:
        try:
            pairs = [(sorted({int(f) for f in ms}), sorted({int(r) for r in rs})) for ms, rs in spec]
        except (TypeError, ValueError):
            raise ValueError("%s: players must be one of %s or a list of (marks, regions) pairs of index iterables, got %r"
                             % (who, specs, spec)) from None
        names = ["marks(%s)@regions(%s)" % (",".join(map(str, ms)), ",".join(map(str, rs))) for ms, rs in pairs]
    if not 1 <= len(pairs) <= limit:
        raise ValueError("%s: %d players; %s" % (who, len(pairs), limit_text))
    for p, (ms, rs) in enumerate(pairs):
        if not ms or not rs:
            raise ValueError("%s: player %d is empty: at least one mark and one region" % (who, p))
        if ms[0] < 0 or ms[-1] >= min(F, 32):
            raise ValueError("%s: player %d names mark(s) %s outside [0, n_feats = %d)" % (who, p, ms, F))
        if rs[0] < 0 or rs[-1] > S:
            raise ValueError("%s: player %d names region(s) %s outside [0, i_max = %d]" % (who, p, rs, S))
    marks = np.array([sum(1 << f for f in ms) for ms, _ in pairs], dtype=np.uint32)
    regions = np.array([sum(1 << r for r in rs) for _, rs in pairs], dtype=np.uint32)
    return marks, regions, names


def mark_coalition_words(keep, n_players, who="mark_coalitions"):
    """`keep` as the uint32 words the library reads: a sequence / array of ints (bit p set: player p present), or a bool array
    [n_coal, P].  Empty input, a negative word or a bit >= P raise ValueError naming `who`."""
    return coalition_words(keep, n_players, who, item="player", limit="n_players")


CONTACT_PLAYER_SPECS = ("contacts", "pcres", "pcres_and_contacts", "all")


def contact_players(spec, i_max):
    """The players of the contact game (chromoformer_amd.contact: contact_coalitions / contact_shapley / contact_epistasis) ->
    (drop uint32 [P], contact uint32 [P], names): bit j of drop[p] set = pCRE slot j is deleted while player p is absent; bit j of
    contact[p] set = slot j's promoter contact frequency is edited while player p is absent.  spec:

      "contacts"            P = i_max: player j is slot j's contact ("contact0", ...)
      "pcres"               P = i_max: player j deletes slot j ("pcre0", ...): the pCRE game, the cross-check against pcre_shapley
      "pcres_and_contacts"  P = 2 i_max: players 0 .. i_max - 1 delete slot j ("pcre0", ...), players i_max .. 2 i_max - 1 edit its
                            contact ("contact0", ...): chromatin state against contact, slot by slot; i_max <= 8
      "all"                 P = 1: one player holding every contact ("contacts"): the model without Hi-C
      a list of (drop_slots, contact_slots) pairs of index iterables (either may be empty, not both); players may overlap

    More than 16 players, an empty player or a slot outside [0, i_max) raise ValueError naming contact_players."""
    who, S = "contact_players", int(i_max)
    slots = list(range(S))
    if isinstance(spec, str):
        if spec == "contacts":
            pairs, names = [([], [j]) for j in slots], ["contact%d" % j for j in slots]
        elif spec == "pcres":
            pairs, names = [([j], []) for j in slots], ["pcre%d" % j for j in slots]
        elif spec == "pcres_and_contacts":
            if S > 8:
                raise ValueError("%s: players 'pcres_and_contacts' needs 2 i_max = %d players and the exact game takes 1..16 (2^P rows "
                                 "per gene): with i_max = %d > 8 choose 'contacts' or give a list of (drop_slots, contact_slots) pairs "
                                 "for the slots of interest" % (who, 2 * S, S))
            pairs = [([j], []) for j in slots] + [([], [j]) for j in slots]
            names = ["pcre%d" % j for j in slots] + ["contact%d" % j for j in slots]
        elif spec == "all":
            pairs, names = [([], slots)], ["contacts"]
        else:
            raise ValueError("%s: players %r; choose from %s or give a list of (drop_slots, contact_slots) pairs" % (who, spec, CONTACT_PLAYER_SPECS))
    else:
        try:
            pairs = [(sorted({int(j) for j in ds}), sorted({int(j) for j in cs})) for ds, cs in spec]
        except (TypeError, ValueError):
            raise ValueError("%s: players must be one of %s or a list of (drop_slots, contact_slots) pairs of index iterables, got %r"
                             % (who, CONTACT_PLAYER_SPECS, spec)) from None
        names = ["drop(%s)+contact(%s)" % (",".join(map(str, ds)), ",".join(map(str, cs))) for ds, cs in pairs]
    if not 1 <= len(pairs) <= 16:
        raise ValueError("%s: %d players; the exact game takes 1..16" % (who, len(pairs)))
    for p, (ds, cs) in enumerate(pairs):
        if not ds and not cs:
            raise ValueError("%s: player %d is empty: at least one pCRE slot to delete or one contact to edit" % (who, p))
        for what, js in (("drop", ds), ("contact", cs)):
            if js and (js[0] < 0 or js[-1] >= S):
                raise ValueError("%s: player %d names %s slot(s) %s outside [0, i_max = %d)" % (who, p, what, js, S))
    drop = np.array([sum(1 << j for j in ds) for ds, _ in pairs], dtype=np.uint32)
    contact = np.array([sum(1 << j for j in cs) for _, cs in pairs], dtype=np.uint32)
    return drop, contact, names


MARK_WIDE_PLAYER_SPECS = MARK_PLAYER_SPECS + ("cells",)
MARK_WIDE_MAX_PLAYERS = 128


def mark_players_wide(spec, n_feats, i_max):
    """The players of the wide histone-mark game (ChromoformerBase.mark_coalitions_wide / mark_shapley_sampled) -> (marks, regions,
    names) as mark_players returns them, for up to 128 players.  spec: what mark_players takes, or

      "cells"   P = n_feats (i_max + 1): player rho * n_feats + f is mark f in region rho alone ("mark0@promoter", ...,
                "mark0@pcre0", ...); a [B, P, n_out] result reshapes to [B, i_max + 1, n_feats, n_out]

    More than 128 players, an empty player or an index out of range raise ValueError naming mark_players_wide."""
    return _mark_players(spec, n_feats, i_max, "mark_players_wide", MARK_WIDE_PLAYER_SPECS, MARK_WIDE_MAX_PLAYERS,
                         "the sampled game takes 1..%d" % MARK_WIDE_MAX_PLAYERS)


def mark_wide_words(keep, P, who="mark_coalitions_wide"):
    """`keep` as the uint32 words [n_coal, kw], kw = ceil(P / 32), the wide game reads (bit p % 32 of word p / 32 set: player p
    present): a bool array [n_coal, P], or a sequence of Python ints of any width (bit p set: player p present).  Empty input, a
    negative int or a bit >= P raise ValueError naming `who`."""
    P = int(P)
    kw = (P + 31) // 32
    a = keep.cpu().numpy() if hasattr(keep, "cpu") else keep
    if isinstance(a, np.ndarray) and a.dtype == np.bool_:
        if a.ndim != 2 or a.shape[1] != P or a.shape[0] < 1:
            raise ValueError("%s: a bool keep must be [n_coal >= 1, n_players = %d], got %s" % (who, P, tuple(a.shape)))
        bits = np.zeros((a.shape[0], kw * 32), dtype=np.uint64)
        bits[:, :P] = a
        return np.ascontiguousarray((bits.reshape(a.shape[0], kw, 32) << np.arange(32, dtype=np.uint64)).sum(2).astype(np.uint32))
    try:
        ints = [int(m) for m in a]
        exact = all(m == x for m, x in zip(ints, a))
    except (TypeError, ValueError):
        ints, exact = [], False
    if not ints or not exact:
        raise ValueError("%s: keep must be a non-empty sequence of ints or a bool array [n_coal, n_players = %d]" % (who, P))
    bad = [m for m in ints if m < 0 or m >> P]
    if bad:
        raise ValueError("%s: keep word(s) %s name a player >= n_players = %d (or are negative)" % (who, [hex(m) for m in bad[:4]], P))
    return np.array([[(m >> (32 * w)) & 0xFFFFFFFF for w in range(kw)] for m in ints], dtype=np.uint32).reshape(len(ints), kw)


INTERACTION_INDICES = ("sii", "sti")


def interaction_index(index, who="interaction_index"):
    """The library's constant of an interaction index name ("sii": the Shapley interaction index, "sti": Shapley-Taylor of order 2);
    anything else raises ValueError listing the two."""
    from . import _lib
    if not isinstance(index, str) or index not in _lib.INTERACTION_INDEX:
        raise ValueError("%s: unknown interaction index %r; choose from %s" % (who, index, list(INTERACTION_INDICES)))
    return _lib.INTERACTION_INDEX[index]


def interaction_weights(P, index="sii"):
    """The weight table of the pairwise interaction index of a game of P >= 2 players -> float64 [P - 1]: w[s] for a coalition of s
    players that holds neither of the pair.  "sii": s! (P - s - 2)! / (P - 1)!, which sums to 1 over all such coalitions; "sti":
    (2 / P) / C(P - 1, s).  The library computes the same table in double and rounds it to fp32."""
    from math import comb, factorial
    interaction_index(index, "interaction_weights")
    P = int(P)
    if P < 2:
        raise ValueError("interaction_weights: P = %d: a pair needs at least 2 players" % P)
    if index == "sii":
        return np.array([factorial(s) * factorial(P - s - 2) / factorial(P - 1) for s in range(P - 1)], dtype=np.float64)
    return np.array([(2.0 / P) / comb(P - 1, s) for s in range(P - 1)], dtype=np.float64)


def _popcount(words):
    """The number of players in each uint32 word -> int64, the shape of `words`."""
    words = np.asarray(words, dtype=np.uint32)
    n = np.zeros(words.shape, dtype=np.int64)
    for k in range(32):
        n += (words >> np.uint32(k)) & np.uint32(1)
    return n


def _order_check(who, P, order):
    P, order = int(P), int(order)
    if not 1 <= P <= 16:
        raise ValueError("%s: P = %d outside 1..16" % (who, P))
    if not 1 <= order <= P:
        raise ValueError("%s: order = %d outside 1..P = %d" % (who, order, P))
    return P, order


def interaction_sets(P, order):
    """The words of every set of 1..order of P players -> uint32 [n]: bit p set = player p in the set, ordered by size and then by
    ascending word (P = 16, order = 3: 16 + 120 + 560 = 696 sets).  1 <= order <= P <= 16."""
    P, order = _order_check("interaction_sets", P, order)
    words = np.arange(1, 1 << P, dtype=np.uint32)
    size = _popcount(words)
    words, size = words[size <= order], size[size <= order]
    return np.ascontiguousarray(words[np.argsort(size, kind="stable")])


def set_interaction_weights(P, index="sii", order=2):
    """The weights that turn Harsanyi dividends into an interaction index of top order `order` -> float64 [order + 1, P + 1]:
    index(S) = sum over U >= S of w[|S|, |U|] dividend(U); entries with |U| < |S| and row 0 are 0.  "sii": 1 / (|U| - |S| + 1) -- the
    Shapley value at |S| = 1, the pairwise Shapley interaction index at |S| = 2.  "sti" (Shapley-Taylor of order k = `order`): a set
    below the top order gets its own dividend (w = 1 at U = S alone), a set of size k gets 1 / C(|U|, k); the index then sums to
    v(everybody) - v(nobody) over all sets of size 1..k.  The library computes the same table in double and rounds it to fp32."""
    from math import comb
    interaction_index(index, "set_interaction_weights")
    P, order = _order_check("set_interaction_weights", P, order)
    w = np.zeros((order + 1, P + 1), dtype=np.float64)
    for s in range(1, order + 1):
        for u in range(s, P + 1):
            if index == "sii":
                w[s, u] = 1.0 / (u - s + 1)
            elif s == order:
                w[s, u] = 1.0 / comb(u, order)
            else:
                w[s, u] = 1.0 if u == s else 0.0
    return w


def set_names(words, names):
    """The names of sets of players given as words -> a list of strings: the players' names in ascending bit order joined by "*"
    ("mark0*mark3"); the empty set is "" .  A word with a bit >= len(names) raises ValueError."""
    names = list(names)
    out = []
    for k, w in enumerate(np.asarray(words).reshape(-1).tolist()):
        w = int(w)
        if w < 0 or w >> len(names):
            raise ValueError("set_names: words[%d] = 0x%x names a player >= %d" % (k, w, len(names)))
        out.append("*".join(names[p] for p in range(len(names)) if w >> p & 1))
    return out


def dividend_bound(mass, P):
    """The rounding bound of the fp32 dividends -> an array of the shape of `mass` ([..., 2^P, n_out], numpy or anything np.asarray
    takes), float64: |dividend(S) - exact| <= ((1 + 2^-24)^|S| - 1) mass(S), since the element passes through |S| subtractions, each
    with a relative error of at most 2^-24, of quantities whose magnitudes sum to at most mass(S) = sum over T <= S of |v(T)|.  The
    fp32 `mass` itself is |S| rounded additions of non-negative numbers, so it may fall short of the exact sum by a factor
    (1 - 2^-24)^|S|: the bound is widened by (1 - 2^-24)^-|S|.  A dividend smaller than its bound is rounding noise."""
    P = int(P)
    m = np.asarray(mass, dtype=np.float64)
    if m.ndim < 2 or m.shape[-2] != 1 << P:
        raise ValueError("dividend_bound: mass has shape %s; expected [..., 2^P = %d, n_out]" % (m.shape, 1 << P))
    size = _popcount(np.arange(1 << P, dtype=np.uint32)).astype(np.float64)
    u = 2.0 ** -24
    factor = ((1.0 + u) ** size - 1.0) * (1.0 - u) ** -size
    return m * factor[:, None]


def top_dividends(div, names, k=10, min_order=1):
    """The k largest dividends of one gene by magnitude among the sets of at least min_order players -> a list of (set name, word,
    value) with value float32 [n_out], sorted by falling max |value| over the outputs.  div: [2^P, n_out] (numpy or a tensor's
    .cpu().numpy()), names: the P players' names."""
    d = np.asarray(div)
    P = len(names)
    if d.ndim != 2 or d.shape[0] != 1 << P:
        raise ValueError("top_dividends: div has shape %s; expected [2^P = %d, n_out] for %d names" % (d.shape, 1 << P, P))
    if int(k) < 1 or int(min_order) < 0:
        raise ValueError("top_dividends: k >= 1 and min_order >= 0")
    words = np.arange(1 << P, dtype=np.uint32)
    words = words[_popcount(words) >= int(min_order)]
    mag = np.abs(d[words]).max(axis=1)
    pick = words[np.argsort(-mag, kind="stable")[:int(k)]]
    return [(nm, int(w), d[w].copy()) for nm, w in zip(set_names(pick, names), pick)]


def shapley_permutations(P, n_perm, seed=0):
    """n_perm independent uniform orders of P players -> uint8 [n_perm, P], each row a permutation of 0..P-1, from
    numpy.random.Generator(PCG64(seed)): the same seed gives the same orders."""
    P, n_perm = int(P), int(n_perm)
    if not 1 <= P <= MARK_WIDE_MAX_PLAYERS or n_perm < 1:
        raise ValueError("shapley_permutations: P = %d in 1..%d and n_perm = %d >= 1 are required" % (P, MARK_WIDE_MAX_PLAYERS, n_perm))
    rng = np.random.Generator(np.random.PCG64(int(seed)))
    return np.stack([rng.permutation(P) for _ in range(n_perm)]).astype(np.uint8)


def focal_players(focal, names, P):
    """The focal players of a sampled interactions call -> int32 [n_focal]: `focal` is a sequence of player indices or of player names
    (entries of `names`), or one of either.  An empty sequence, an unknown name, an index outside 0..P-1 or a repeated player raise
    ValueError naming focal_players."""
    P = int(P)
    if isinstance(focal, (str, int, np.integer)):
        focal = [focal]
    try:
        given = list(focal.tolist() if hasattr(focal, "tolist") else focal)
    except TypeError:
        given = []
    if not given:
        raise ValueError("focal_players: focal must name at least one player (indices or names)")
    out = []
    for at, x in enumerate(given):
        if isinstance(x, str):
            if names is None or x not in names:
                raise ValueError("focal_players: focal[%d] = %r is not a player name" % (at, x))
            x = list(names).index(x)
        elif isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)):
            raise ValueError("focal_players: focal[%d] = %r is neither a player index nor a player name" % (at, x))
        x = int(x)
        if not 0 <= x < P:
            raise ValueError("focal_players: focal[%d] = %d outside 0..%d" % (at, x, P - 1))
        if x in out:
            raise ValueError("focal_players: focal[%d] = %d repeats focal[%d]" % (at, x, out.index(x)))
        out.append(x)
    return np.array(out, dtype=np.int32)


def focal_row_count(perms, focal):
    """The rows per gene of focal_words(perms, focal) without building them: 2 + n_perm (P - 1) shared with mark_shapley_sampled, then
    per focal player 2 + sum over the orders of P - 2 (the player first or last in the order) or P - 3 (elsewhere)."""
    perms = np.asarray(perms)
    n_perm, P = perms.shape
    R = 2 + n_perm * (P - 1)
    for i in focal:
        r = np.argmax(perms == int(i), axis=1)
        ends = int(((r == 0) | (r == P - 1)).sum())
        R += 2 + ends * (P - 2) + (n_perm - ends) * (P - 3)
    return int(R)


def focal_words(perms, focal):
    """The rows of a sampled interactions call (ChromoformerBase.mark_shapley_interactions_sampled) -> (words, col).  perms: integer
    [n_perm, P], each row an order of the P >= 2 players; focal: distinct player indices.  words: the R coalitions as Python ints (bit p
    set: player p present) in row order -- nobody, everybody, per order q its first k = 1 .. P - 1 players (mark_shapley_sampled's
    table), then per focal player i: {i} alone, everybody but i, and per order, with o the order without i, T_k its first k players and
    r the position of i in the order, the rows T_k + i for k = 1 .. r - 1, then the rows T_k for k = r + 1 .. P - 2 (the others are
    prefixes of the order itself).  col: uint32 [n_focal, n_perm, P, 2], col[f, q, k, 0] the row of T_k and col[f, q, k, 1] that of
    T_k + i, k = 0 .. P - 1: what the library's reducer reads.  Where a set is a prefix of the order, col names that leading row ({i}
    alone for an order that starts with i, everybody but i for one that ends with it, too).  Focal player f's own rows start at row
    focal_row_count(perms, focal[:f])."""
    perms = np.asarray(perms)
    if perms.ndim != 2 or perms.shape[1] < 2 or perms.dtype.kind not in "iu":
        raise ValueError("focal_words: perms must be an integer array [n_perm, P >= 2]")
    n_perm, P = perms.shape
    for q in range(n_perm):
        if sorted(int(x) for x in perms[q]) != list(range(P)):
            raise ValueError("focal_words: perms[%d] is not a permutation of 0..%d" % (q, P - 1))
    focal = focal_players(focal, None, P)
    full = (1 << P) - 1
    words = [0, full]
    for q in range(n_perm):
        m = 0
        for k in range(1, P):
            m |= 1 << int(perms[q, k - 1])
            words.append(m)
    col = np.zeros((len(focal), n_perm, P, 2), dtype=np.uint32)
    for f, i in enumerate(int(x) for x in focal):
        alone, without = len(words), len(words) + 1
        words += [1 << i, full & ~(1 << i)]
        for q in range(n_perm):
            pi = [int(x) for x in perms[q]]
            r = pi.index(i)
            prefix = lambda k: 2 + q * (P - 1) + (k - 1)      # noqa: E731 (the first k of pi, 1 <= k <= P - 1)
            col[f, q, 0] = (0, prefix(1) if r == 0 else alone)      # (a prefix of the order where there is one)
            col[f, q, P - 1] = (prefix(P - 1) if r == P - 1 else without, 1)
            m = 1 << i
            for k in range(1, P - 1):      # T_k + i
                if k < r:
                    m |= 1 << pi[k - 1]
                    col[f, q, k, 1] = len(words)
                    words.append(m)
                else:
                    col[f, q, k, 1] = prefix(k + 1)
            m = sum(1 << p for p in pi[:r])
            for k in range(1, P - 1):      # T_k
                if k > r:
                    m |= 1 << pi[k]
                    col[f, q, k, 0] = len(words)
                    words.append(m)
                else:
                    col[f, q, k, 0] = prefix(k)
    return words, col


WINDOW_PLAYER_SPECS = ("promoter", "promoter_cells", "regions")


def window_players(spec, n_feats, i_max, W, width=1):
    """The players of the window game (ChromoformerBase.mark_window_coalitions / mark_window_shapley / mark_window_shapley_sampled) ->
    (marks, regions, lo, hi, names): uint32 [P] mark and region words as mark_players returns them, int32 [P] windows [lo, hi) in
    bins of the coarsest resolution (W of them per region: the windows of the perturbation scan), and a name per player.  With
    n_win = ceil(W / width) windows [g width, min((g + 1) width, W)):

      "promoter"         P = n_win: all marks over window g of the promoter ("promoter[4:6]")
      "promoter_cells"   P = n_feats n_win: player g * n_feats + f is mark f over window g of the promoter ("mark3@promoter[4:6]"); a
                         [B, P, n_out] result reshapes to [B, n_win, n_feats, n_out]
      "regions"          P = (i_max + 1) n_win: player rho * n_win + g is all marks over window g of region rho ("promoter[0:2]", ...,
                         "pcre1[0:2]", ...)
      a list of (marks, regions, (lo, hi)) triples: index iterables as in mark_players and a window; players may overlap

    More than 128 players (the count is named: choose a larger width), an empty player, an index out of range or a window outside
    0 <= lo < hi <= W raise ValueError naming window_players."""
    who = "window_players"
    F, S, W = int(n_feats), int(i_max), int(W)
    if W < 1:
        raise ValueError("%s: W = %d: the coarsest resolution has at least one bin" % (who, W))
    every_mark = list(range(F))

    def region_name(rho):
        return "promoter" if rho == 0 else "pcre%d" % (rho - 1)

    if isinstance(spec, str):
        if spec not in WINDOW_PLAYER_SPECS:
            raise ValueError("%s: players %r; choose from %s or give a list of (marks, regions, (lo, hi)) triples" % (who, spec, WINDOW_PLAYER_SPECS))
        width = int(width)
        if width < 1:
            raise ValueError("%s: width = %d: at least 1 coarsest bin" % (who, width))
        wins = [(g, min(g + width, W)) for g in range(0, W, width)]
        if spec == "promoter":
            triples = [(every_mark, [0], w) for w in wins]
            names = ["promoter[%d:%d]" % w for w in wins]
        elif spec == "promoter_cells":
            triples = [([f], [0], w) for w in wins for f in every_mark]
            names = ["mark%d@promoter[%d:%d]" % ((f,) + w) for w in wins for f in every_mark]
        else:
            triples = [(every_mark, [rho], w) for rho in range(S + 1) for w in wins]
            names = ["%s[%d:%d]" % ((region_name(rho),) + w) for rho in range(S + 1) for w in wins]
        if len(triples) > MARK_WIDE_MAX_PLAYERS:
            raise ValueError("%s: %r at width = %d gives %d players; the game takes 1..%d: choose a larger width"
                             % (who, spec, width, len(triples), MARK_WIDE_MAX_PLAYERS))
    else:
        try:
            triples = [(sorted({int(f) for f in ms}), sorted({int(r) for r in rs}), (int(w[0]), int(w[1]))) for ms, rs, w in spec]
        except (TypeError, ValueError, IndexError):
            raise ValueError("%s: players must be one of %s or a list of (marks, regions, (lo, hi)) triples, got %r"
                             % (who, WINDOW_PLAYER_SPECS, spec)) from None
        names = ["marks(%s)@regions(%s)[%d:%d]" % (",".join(map(str, ms)), ",".join(map(str, rs)), w[0], w[1]) for ms, rs, w in triples]
        if not 1 <= len(triples) <= MARK_WIDE_MAX_PLAYERS:
            raise ValueError("%s: %d players; the game takes 1..%d: choose a larger width" % (who, len(triples), MARK_WIDE_MAX_PLAYERS))
    for p, (ms, rs, (lo, hi)) in enumerate(triples):
        if not ms or not rs:
            raise ValueError("%s: player %d is empty: at least one mark and one region" % (who, p))
        if ms[0] < 0 or ms[-1] >= min(F, 32):
            raise ValueError("%s: player %d names mark(s) %s outside [0, n_feats = %d)" % (who, p, ms, F))
        if rs[0] < 0 or rs[-1] > S:
            raise ValueError("%s: player %d names region(s) %s outside [0, i_max = %d]" % (who, p, rs, S))
        if lo < 0 or hi > W or lo >= hi:
            raise ValueError("%s: player %d has the window [%d, %d): 0 <= lo < hi <= W = %d is required" % (who, p, lo, hi, W))
    marks = np.array([sum(1 << f for f in ms) for ms, _, _ in triples], dtype=np.uint32)
    regions = np.array([sum(1 << r for r in rs) for _, rs, _ in triples], dtype=np.uint32)
    lo = np.array([w[0] for _, _, w in triples], dtype=np.int32)
    hi = np.array([w[1] for _, _, w in triples], dtype=np.int32)
    return marks, regions, lo, hi, names


FINE_WINDOW_PLAYER_SPECS = ("windows", "cells")


def fine_window_players(spec, n_feats, width=1, n_windows=1):
    """The players of the fine window game (ChromoformerBase.mark_fine_window_coalitions / mark_fine_window_shapley /
    mark_fine_window_shapley_sampled) -> (marks, lo, hi, names): uint32 [P] mark words as mark_players returns them, int32 [P] windows
    [lo, hi) in bins of the FINEST resolution relative to each gene's start, and a name per player.  With window g = [g width,
    (g + 1) width), g < n_windows:

      "windows"   P = n_windows: all marks over window g ("fine[4:6]")
      "cells"     P = n_feats n_windows: player g * n_feats + f is mark f over window g ("mark3@fine[4:6]"); a [B, P, n_out] result
                  reshapes to [B, n_windows, n_feats, n_out]
      a list of (marks, (lo, hi)) pairs: index iterables as in mark_players and a window; players may overlap

    More than 128 players (the count is named: choose a larger width), an empty player, a mark out of range or a window without
    0 <= lo < hi raise ValueError naming fine_window_players."""
    who = "fine_window_players"
    F = int(n_feats)
    every_mark = list(range(F))
    if isinstance(spec, str):
        if spec not in FINE_WINDOW_PLAYER_SPECS:
            raise ValueError("%s: players %r; choose from %s or give a list of (marks, (lo, hi)) pairs" % (who, spec, FINE_WINDOW_PLAYER_SPECS))
        width, n_windows = int(width), int(n_windows)
        if width < 1:
            raise ValueError("%s: width = %d: at least 1 finest bin" % (who, width))
        if n_windows < 1:
            raise ValueError("%s: n_windows = %d: at least 1 window" % (who, n_windows))
        count = n_windows * (F if spec == "cells" else 1)
        if count > MARK_WIDE_MAX_PLAYERS:
            raise ValueError("%s: %r at width = %d over %d windows gives %d players; the game takes 1..%d: choose a larger width"
                             % (who, spec, width, n_windows, count, MARK_WIDE_MAX_PLAYERS))
        wins = [(g * width, (g + 1) * width) for g in range(n_windows)]
        if spec == "windows":
            pairs = [(every_mark, w) for w in wins]
            names = ["fine[%d:%d]" % w for w in wins]
        else:
            pairs = [([f], w) for w in wins for f in every_mark]
            names = ["mark%d@fine[%d:%d]" % ((f,) + w) for w in wins for f in every_mark]
    else:
        try:
            pairs = [(sorted({int(f) for f in ms}), (int(w[0]), int(w[1]))) for ms, w in spec]
        except (TypeError, ValueError, IndexError):
            raise ValueError("%s: players must be one of %s or a list of (marks, (lo, hi)) pairs, got %r" % (who, FINE_WINDOW_PLAYER_SPECS, spec)) from None
        names = ["marks(%s)@fine[%d:%d]" % (",".join(map(str, ms)), w[0], w[1]) for ms, w in pairs]
        if not 1 <= len(pairs) <= MARK_WIDE_MAX_PLAYERS:
            raise ValueError("%s: %d players; the game takes 1..%d: choose a larger width" % (who, len(pairs), MARK_WIDE_MAX_PLAYERS))
    for p, (ms, (lo, hi)) in enumerate(pairs):
        if not ms:
            raise ValueError("%s: player %d is empty: at least one mark" % (who, p))
        if ms[0] < 0 or ms[-1] >= min(F, 32):
            raise ValueError("%s: player %d names mark(s) %s outside [0, n_feats = %d)" % (who, p, ms, F))
        if lo < 0 or lo >= hi or hi >= 2 ** 31:
            raise ValueError("%s: player %d has the window [%d, %d): 0 <= lo < hi finest bins is required" % (who, p, lo, hi))
    marks = np.array([sum(1 << f for f in ms) for ms, _ in pairs], dtype=np.uint32)
    lo = np.array([w[0] for _, w in pairs], dtype=np.int32)
    hi = np.array([w[1] for _, w in pairs], dtype=np.int32)
    return marks, lo, hi, names


_BATCH_KEYS = ("promoter_feats", "promoter_pad_masks", "pcre_feats", "pcre_pad_masks", "interaction_masks", "interaction_freq")      # forward()'s arguments, in order


def _donor_pair(dd):
    """The donor of a batch, from the donor store's batch dict -> (promoter_feats, pcre_feats), contiguous, by bin size."""
    return ({b: t.contiguous() for b, t in dd["promoter_feats"].items()}, {b: t.contiguous() for b, t in dd["pcre_feats"].items()})


def _region_index(who, region, S):
    """"promoter" or a pCRE slot j -> the region index (0 the promoter, 1 + j pCRE slot j)."""
    if region == "promoter":
        return 0
    if isinstance(region, str) or not 0 <= int(region) < S:
        raise ValueError("%s: region %r; choose 'promoter' or a pCRE slot in [0, i_max = %d)" % (who, region, S))
    return 1 + int(region)


def _gene_region(ds, g, region, col0):
    """Region `region` of gene g -> (chrom, start, end): the promoter window from its first stored column col0 on, or the pCRE; None
    for a pCRE slot the gene does not have."""
    if region == 0:
        chrom, tss, _ = ds.genes[g]["tss"]
        return (chrom, tss - 20000 + col0, tss - 20000 + col0 + min(ds.w_prom, 40000 - col0))
    pc = ds.genes[g]["pcres"]
    return tuple(pc[region - 1]) if region - 1 < len(pc) else None


def _geometry_check(who, model, dataset, binsizes):
    """The model is on the device and the dataset has its geometry -> n_bins."""
    ds = dataset
    if model._handle is None:
        raise RuntimeError("call .cuda() first: the Chromoformer HIP path needs device buffers")
    n_bins = [ds.w_max // b for b in binsizes]
    if binsizes != list(model.binsizes) or n_bins != list(model.n_bins) or ds.i_max != model.i_max or ds.n_feats != model.n_feats:
        raise ValueError("%s: the dataset (binsizes %s, w_max %d, i_max %d, n_feats %d) does not match the model "
                         "(binsizes %s, w_max %d, i_max %d, n_feats %d)" % (who, binsizes, ds.w_max, ds.i_max, ds.n_feats, list(model.binsizes),
                                                                            model.w_max, model.i_max, model.n_feats))
    return n_bins


def _genes_check(who, model, dataset, genes, bsz):
    """-> (the genes, all in the dataset's metadata; chunk size)."""
    genes = list(dataset.target_genes if genes is None else genes)
    missing = [g for g in genes if g not in dataset.genes]
    if missing:
        raise KeyError("%s: gene(s) %s are not in the dataset's metadata" % (who, missing[:5]))
    return genes, model._max_batch if bsz is None else max(1, min(int(bsz), model._max_batch))


def _raw_check(who, model, dataset, genes, target, bsz):
    """The checks the raw-signal generators share -> (binsizes, n_bins, target, genes, chunk size)."""
    binsizes = [int(b) for b in dataset.binsizes]
    if len(binsizes) > 3 or len(set(binsizes)) != len(binsizes):
        raise ValueError("%s: binsizes %s: more than three or repeated bin sizes are binned by one cf_bin_regions launch "
                         "per resolution, which has no backward; use at most three distinct bin sizes" % (who, binsizes))
    n_bins = _geometry_check(who, model, dataset, binsizes)
    target = (1 if model.n_out == 2 else 0) if target is None else int(target)
    if not 0 <= target < model.n_out:
        raise ValueError("%s: target = %d outside [0, n_out = %d)" % (who, target, model.n_out))
    genes, chunk = _genes_check(who, model, dataset, genes, bsz)
    return binsizes, n_bins, target, genes, chunk


class _RawChunk:
    """The raw regions of a chunk of genes on the device, binned by cf_bin_regions_multi into the model's inputs: what the raw-signal
    generators share -- region loading, the job tables of the binning and of its backward, the scatter back into per-gene tracks."""

    def __init__(self, model, ds, ids, binsizes, n_bins):
        import torch

        from . import _lib
        from .data import BIN_JOB_MULTI, load_raw_regions, raw_window
        self.ds, self.ids, self.binsizes, self.n_bins = ds, ids, binsizes, n_bins
        self.dev, self.lib = model._device, _lib.lib()
        dev = self.dev
        B = len(ids)
        S, T, F, nres = ds.i_max, ds.i_max + 1, ds.n_feats, len(binsizes)
        self.F, self.nres = F, nres
        self.order = order = sorted(range(nres), key=lambda r: -binsizes[r])      # coarsest first
        self.cb = (C.c_int * nres)(*[binsizes[r] for r in order])
        self.cl = (C.c_int * nres)(*[n_bins[r] for r in order])
        self.regs = regs = []                                    # (gene row, slot, flip, raw array, col0, ncols, raw offset, draw offset, ld_out)
        n_raw = n_out = max_cols = 0
        for i, gene in enumerate(ids):
            for s, flip, a in load_raw_regions(ds, gene):
                c0, nc = raw_window(ds, s, a.shape[1])
                for r, b in enumerate(binsizes):
                    if -(-nc // b) > n_bins[r]:
                        raise ValueError("region spans %d bins but w_max allows %d" % (-(-nc // b), n_bins[r]))
                ld_out = -(-nc // 4) * 4
                regs.append((i, s, flip, a, c0, nc, n_raw, n_out, ld_out))
                n_raw += -(-a.size // 4) * 4                     # every region starts 8-byte aligned
                n_out += F * ld_out
                max_cols = max(max_cols, nc)
        self.max_cols = max_cols
        flat = np.zeros(n_raw, dtype=np.float16)
        for _, _, _, a, _, _, off, _, _ in regs:
            flat[off:off + a.size] = a.reshape(-1)
        self.stream = torch.cuda.current_stream(dev)
        with torch.cuda.device(dev):
            self.raw = raw = torch.from_numpy(flat).to(dev)
            self.draw = torch.empty(max(n_out, 1), dtype=torch.float32, device=dev)      # (every window sample is written by the library)
            self.pf = pf = [torch.zeros(B, 1, L, F, device=dev) for L in n_bins]
            self.cf = cf = [torch.zeros(B, S, L, F, device=dev) for L in n_bins]
            self.pm = pm = [torch.ones(B, L, dtype=torch.uint8, device=dev) for L in n_bins]
            self.cm = cm = [torch.ones(B, S, L, dtype=torch.uint8, device=dev) for L in n_bins]      # dummy slots stay fully masked
            im = torch.ones(B, T, T, dtype=torch.uint8)
            freq = torch.zeros(B, T, T)
            for i, gene in enumerate(ids):
                g = ds.genes[gene]
                n_part = len(g["pcres"])
                im[i, :n_part + 1, :n_part + 1] = 0
                for s, sc in enumerate(g["scores"]):
                    freq[i, 0, s + 1] = sc
            self.im, self.freq = im.to(dev), freq.to(dev)
            self.fj = fj = np.zeros(len(regs), dtype=BIN_JOB_MULTI)
            for k, (i, s, flip, a, c0, nc, off, _, _) in enumerate(regs):
                fj[k]["raw"], fj[k]["ld"], fj[k]["col0"], fj[k]["ncols"], fj[k]["flip"] = raw.data_ptr() + 2 * off, a.shape[1], c0, nc, int(flip)
                for r in range(nres):
                    out = pf[r][i, 0] if s < 0 else cf[r][i, s]
                    msk = pm[r][i] if s < 0 else cm[r][i, s]
                    fj[k]["out"][order.index(r)], fj[k]["mask"][order.index(r)] = out.data_ptr(), msk.data_ptr()
            tab = torch.from_numpy(fj.view(np.uint8)).to(dev)
            _lib.check(self.lib.cf_bin_regions_multi(C.c_void_p(tab.data_ptr()), len(regs), F, nres, self.cb, self.cl, int(max_cols),
                                                     self.stream.cuda_stream), "cf_bin_regions_multi")

    def model_args(self):
        """The six arguments of model(...) / model.integrated_gradients(...)."""
        bs = self.binsizes
        return ({b: self.pf[r] for r, b in enumerate(bs)}, {b: self.pm[r] for r, b in enumerate(bs)},
                {b: self.cf[r] for r, b in enumerate(bs)}, {b: self.cm[r] for r, b in enumerate(bs)},
                {b: self.im for b in bs}, self.freq)

    def backward(self, dp, dc, times_input):
        """cf_bin_regions_multi_backward with dfeat pointing into dp[r] [B, 1, L, F] / dc[r] [B, S, L, F] -> the tracks, host float32."""
        import torch

        from . import _lib
        from .data import BIN_GRAD_JOB
        regs, fj, order, draw = self.regs, self.fj, self.order, self.draw
        with torch.cuda.device(self.dev):
            bj = np.zeros(len(regs), dtype=BIN_GRAD_JOB)
            for k, (i, s, flip, a, c0, nc, off, ooff, ld_out) in enumerate(regs):
                for name in ("raw", "ld", "col0", "ncols", "flip"):
                    bj[k][name] = fj[k][name]
                for r in range(self.nres):
                    bj[k]["dfeat"][order.index(r)] = (dp[r][i, 0] if s < 0 else dc[r][i, s]).data_ptr()
                bj[k]["draw"], bj[k]["ld_out"] = draw.data_ptr() + 4 * ooff, ld_out
            tab2 = torch.from_numpy(bj.view(np.uint8)).to(self.dev)
            _lib.check(self.lib.cf_bin_regions_multi_backward(C.c_void_p(tab2.data_ptr()), len(regs), self.F, self.nres, self.cb, self.cl,
                                                              int(self.max_cols), 1 if times_input else 0, self.stream.cuda_stream),
                       "cf_bin_regions_multi_backward")
            return draw.cpu().numpy()

    def spread(self, donor, mp, mc):
        """cf_bin_spread_difference between this chunk's raw regions and those of `donor` (a _RawChunk of the same genes in another
        dataset over the same regions), cmean pointing into mp[r] [B, 1, L, F] / mc[r] [B, S, L, F] -> the tracks, host float32."""
        import torch

        from . import _lib
        from .data import BIN_SPREAD_JOB
        regs, fj, order, draw = self.regs, self.fj, self.order, self.draw
        if len(donor.regs) != len(regs) or any((a[0], a[1], a[4], a[5]) != (b[0], b[1], b[4], b[5]) for a, b in zip(regs, donor.regs)):
            raise ValueError("the donor's raw regions do not cover the same windows as the dataset's")
        with torch.cuda.device(self.dev):
            sj = np.zeros(len(regs), dtype=BIN_SPREAD_JOB)
            for k, (i, s, flip, a, c0, nc, off, ooff, ld_out) in enumerate(regs):
                for name in ("raw", "ld", "col0", "ncols", "flip"):
                    sj[k][name] = fj[k][name]
                sj[k]["raw_donor"], sj[k]["ld_donor"] = donor.fj[k]["raw"], donor.fj[k]["ld"]
                for r in range(self.nres):
                    sj[k]["cmean"][order.index(r)] = (mp[r][i, 0] if s < 0 else mc[r][i, s]).data_ptr()
                sj[k]["draw"], sj[k]["ld_out"] = draw.data_ptr() + 4 * ooff, ld_out
            tab = torch.from_numpy(sj.view(np.uint8)).to(self.dev)
            _lib.check(self.lib.cf_bin_spread_difference(C.c_void_p(tab.data_ptr()), len(regs), self.F, self.nres, self.cb, self.cl,
                                                         int(self.max_cols), self.stream.cuda_stream), "cf_bin_spread_difference")
            return draw.cpu().numpy()

    def scatter(self, host, per):
        """The tracks of `host` into the per-gene dicts `per` (promoter, pcres, regions), genomic coordinates."""
        ds, ids, F = self.ds, self.ids, self.F
        for i, s, flip, a, c0, nc, off, ooff, ld_out in self.regs:
            track = host[ooff:ooff + F * ld_out].reshape(F, ld_out)[:, :nc].copy()
            g = ds.genes[ids[i]]
            if s < 0:
                chrom, tss, _ = g["tss"]
                per[i]["promoter"] = track
                per[i]["regions"].append((chrom, tss - 20000 + c0, tss - 20000 + c0 + nc))
            else:
                per[i]["pcres"].append(track)
                per[i]["regions"].append(tuple(g["pcres"][s]))
        return per


def raw_signal_gradients(model, dataset, genes=None, target=None, times_input=False, bsz=None):
    """Raw-signal saliency: the gradient of logit column `target` (default: 1 for the classifier, 0 for the regressor) with respect to
    the RAW histone signals of a ChromoformerDataset -- the fp16 [F, len] .npy regions, at their own resolution and in genomic
    orientation -- by the exact chain rule on one backward pass.  A generator over `genes` (ids; default: the dataset's), working in
    chunks of at most min(bsz, model.max_batch) genes; per chunk

        raw regions -> HBM -> cf_bin_regions_multi -> model(...) with the binned features as leaves -> logits[:, target].sum().backward()
        (cf_backward_from_inputs) -> cf_bin_regions_multi_backward with dfeat pointing into the .grad tensors

    and per gene it yields a dict of host arrays:

        gene_id    the id
        logits     float32 [n_out]
        promoter   float32 [F, window]: the window of the promoter file the dataset bins (w_prom-narrowed), genomic orientation (the mirror
                   of a '-' strand promoter is undone)
        pcres      list of float32 [F, len_s], one per pCRE, in the order of the metadata
        regions    [(chrom, start, end)] of the promoter window and of every pCRE: sample s of a track is position start + s

    times_input: gradient x input (each value multiplied by the raw sample).  Gradient and gradient x input only: integrated gradients
    in raw space is a different path integral (log(1 + x) is not linear) and is not what this computes -- raw_integrated_gradients
    below does.  Parameters, their .grad and the optimiser state are left as they are; the pass overwrites the activations a
    grad-enabled model(...) keeps for its backward."""
    import torch
    ds = dataset
    binsizes, n_bins, target, genes, chunk = _raw_check("raw_signal_gradients", model, ds, genes, target, bsz)
    for lo in range(0, len(genes), chunk):
        ids = genes[lo:lo + chunk]
        ch = _RawChunk(model, ds, ids, binsizes, n_bins)
        pf, cf = ch.pf, ch.cf
        with torch.cuda.device(ch.dev):
            # the backward of the model writes the flat gradient buffer and publishes it as the parameters' .grad: both are put back
            named = model._named()
            kept = {k: p.grad for k, p in named.items()}
            kept_flat, kept_top = model._gflat.clone(), getattr(model, "_grads_top", None)
            try:
                for t in pf + cf:
                    t.requires_grad_(True)
                with torch.enable_grad():
                    logits = model(*ch.model_args())
                    logits[:, target].sum().backward()
            finally:
                model._gflat.copy_(kept_flat)
                for k, p in named.items():
                    p.grad = kept[k]
                model._grads_top = kept_top
            dp, dc = [t.grad for t in pf], [t.grad for t in cf]
            if any(t is None or not t.is_contiguous() for t in dp + dc):
                raise RuntimeError("raw_signal_gradients: the backward pass left no gradient for a binned input")
            host = ch.backward(dp, dc, times_input)
            lg = logits.detach().cpu().numpy()
        per = [dict(gene_id=gene, logits=lg[i].copy(), promoter=None, pcres=[], regions=[]) for i, gene in enumerate(ids)]
        for d in ch.scatter(host, per):
            yield d


def raw_integrated_gradients(model, dataset, genes=None, target=None, n_steps=50, method="gausslegendre", bsz=None, donor_dataset=None):
    """Integrated gradients in raw-signal space: the attribution of logit column `target` (default: 1 for the classifier, 0 for the
    regressor) to every sample of the RAW histone signals of a ChromoformerDataset, along the path a * x from the zero signal, with the
    nodes and weights of ig_quadrature(method, n_steps).  Binning is linear and followed by log(1 + .), so along the path a bin of
    mean m has the feature log1p(a m), and with g_k the input gradient at node k and C = sum_k g_k / (1 + a_k m):

        attr  = m * C                                             per bin: IG with respect to the bin mean (complete)
        IG_raw[f, s] = x[f, s] * sum_r C_r[p_r(s), f] / cnt       per sample: each bin's attr spread over its samples in proportion to x

    A generator over `genes` like raw_signal_gradients, in chunks of at most min(bsz, model.max_batch) genes; per chunk

        raw regions -> HBM -> cf_bin_regions_multi -> cf_integrated_gradients_raw over the features (frequencies and masks held at the
        gene's) -> cf_bin_regions_multi_backward(times_input = 1) with dfeat pointing at its `coeff` = (1 + m) * C

    and per gene it yields the dict of raw_signal_gradients (gene_id, logits, promoter, pcres, regions; the tracks now hold IG_raw) plus

        baseline_logits   float32 [n_out]: the prediction on the zero signal (same masks and frequencies)
        delta             float32 scalar: sum of the per-bin attr - (logits - baseline_logits)[target], the quadrature error; the tracks
                          sum to the same total up to fp32 rounding

    donor_dataset: a ChromoformerDataset of another cell type over the same regions (same_regions runs first).  The baseline is then
    that cell type's signal xd and the path xd + a (x - xd): a bin with means m, md has the feature log1p(md + a (m - md)), and with
    C = sum_k g_k / (1 + md + a_k (m - md))

        attr  = (m - md) * C                                      per bin (complete: sums to F(x) - F(xd))
        IG_raw[f, s] = (x[f, s] - xd[f, s]) * sum_r C_r[p_r(s), f] / cnt      per sample, coarsest resolution first

    by cf_integrated_gradients_raw_donor and cf_bin_spread_difference on both chunks' raw buffers.  baseline_logits is then the donor's
    signal under the gene's masks and frequencies, and each dict gains

        donor_prediction  float32 [n_out]: the donor dataset's own plain forward of the gene (its masks, its frequencies)

    A sample where the two signals agree gets exactly 0.

    Limits: without a donor the zero-signal baseline; binned features below ~80 (expm1 in fp32; preprocessed signals are far below); a
    negative signal with 1 + a m <= 0 gives inf / NaN as the forward's log does.  Parameters, their .grad, the flat gradient buffer and
    the optimiser state are left as they are; the pass overwrites the activations a grad-enabled model(...) keeps for its backward."""
    import torch
    ds = dataset
    binsizes, n_bins, target, genes, chunk = _raw_check("raw_integrated_gradients", model, ds, genes, target, bsz)
    ig_quadrature(method, n_steps)      # (refuses an unknown method or node count before anything is loaded)
    if donor_dataset is not None:
        same_regions(ds, donor_dataset, genes)
    for lo in range(0, len(genes), chunk):
        ids = genes[lo:lo + chunk]
        ch = _RawChunk(model, ds, ids, binsizes, n_bins)
        if donor_dataset is not None:
            dch = _RawChunk(model, donor_dataset, ids, binsizes, n_bins)
            with torch.cuda.device(ch.dev):
                with torch.no_grad():
                    dp = model(*dch.model_args()).cpu().numpy()
                attr, info = model.integrated_gradients(*ch.model_args(), target=target, n_steps=n_steps, method=method,
                                                        inputs=("promoter_feats", "pcre_feats"), path="signal",
                                                        donor=({b: dch.pf[r] for r, b in enumerate(binsizes)},
                                                               {b: dch.cf[r] for r, b in enumerate(binsizes)}))
                cm = info["cmean"]
                host = ch.spread(dch, [cm["promoter_feats"][b] for b in binsizes], [cm["pcre_feats"][b] for b in binsizes])
                lg, lb, dl = (info[k].cpu().numpy() for k in ("logits", "baseline_logits", "delta"))
            per = [dict(gene_id=gene, logits=lg[i].copy(), baseline_logits=lb[i].copy(), delta=dl[i].copy(), donor_prediction=dp[i].copy(),
                        promoter=None, pcres=[], regions=[]) for i, gene in enumerate(ids)]
            for d in ch.scatter(host, per):
                yield d
            continue
        with torch.cuda.device(ch.dev):
            attr, info = model.integrated_gradients(*ch.model_args(), target=target, n_steps=n_steps, method=method,
                                                    inputs=("promoter_feats", "pcre_feats"), path="signal")
            co = info["coeff"]
            host = ch.backward([co["promoter_feats"][b] for b in binsizes], [co["pcre_feats"][b] for b in binsizes], True)
            lg, lb, dl = (info[k].cpu().numpy() for k in ("logits", "baseline_logits", "delta"))
        per = [dict(gene_id=gene, logits=lg[i].copy(), baseline_logits=lb[i].copy(), delta=dl[i].copy(), promoter=None, pcres=[], regions=[])
               for i, gene in enumerate(ids)]
        for d in ch.scatter(host, per):
            yield d


def scan_windows(start, end, binsize, width, n_win):
    """Genomic [start, end) of windows 0 .. n_win - 1 of a region [start, end): window g begins at start + g * binsize and spans
    `width` coarsest bins, its end clipped to the region -> int64 [n_win, 2]."""
    g = np.arange(int(n_win), dtype=np.int64)
    lo = int(start) + g * int(binsize)
    return np.stack([lo, np.minimum(lo + int(width) * int(binsize), int(end))], axis=1).reshape(-1, 2)


def scan_mark_sets(mark_sets, n_feats):
    """The mark sets of a scan as a list of tuples of mark indices; None: each mark alone, then all marks together (n_feats + 1 sets)."""
    if mark_sets is None:
        mark_sets = [(f,) for f in range(n_feats)] + [tuple(range(n_feats))]
    return [tuple(int(f) for f in ms) for ms in mark_sets]


def scan_regions_expand(regions, i_max, who="perturbation_scan"):
    """The scanned regions as a sorted list of region indices (0 the promoter, 1 + j pCRE slot j): "promoter" -> [0], "all" ->
    [0 .. i_max], "pcres" -> [1 .. i_max], or an iterable of indices (duplicates dropped).  Raises ValueError on anything else."""
    S = int(i_max)
    if isinstance(regions, str):
        named = {"promoter": [0], "all": list(range(S + 1)), "pcres": list(range(1, S + 1))}
        if regions not in named:
            raise ValueError("%s: regions %r; choose 'promoter', 'all', 'pcres' or a list of region indices" % (who, regions))
        return named[regions]
    regions = sorted({int(r) for r in regions})
    if not regions or regions[0] < 0 or regions[-1] > S:
        raise ValueError("%s: regions %s outside [0, i_max = %d]" % (who, regions, S))
    return regions


def scan_row(q, k, g, n_sets, W):
    """Row of (block q of the scanned regions, mark set k, window g) in the flattened [n_reg * V] rows of a scan, V = 1 + n_sets * W;
    k = None: the block's unperturbed row."""
    V = 1 + int(n_sets) * int(W)
    if k is None:
        return int(q) * V
    if not (0 <= k < n_sets and 0 <= g < W):
        raise ValueError("scan_row: set %d / window %d outside [0, %d) x [0, %d)" % (k, g, n_sets, W))
    return int(q) * V + 1 + int(k) * int(W) + int(g)


def scan_row_inverse(row, n_sets, W):
    """The inverse of scan_row: row -> (q, k, g), or (q, None, None) for a block's unperturbed row."""
    V = 1 + int(n_sets) * int(W)
    q, v = divmod(int(row), V)
    if v == 0:
        return q, None, None
    k, g = divmod(v - 1, int(W))
    return q, k, g


def _resident_store(who, ds, genes, binsizes, dev, store=None):
    """The binned features of `genes` on the device: `store` (a device-resident GeneStore holding `genes` in order) if given, else the
    packed store next to the raw files if one matches, else the raw .npy files binned on the device."""
    import copy

    from . import pack
    from .data import GeneStore
    if store is None:
        packed = pack.find(ds.npy_dir, None, binsizes, ds.i_max, ds.w_prom, ds.w_max, ds.n_feats, genes, meta=ds.meta)
        if packed is not None:
            store = packed.store(genes, device=dev, regression=False)
        else:
            sub = copy.copy(ds)
            sub.target_genes = genes
            store = GeneStore(sub, device=dev, resident=True)
    if len(store) != len(genes):
        raise ValueError("%s: the store holds %d genes, `genes` names %d" % (who, len(store), len(genes)))
    return store


def _open(who, model, dataset, genes, bsz, donor_dataset=None):
    """The opening of the dataset generators -> (binsizes, n_bins, genes, chunk size): the model is on the device and the dataset has
    its geometry, the genes are in its metadata and, with a donor dataset, both hold them over the same regions.  Host checks only."""
    binsizes = [int(b) for b in dataset.binsizes]
    n_bins = _geometry_check(who, model, dataset, binsizes)
    genes, chunk = _genes_check(who, model, dataset, genes, bsz)
    if donor_dataset is not None:
        same_regions(dataset, donor_dataset, genes)
    return binsizes, n_bins, genes, chunk


def _batches(who, model, dataset, genes, chunk, binsizes, store=None, donor_dataset=None, donor_store=None):
    """The resident stores of the dataset and, if given, of the donor (_resident_store), then per chunk of `genes` -> (the gene ids,
    their store indices, the batch dict, forward()'s six arguments, the donor pair or None, the donor's batch dict or None).  A
    generator: nothing is loaded before the first next(), so a caller's refusals come first."""
    store = _resident_store(who, dataset, genes, binsizes, model._device, store)
    if donor_dataset is not None:
        donor_store = _resident_store(who, donor_dataset, genes, binsizes, model._device, donor_store)
    for lo in range(0, len(genes), chunk):
        ids = genes[lo:lo + chunk]
        idx = list(range(lo, lo + len(ids)))
        d = store.batch(idx)
        dd = donor_store.batch(idx) if donor_dataset is not None else None
        yield ids, idx, d, tuple(d[k] for k in _BATCH_KEYS), None if dd is None else _donor_pair(dd), dd


def _exact_game(model, prefix, args, kw, interactions, dividends, methods=None):
    """One exact game of a batch (prefix "mark", "mark_donor", "mark_window" or "mark_fine_window"; "contact" with `methods`, the
    holder of <prefix>_shapley and <prefix>_shapley_interactions where that is not the model) -> (phi, interactions or None, info,
    dividends, mass): one model.<prefix>_shapley(*args, **kw), or with `interactions` (an index name) one
    model.<prefix>_shapley_interactions in its place, phi from info["phi"]; with `dividends` the call keeps its coalition table and
    model.shapley_dividends turns it into (dividends, mass) [B, 2^P, n_out], else (None, None).  Host arrays but for info, the call's."""
    methods = model if methods is None else methods
    if interactions is None:
        inter, (phi, info) = None, getattr(methods, prefix + "_shapley")(*args, return_coalitions=bool(dividends), **kw)
    else:
        inter, info = getattr(methods, prefix + "_shapley_interactions")(*args, index=interactions, return_coalitions=bool(dividends), **kw)
        phi, inter = info["phi"], inter.cpu().numpy()
    div, mass = None, None
    if dividends:
        div, mass = (t.cpu().numpy() for t in model.shapley_dividends(info["coalitions"], return_mass=True))
    return phi.cpu().numpy(), inter, info, div, mass


def _optional_keys(out, i, eps=None, interactions=None, dividends=None, mass=None):
    """Gene i's rows of a batch's optional arrays into its dict `out`, each under its argument's name where it is given -> out."""
    for key, a in (("eps", eps), ("interactions", interactions), ("dividends", dividends), ("mass", mass)):
        if a is not None:
            out[key] = a[i].copy()
    return out


def perturbation_scan(model, dataset, genes=None, regions="promoter", scale=0.0, width=1, mark_sets=None, bsz=None, store=None):
    """In-silico perturbation scan of the genes of a ChromoformerDataset (one model.perturbation_scan_regions per batch, windows in
    genomic coordinates): what the prediction becomes with the marks of a mark set scaled by `scale` in raw-signal space -- 0 erases, 2
    doubles -- over each window of `width` coarsest bins of a region.  A generator over `genes` (ids; default: the dataset's) in
    chunks of at most min(bsz, model.max_batch) genes; per gene it yields a dict of host arrays:

        gene_id    the id
        logits     float32 [n_out]: the unperturbed prediction
        mark_sets  the sets, tuples of mark indices (default: each mark alone, then all together)
        regions    [(chrom, start, end)] of the scanned regions the gene has: the promoter window (start = tss - 20000 +
                   promoter_col0), then its pCREs
        windows    per region int64 [n_win, 2]: genomic start and end of each REAL window, start + g * binsize_c, the end clipped to
                   the region
        scan       per region float32 [n_sets, n_win, n_out]: the logits with set k scaled over window g, genomic order

    regions: "promoter", "all" (the promoter and every pCRE the gene has), "pcres" or a list of region indices (0 the promoter, 1 + j pCRE
    slot j; a slot the gene does not have is left out).  Strand and coordinates come from the dataset's metadata ('-' strand promoters
    are stored mirrored: window 0 is still the genomic start).  The binned features come from `store` (a device-resident GeneStore
    holding `genes` in order) if given, else from the packed store next to the raw files if one matches, else from the raw .npy
    files binned on the device: the raw files are not required.  Parameters, gradients and optimiser state are left as they are; the
    pass overwrites the activations a grad-enabled model(...) keeps for its backward."""
    import torch

    from .data import promoter_col0
    ds = dataset
    binsizes, n_bins, genes, chunk = _open("perturbation_scan", model, ds, genes, bsz)
    S, F = ds.i_max, ds.n_feats
    order = scan_regions_expand(regions, S) if isinstance(regions, str) else [int(r) for r in regions]      # (the caller's order is kept)
    regions = scan_regions_expand(order, S)
    mark_sets = scan_mark_sets(mark_sets, F)
    rc = int(np.argmin(n_bins))
    W, bc = n_bins[rc], binsizes[rc]
    col0 = promoter_col0(ds)
    for ids, _, d, args, _, _ in _batches("perturbation_scan", model, ds, genes, chunk, binsizes, store):
        B = len(ids)
        flip = [ds.genes[g]["tss"][2] != "+" for g in ids]
        per = [dict(gene_id=g, logits=None, mark_sets=list(mark_sets), regions=[], windows=[], scan=[]) for g in ids]
        has_of = {region: [region == 0 or region - 1 < len(ds.genes[g]["pcres"]) for g in ids] for region in regions}
        live = [region for region in regions if any(has_of[region])]      # (a slot no gene of the chunk has is not scanned)
        blocks = None
        if live:
            blocks, _ = model.perturbation_scan_regions(*args, regions=live, scale=scale, width=width, mark_sets=mark_sets, flip=flip)
            blocks = blocks.cpu().numpy()
        K = len(mark_sets)
        for region in (r for r in order if r in live):
            has, out = has_of[region], blocks[live.index(region)]
            m = (d["promoter_pad_masks"][bc] if region == 0 else d["pcre_pad_masks"][bc][:, region - 1]).reshape(B, W).cpu().numpy() == 0
            for i, g in enumerate(ids):
                per[i]["logits"] = out[i, scan_row(0, None, None, K, W)].copy()
                if not has[i]:
                    continue
                real = np.flatnonzero(m[i])
                n_win = int(real[-1] - real[0] + 1) if real.size else 0
                reg = _gene_region(ds, g, region, col0)
                per[i]["regions"].append(reg)
                per[i]["windows"].append(scan_windows(reg[1], reg[2], bc, width, n_win))
                per[i]["scan"].append(out[i, scan_row(0, 0, 0, K, W):].reshape(K, W, -1)[:, :n_win].copy())
        if per[0]["logits"] is None:      # (no gene of the chunk has any of the regions: the prediction alone)
            with torch.no_grad():
                out = model(*args).cpu().numpy()
            for i in range(B):
                per[i]["logits"] = out[i].copy()
        for p in per:
            yield p


def fine_scan_windows(chrom, start, end, binsize, first, width, stride, n_win):
    """Genomic windows of a fine scan of the region [start, end): window g begins at start + (first + g * stride) * binsize and spans
    `width` finest bins, its end clipped to the region; only windows that begin inside the region -> [(chrom, start, end)]."""
    out = []
    for g in range(int(n_win)):
        lo = int(start) + (int(first) + g * int(stride)) * int(binsize)
        if lo >= end:
            break
        out.append((chrom, lo, min(lo + int(width) * int(binsize), int(end))))
    return out


def perturbation_scan_fine(model, dataset, genes=None, region="promoter", zoom=None, scale=0.0, width=1, stride=None, mark_sets=None,
                           target=None, bsz=None, store=None):
    """Fine-resolution perturbation scan of the genes of a ChromoformerDataset (model.perturbation_scan_fine per batch, windows in
    genomic coordinates): what the prediction becomes with the marks of a mark set scaled by `scale` in raw-signal space over each
    window of `width` FINEST bins of one region, windows `stride` (default: width) finest bins apart.  A generator over `genes` (ids;
    default: the dataset's) in chunks of at most min(bsz, model.max_batch) genes; per gene it yields a dict:

        gene_id    the id
        logits     float32 [n_out]: the unperturbed prediction
        mark_sets  the sets, tuples of mark indices (default: each mark alone, then all together)
        region     (chrom, start, end) of the scanned region, None if the gene does not have it (windows and scan are then empty)
        windows    [(chrom, start, end)]: each window in genomic coordinates, the end clipped to the region
        scan       float32 [n_sets, n_win, n_out]: the logits with set k scaled over window g, in the order of `windows`

    region: "promoter" or a pCRE slot j (an int).  zoom = None scans the whole region.  zoom = k first runs the coarse scan
    (model.perturbation_scan, width 1) and fine-scans, per gene, the k coarse windows in which some mark set moves logit `target`
    (default: the last) the most -- one model.perturbation_scan_fine per rank, each gene at its own start; `windows` / `scan` then hold the
    fine windows of rank 0, then of rank 1, ..., and the dict also carries

        zoom           int64 [k']: the chosen coarse windows, most important first (k' = min(k, the region's real coarse windows))
        coarse_windows [(chrom, start, end)] and coarse_scan float32 [n_sets, n_cwin, n_out]: the coarse scan

    Strand and the region's length come from the dataset's metadata: '-' strand promoters are stored mirrored (window 0 is still the
    genomic start), and the short last bin of a pCRE is weighted by the samples it holds.  Features, parameters and the effect on a
    pending backward: as perturbation_scan."""
    from .data import promoter_col0
    who = "perturbation_scan_fine"
    ds = dataset
    binsizes, n_bins, genes, chunk = _open(who, model, ds, genes, bsz)
    S, F = ds.i_max, ds.n_feats
    region = _region_index(who, region, S)
    mark_sets = scan_mark_sets(mark_sets, F)
    K = len(mark_sets)
    width = int(width)
    stride = width if stride is None else int(stride)
    if width < 1 or stride < 1:
        raise ValueError("%s: width = %d, stride = %d: at least 1 finest bin each" % (who, width, stride))
    if zoom is not None and int(zoom) < 1:
        raise ValueError("%s: zoom = %r: at least 1 coarse window, or None" % (who, zoom))
    rf, rc = int(np.argmin(binsizes)), int(np.argmin(n_bins))
    Lf, bf, W, bc = n_bins[rf], binsizes[rf], n_bins[rc], binsizes[rc]
    Rc = Lf // W
    target = model.n_out - 1 if target is None else int(target)
    col0 = promoter_col0(ds)
    for ids, _, _, args, _, _ in _batches(who, model, ds, genes, chunk, binsizes, store):
        flip = [region == 0 and ds.genes[g]["tss"][2] != "+" for g in ids]
        regs = [_gene_region(ds, g, region, col0) for g in ids]
        lengths = [r[2] - r[1] if r else 0 for r in regs]
        kw = dict(region=region, scale=scale, width=width, stride=stride, mark_sets=mark_sets, lengths=lengths, flip=flip)
        per = [dict(gene_id=g, logits=None, mark_sets=list(mark_sets), region=regs[i], windows=[], scan=np.zeros((K, 0, model.n_out), np.float32))
               for i, g in enumerate(ids)]
        if zoom is None:
            n_win = -(-Lf // stride)
            out = model.perturbation_scan_fine(*args, n_windows=n_win, **kw).cpu().numpy()
            for i, r in enumerate(regs):
                per[i]["logits"] = out[i, 0].copy()
                if r:
                    per[i]["windows"] = fine_scan_windows(r[0], r[1], r[2], bf, 0, width, stride, n_win)
                    per[i]["scan"] = out[i, 1:].reshape(K, n_win, -1)[:, :len(per[i]["windows"])].copy()
        else:
            coarse = model.perturbation_scan(*args, region=region, scale=scale, width=1, mark_sets=mark_sets, flip=flip).cpu().numpy()
            ranks = []
            for i, r in enumerate(regs):
                per[i]["logits"] = coarse[i, 0].copy()
                n_cw = -(-(r[2] - r[1]) // bc) if r else 0
                cs = coarse[i, 1:].reshape(K, W, -1)[:, :n_cw]
                moved = np.abs(cs[..., target] - coarse[i, 0, target]).max(axis=0) if n_cw else np.zeros(0)
                ranks.append(np.argsort(-moved, kind="stable")[:int(zoom)].astype(np.int64))
                per[i]["zoom"] = ranks[i]
                per[i]["coarse_windows"] = [(r[0], int(a), int(b)) for a, b in scan_windows(r[1], r[2], bc, 1, n_cw)] if r else []
                per[i]["coarse_scan"] = cs.copy()
            n_win = -(-Rc // stride)
            for rank in range(max([len(z) for z in ranks] + [0])):
                # a gene with fewer real coarse windows than ranks starts past its region: the baseline's rows, left out below
                start = [int(z[rank]) * Rc if rank < len(z) else Lf for z in ranks]
                out = model.perturbation_scan_fine(*args, start=start, n_windows=n_win, **kw).cpu().numpy()
                for i, r in enumerate(regs):
                    if rank < len(ranks[i]):
                        wins = fine_scan_windows(r[0], r[1], r[2], bf, start[i], width, stride, n_win)
                        per[i]["windows"] += wins
                        per[i]["scan"] = np.concatenate([per[i]["scan"], out[i, 1:].reshape(K, n_win, -1)[:, :len(wins)]], axis=1)
        for p in per:
            yield p


def mark_shapley(model, dataset, genes=None, players="marks", scale=0.0, epistasis=False, bsz=None, store=None, interactions=None,
                 dividends=False):
    """Exact Shapley values of the histone marks for the genes of a ChromoformerDataset (one model.mark_shapley per batch, with
    epistasis=True also one model.mark_epistasis): which marks carry the prediction when an absent mark's raw signal is scaled by
    `scale` (0 erases it) over the regions of its player.  A generator over `genes` (ids; default: the dataset's) in chunks of at most
    min(bsz, model.max_batch) genes; per gene it yields a dict of host arrays:

        gene_id   the id
        phi       float32 [P, n_out]: the players' Shapley values, in logit space; phi.sum(0) = logits - erased up to rounding
        logits    float32 [n_out]: the prediction (every player present)
        erased    float32 [n_out]: every player absent
        players   the players' names (mark_players)
        eps       float32 [P, P, n_out], with epistasis=True: the pair epistasis, the leave-one-out effects on the diagonal
        interactions  float32 [P, P, n_out], with interactions="sii" / "sti": the pairwise Shapley interaction index; the batch then makes
                  one model.mark_shapley_interactions call in place of model.mark_shapley (the 2^P forwards run once; phi keeps its bits)
        dividends, mass  float32 [2^P, n_out] each, with dividends=True: the Harsanyi dividend of every set of players, word m at row m
                  (set_names names them), and the scale of its rounding error (dividend_bound); model.shapley_dividends on the table of
                  the batch's one Shapley call: no forward is added

    players: "marks", "compartments", "regions" or a list of (marks, regions) pairs (mark_players).  The binned features come from
    `store` (a device-resident GeneStore holding `genes` in order) if given, else from the packed store next to the raw files if one
    matches, else from the raw .npy files binned on the device.  Parameters, gradients and optimiser state are left as they are; the
    pass overwrites the activations a grad-enabled model(...) keeps for its backward."""
    ds = dataset
    binsizes, _, genes, chunk = _open("mark_shapley", model, ds, genes, bsz)
    spec = players if isinstance(players, str) else list(players)
    names = mark_players(spec, ds.n_feats, ds.i_max)[2]      # (refusals before anything is loaded)
    if interactions is not None:
        interaction_index(interactions, "mark_shapley")
    for ids, _, _, args, _, _ in _batches("mark_shapley", model, ds, genes, chunk, binsizes, store):
        phi, inter, info, div, mass = _exact_game(model, "mark", args, dict(players=spec, scale=scale), interactions, dividends)
        logits, erased = info["logits"].cpu().numpy(), info["erased"].cpu().numpy()
        eps = model.mark_epistasis(*args, players=spec, scale=scale)[0].cpu().numpy() if epistasis else None
        for i, g in enumerate(ids):
            out = dict(gene_id=g, phi=phi[i].copy(), logits=logits[i].copy(), erased=erased[i].copy(), players=list(names))
            yield _optional_keys(out, i, eps, inter, div, mass)


def same_regions(dataset, donor_dataset, genes=None):
    """The donor rule replaces a mark's signal over a region by the other cell type's signal over the SAME region: both datasets must
    read the genes' promoters and pCREs at the same coordinates with the same geometry.  A pure host check (no device): raises
    ValueError naming the geometry fields that differ (binsizes, w_max, w_prom, i_max, n_feats), genes the donor's metadata does not
    hold, or up to five genes whose TSS, strand or pCRE list differ.  -> the genes checked (default: the dataset's)."""
    ds, dn = dataset, donor_dataset
    diff = []
    for field in ("binsizes", "w_max", "w_prom", "i_max", "n_feats"):
        a, b = getattr(ds, field), getattr(dn, field)
        a, b = ([int(x) for x in a], [int(x) for x in b]) if field == "binsizes" else (int(a), int(b))
        if a != b:
            diff.append("%s %s != %s" % (field, a, b))
    if diff:
        raise ValueError("same_regions: the datasets differ in geometry: %s" % ", ".join(diff))
    genes = list(ds.target_genes if genes is None else genes)
    missing = [g for g in genes if g not in ds.genes or g not in dn.genes]
    if missing:
        raise ValueError("same_regions: gene(s) %s are not in both datasets' metadata (%d in all)" % (missing[:5], len(missing)))
    bad = []
    for g in genes:
        a, b = ds.genes[g], dn.genes[g]
        what = [name for name, same in (("tss", a["tss"][:2] == b["tss"][:2]), ("strand", a["tss"][2] == b["tss"][2]),
                                        ("pcres", [tuple(p) for p in a["pcres"]] == [tuple(p) for p in b["pcres"]])) if not same]
        if what:
            bad.append("%s (%s)" % (g, ", ".join(what)))
    if bad:
        raise ValueError("same_regions: %d gene(s) do not have the same regions in the two datasets: %s%s"
                         % (len(bad), "; ".join(bad[:5]), " ..." if len(bad) > 5 else ""))
    return genes


def mark_donor_shapley(model, dataset, donor_dataset, genes=None, players="marks", epistasis=False, bsz=None, store=None, donor_store=None,
                       interactions=None, dividends=False):
    """Exact Shapley values of the histone marks against a donor cell type, for the genes of two ChromoformerDatasets over the same
    regions (same_regions): one model.mark_donor_shapley per batch, with epistasis=True also one model.mark_donor_epistasis -- which
    mark changes account for the difference between the prediction in `dataset` and in `donor_dataset`?  A generator over `genes`
    (ids; default: the dataset's) in chunks of at most min(bsz, model.max_batch) genes; per gene it yields a dict of host arrays:

        gene_id            the id
        phi                float32 [P, n_out]: the players' Shapley values, in logit space; phi.sum(0) = logits - donor up to rounding
        logits             float32 [n_out]: the prediction (every player present)
        donor              float32 [n_out]: every player's marks from the donor, under the gene's masks and frequencies
        donor_prediction   float32 [n_out]: the plain forward of the donor's own batch, with its own frequencies: donor_prediction -
                           donor is what the marks of the players do not explain
        players            the players' names (mark_players)
        eps                float32 [P, P, n_out], with epistasis=True: the pair epistasis, the leave-one-out effects on the diagonal
        interactions       float32 [P, P, n_out], with interactions="sii" / "sti": the pairwise Shapley interaction index; the batch then
                           makes one model.mark_donor_shapley_interactions call in place of model.mark_donor_shapley
        dividends, mass    float32 [2^P, n_out] each, with dividends=True: as in mark_shapley

    players as in mark_shapley.  The binned features come from `store` / `donor_store` (device-resident GeneStores holding `genes` in
    order) if given, else from the packed store next to each dataset's raw files if one matches, else from the raw .npy files binned
    on the device.  Parameters, gradients and optimiser state are left as they are; the pass overwrites the activations a
    grad-enabled model(...) keeps for its backward."""
    import torch
    ds, dn = dataset, donor_dataset
    who = "mark_donor_shapley"
    binsizes, _, genes, chunk = _open(who, model, ds, genes, bsz, dn)
    spec = players if isinstance(players, str) else list(players)
    names = mark_players(spec, ds.n_feats, ds.i_max)[2]      # (refusals before anything is loaded)
    if interactions is not None:
        interaction_index(interactions, who)
    for ids, _, _, args, donor, dd in _batches(who, model, ds, genes, chunk, binsizes, store, dn, donor_store):
        phi, inter, info, div, mass = _exact_game(model, "mark_donor", args, dict(donor=donor, players=spec), interactions, dividends)
        logits, don = info["logits"].cpu().numpy(), info["donor"].cpu().numpy()
        eps = model.mark_donor_epistasis(*args, donor=donor, players=spec)[0].cpu().numpy() if epistasis else None
        with torch.no_grad():
            pred = model(*(dd[k] for k in _BATCH_KEYS)).cpu().numpy()
        for i, g in enumerate(ids):
            out = dict(gene_id=g, phi=phi[i].copy(), logits=logits[i].copy(), donor=don[i].copy(), donor_prediction=pred[i].copy(),
                       players=list(names))
            yield _optional_keys(out, i, eps, inter, div, mass)


def contact_shapley(model, dataset, donor_dataset=None, genes=None, players="contacts", scale=0.0, marks="own", epistasis=False,
                    interactions=None, dividends=False, bsz=None, store=None, donor_store=None):
    """Exact Shapley values of contact players for the genes of a ChromoformerDataset (one contact.contact_shapley per batch, with
    epistasis=True also one contact.contact_epistasis): does a pCRE matter through its chromatin state or through its contact with the
    promoter?  An absent player deletes its pCRE slots and / or edits their promoter contact frequencies (contact_players): scaled by
    `scale` (0 erases the contact, the default), or, with `donor_dataset` (another cell type over the same regions: same_regions runs
    first), replaced by the donor's frequencies.  A generator over `genes` (ids; default: the dataset's) in chunks of at most
    min(bsz, model.max_batch) genes; per gene it yields a dict of host arrays:

        gene_id            the id
        phi                float32 [P, n_out]: the players' Shapley values, in logit space; phi.sum(0) = logits - erased (or - donor) up
                           to rounding; exactly 0 for a dummy slot's players
        logits             float32 [n_out]: every player present
        erased             float32 [n_out], without a donor dataset: every player absent
        donor              float32 [n_out], with a donor dataset: every player absent (its contacts the donor's)
        players            the players' names (contact_players)
        freq               float32 [i_max]: the gene's promoter-pCRE contact frequencies, slot by slot
        donor_freq         float32 [i_max], with a donor dataset: the donor's
        pcres              the (chrom, start, end) of the gene's live slots
        eps                float32 [P, P, n_out], with epistasis=True: the pair epistasis, the leave-one-out effects on the diagonal
        interactions       float32 [P, P, n_out], with interactions="sii" / "sti": the pairwise Shapley interaction index; the batch then
                           makes one contact.contact_shapley_interactions call in place of contact.contact_shapley
        dividends, mass    float32 [2^P, n_out] each, with dividends=True: as in mark_shapley

    marks="own" (default) plays the game on the gene's own features.  marks="donor" (a donor dataset is required) plays it on the donor's
    features under the gene's masks: `logits` is then mark_donor_shapley's `donor` row and, with players that hold every contact, the
    every-player-absent row is the donor dataset's own forward -- the two games' phi together account for logits - donor_prediction
    of mark_donor_shapley.  The Embedding + Pairwise stage runs once per gene; the rows cost what pcre_shapley's cost.  The binned
    features come from `store` / `donor_store` as in mark_donor_shapley.  Parameters, gradients and optimiser state are left as they
    are; the pass overwrites the activations a grad-enabled model(...) keeps for its backward."""
    from . import contact as games
    ds, dn = dataset, donor_dataset
    who = "contact_shapley"
    if marks not in ("own", "donor"):
        raise ValueError("%s: marks = %r: 'own' (the gene's features) or 'donor' (the donor dataset's, under the gene's masks)" % (who, marks))
    if marks == "donor" and dn is None:
        raise ValueError("%s: marks='donor' needs a donor_dataset" % who)
    binsizes, _, genes, chunk = _open(who, model, ds, genes, bsz, dn)
    spec = players if isinstance(players, str) else list(players)
    names = contact_players(spec, ds.i_max)[2]      # (refusals before anything is loaded)
    if interactions is not None:
        interaction_index(interactions, who)
    S, absent = ds.i_max, "erased" if dn is None else "donor"
    for ids, _, d, args, donor, dd in _batches(who, model, ds, genes, chunk, binsizes, store, dn, donor_store):
        kw = dict(players=spec, scale=scale)
        if dn is not None:
            kw["donor_freq"] = dd["interaction_freq"].contiguous()
            if marks == "donor":
                args = (donor[0], args[1], donor[1]) + tuple(args[3:])
        phi, inter, info, div, mass = _exact_game(model, "contact", args, kw, interactions, dividends, games.bound(model))
        logits, gone = info["logits"].cpu().numpy(), info[absent].cpu().numpy()
        eps = games.contact_epistasis(model, *args, **kw)[0].cpu().numpy() if epistasis else None
        freq = d["interaction_freq"][:, 0, 1:].cpu().numpy()
        dfreq = None if dn is None else dd["interaction_freq"][:, 0, 1:].cpu().numpy()
        for i, g in enumerate(ids):
            out = dict(gene_id=g, phi=phi[i].copy(), logits=logits[i].copy(), players=list(names), freq=freq[i].copy(),
                       pcres=[tuple(p) for p in ds.genes[g]["pcres"][:S]])
            out[absent] = gone[i].copy()
            if dfreq is not None:
                out["donor_freq"] = dfreq[i].copy()
            yield _optional_keys(out, i, eps, inter, div, mass)


def mark_shapley_sampled(model, dataset, donor_dataset=None, genes=None, players="cells", n_perm=64, seed=0, scale=0.0, bsz=None, store=None,
                         donor_store=None):
    """Permutation-sampled Shapley values of up to 128 histone-mark players for the genes of a ChromoformerDataset (one
    model.mark_shapley_sampled per batch): which mark matters at which region?  Without `donor_dataset` an absent player's raw signal
    is scaled by `scale` (0 erases it); with one -- the same genes over the same regions in another cell type (same_regions runs
    first) -- it takes the donor's signal.  A generator over `genes` (ids; default: the dataset's) in chunks of at most
    min(bsz, model.max_batch) genes; per gene it yields a dict of host arrays:

        gene_id        the id
        phi            float32 [P, n_out]: the estimates, in logit space; phi.sum(0) = logits - absent up to rounding
        stderr         float32 [P, n_out]: the standard error of phi over the sampled orders -- the sampling error is reported here
                       and not bounded anywhere
        logits         float32 [n_out]: the prediction (every player present)
        absent         float32 [n_out]: every player absent
        players        the players' names (mark_players_wide); "cells": phi.reshape(i_max + 1, n_feats, n_out)
        permutations   uint8 [n_perm, P]: the orders, shapley_permutations(P, n_perm, seed), the same for every gene

    The binned features come from `store` / `donor_store` as in mark_donor_shapley.  Parameters, gradients and optimiser state are left
    as they are; the pass overwrites the activations a grad-enabled model(...) keeps for its backward."""
    ds, dn = dataset, donor_dataset
    who = "mark_shapley_sampled"
    binsizes, _, genes, chunk = _open(who, model, ds, genes, bsz, dn)
    spec = players if isinstance(players, str) else list(players)
    names = mark_players_wide(spec, ds.n_feats, ds.i_max)[2]      # (refusals before anything is loaded)
    perms = shapley_permutations(len(names), n_perm, seed)
    for ids, _, _, args, donor, _ in _batches(who, model, ds, genes, chunk, binsizes, store, dn, donor_store):
        phi, info = model.mark_shapley_sampled(*args, players=spec, permutations=perms, scale=scale, donor=donor)
        phi, se, logits, absent = phi.cpu().numpy(), info["stderr"].cpu().numpy(), info["logits"].cpu().numpy(), info["absent"].cpu().numpy()
        for i, g in enumerate(ids):
            yield dict(gene_id=g, phi=phi[i].copy(), stderr=se[i].copy(), logits=logits[i].copy(), absent=absent[i].copy(), players=list(names),
                       permutations=perms.copy())


def backselect_row_count(P):
    """The forwards per gene of a back-selection over P players: the two end rows, then P - t candidates in round t = 0 .. P - 2."""
    P = int(P)
    if P < 1:
        raise ValueError("backselect_row_count: P = %d: at least 1 player" % P)
    return P * (P + 1) // 2 + 1


def backselect_words(order, mode="backward"):
    """The coalitions a selection order visits -> uint32 [P + 1, kw], kw = ceil(P / 32), bit p % 32 of word p / 32 = player p present
    (mark_wide_words' layout): row t is the set after t moves -- backward: everybody less order[:t]; forward: order[:t]."""
    order = np.asarray(order)
    P = order.size
    if order.ndim != 1 or P < 1 or sorted(order.tolist()) != list(range(P)):
        raise ValueError("backselect_words: order must be a permutation of 0..P-1")
    if mode not in ("backward", "forward"):
        raise ValueError("backselect_words: mode = %r: 'backward' or 'forward'" % (mode,))
    kw = (P + 31) // 32
    cur = 0 if mode == "forward" else (1 << P) - 1
    words = np.zeros((P + 1, kw), dtype=np.uint32)
    for t in range(P + 1):
        for k in range(kw):
            words[t, k] = (cur >> (32 * k)) & 0xFFFFFFFF
        if t < P:
            cur ^= 1 << int(order[t])
    return words


def subset_bools(words, P):
    """Coalition words [..., kw] (an integer tensor, bit p % 32 of word p / 32 = player p) -> bool [..., P]: a change of layout."""
    import torch
    p = torch.arange(P, device=words.device)
    return ((words.to(torch.int64)[..., p // 32] >> (p % 32)) & 1).bool()


def subset_names(subset, names):
    """The names of the players of a subset: a bool array [P], or a coalition as a Python int / its uint32 words."""
    if isinstance(subset, (int, np.integer)):
        return [n for p, n in enumerate(names) if int(subset) >> p & 1]
    a = np.asarray(subset.cpu() if hasattr(subset, "cpu") else subset)
    if a.dtype != np.bool_:
        a = np.array([int(a.reshape(-1)[p // 32]) >> (p % 32) & 1 for p in range(len(names))], dtype=bool)
    if a.shape != (len(names),):
        raise ValueError("subset_names: the subset has shape %s for %d players" % (a.shape, len(names)))
    return [n for n, keep in zip(names, a) if keep]


def mark_shapley_interactions_sampled(model, dataset, donor_dataset=None, genes=None, players="cells", top=4, focal=None, index="sii", n_perm=64,
                                      seed=0, scale=0.0, bsz=None, store=None, donor_store=None):
    """Sampled pairwise Shapley interaction indices of each gene's leading histone-mark players, for the genes of a
    ChromoformerDataset: for the cells that carry the prediction, which other cells are redundant with them, which cooperate?  Per
    batch one model.mark_shapley_sampled call finds every gene's `top` players by |phi| at the last output column (ties: the lower
    index); per gene one model.mark_shapley_interactions_sampled call on that gene alone, with the same orders, takes them as its focal
    players (the rows run in chunks of max_batch either way).  `focal` (indices or names, attribution.focal_players) fixes the focal
    players for every gene instead, and the per-batch call is skipped.  With `donor_dataset` an absent player takes the donor's signal
    (same_regions runs first), else its raw signal is scaled by `scale`.  A generator over `genes` (ids; default: the dataset's); per
    gene it yields a dict of host arrays:

        gene_id        the id
        interactions   float32 [n_focal, P, n_out]: row f estimates the index of focal player focal[f] with every player; the
                       diagonal entry as in model.mark_shapley_interactions_sampled.  Not symmetric between two focal players
        stderr         float32 [n_focal, P, n_out]: the standard error over the orders -- the sampling error is reported here and
                       not bounded anywhere
        phi, phi_stderr   float32 [P, n_out]: the sampled Shapley values from the same forwards
        focal          int32 [n_focal]: the focal players, strongest first;  focal_names: their names
        logits, absent    float32 [n_out]: every player present (the prediction), every player absent
        players        the players' names (mark_players_wide)
        index          the index name
        permutations   uint8 [n_perm, P]: the orders, shapley_permutations(P, n_perm, seed), the same for every gene

    The binned features come from `store` / `donor_store` as in mark_donor_shapley.  Parameters, gradients and optimiser state are left
    as they are; the pass overwrites the activations a grad-enabled model(...) keeps for its backward."""
    ds, dn = dataset, donor_dataset
    who = "mark_shapley_interactions_sampled"
    binsizes, _, genes, chunk = _open(who, model, ds, genes, bsz, dn)
    spec = players if isinstance(players, str) else list(players)
    names = mark_players_wide(spec, ds.n_feats, ds.i_max)[2]      # (refusals before anything is loaded)
    P = len(names)
    interaction_index(index, who)
    if P < 2:
        raise ValueError("%s: %d player; a pair needs at least 2" % (who, P))
    if focal is not None:
        focal = focal_players(focal, names, P)
    elif not 1 <= int(top) <= P:
        raise ValueError("%s: top = %r outside 1..%d" % (who, top, P))
    perms = shapley_permutations(P, n_perm, seed)
    store = _resident_store(who, ds, genes, binsizes, model._device, store)      # (here: both iterators below read the same stores)
    if dn is not None:
        donor_store = _resident_store(who, dn, genes, binsizes, model._device, donor_store)

    def focal_of():      # per gene its focal players: `focal`, else the leaders among its chunk's sampled Shapley values
        if focal is not None:
            yield from (focal for _ in genes)
            return
        for _, _, _, args, donor, _ in _batches(who, model, ds, genes, chunk, binsizes, store, dn, donor_store):
            phi = model.mark_shapley_sampled(*args, players=spec, permutations=perms, scale=scale, donor=donor)[0]
            yield from np.argsort(-np.abs(phi[..., -1].cpu().numpy()), axis=1, kind="stable")[:, :int(top)].astype(np.int32)

    # a chunk's batch is loaded when its first gene asks for its focal players, then each gene's own batch
    for mine, ((g,), _, _, args, donor, _) in zip(focal_of(), _batches(who, model, ds, genes, 1, binsizes, store, dn, donor_store)):
        inter, info = model.mark_shapley_interactions_sampled(*args, players=spec, focal=mine, index=index, permutations=perms, scale=scale,
                                                              donor=donor)
        host = lambda t: t[0].cpu().numpy().copy()      # noqa: E731
        yield dict(gene_id=g, interactions=host(inter), stderr=host(info["stderr"]), phi=host(info["phi"]), phi_stderr=host(info["phi_stderr"]),
                   focal=np.array(mine, dtype=np.int32), focal_names=[names[int(p)] for p in mine], logits=host(info["logits"]),
                   absent=host(info["absent"]), players=list(names), index=index, permutations=perms.copy())


def window_player_coordinates(marks_regions_windows, regions, n_real, binsize):
    """Genomic coordinates of window players for one gene.  marks_regions_windows: window_players' (marks, regions, lo, hi, ...);
    regions: {region index: (chrom, start, end)} of the regions the gene has; n_real: {region index: real bins at the coarsest
    resolution}; binsize: the coarsest bin size -> (windows, null): per player the list of (region index, chrom, start, end) of its REAL
    windows -- start + lo * binsize, the end clipped to the region, the windows of the perturbation scan -- and a bool [P], True where
    the player has none (a null player for this gene: its phi is exactly 0)."""
    _, pr, lo, hi = marks_regions_windows[:4]
    windows = []
    for p in range(len(pr)):
        real = []
        for rho, (chrom, start, end) in sorted(regions.items()):
            if (int(pr[p]) >> rho) & 1 and int(lo[p]) < n_real[rho]:
                real.append((rho, chrom, int(start) + int(lo[p]) * int(binsize), min(int(start) + int(hi[p]) * int(binsize), int(end))))
        windows.append(real)
    return windows, np.array([not w for w in windows], dtype=bool)


def mark_window_shapley(model, dataset, donor_dataset=None, genes=None, players="promoter", width=1, n_perm=64, seed=0, scale=0.0, bsz=None,
                        store=None, donor_store=None, interactions=None, dividends=False):
    """Shapley values of WINDOW players for the genes of a ChromoformerDataset: where inside a region does the signal lie?  With at most
    16 players one model.mark_window_shapley per batch (exact), else one model.mark_window_shapley_sampled (n_perm orders from `seed`).
    Without `donor_dataset` an absent player's raw signal inside its window is scaled by `scale` (0 erases it); with one -- the same
    genes over the same regions in another cell type (same_regions runs first) -- it takes the donor's signal.  A generator over
    `genes` (ids; default: the dataset's) in chunks of at most min(bsz, model.max_batch) genes; per gene it yields a dict of host arrays:

        gene_id        the id
        estimator      "exact" or "sampled"
        phi            float32 [P, n_out]: the values, in logit space; phi.sum(0) = logits - absent up to rounding
        stderr         float32 [P, n_out]: the standard error of phi over the sampled orders; zeros from the exact call
        logits         float32 [n_out]: the prediction (every player present)
        absent         float32 [n_out]: every player absent
        players        the players' names (window_players)
        windows        per player the list of (region index, chrom, start, end) of its real windows in this gene, genomic coordinates as
                       perturbation_scan reports them ('-' strand promoters are stored mirrored: window 0 is still the genomic start)
        null           bool [P]: the player has no real window in this gene (a dummy slot, a short pCRE, a narrowed promoter): phi = 0
        permutations   uint8 [n_perm, P], sampled only: the orders, the same for every gene
        interactions   float32 [P, P, n_out], with interactions="sii" / "sti": the pairwise Shapley interaction index of the players (a
                       null player's row and column are 0); the batch then makes one model.mark_window_shapley_interactions call in
                       place of model.mark_window_shapley.  The index has no sampled estimator: more than 16 players raise ValueError
        dividends, mass  float32 [2^P, n_out] each, with dividends=True: as in mark_shapley (a set that holds a null player is 0); the
                       exact game only: more than 16 players raise ValueError

    Strand and coordinates come from the dataset's metadata.  The binned features come from `store` / `donor_store` as in
    mark_donor_shapley.  Parameters, gradients and optimiser state are left as they are; the pass overwrites the activations a
    grad-enabled model(...) keeps for its backward."""
    from .data import promoter_col0
    ds, dn = dataset, donor_dataset
    who = "mark_window_shapley"
    binsizes, n_bins, genes, chunk = _open(who, model, ds, genes, bsz, dn)
    spec = players if isinstance(players, str) else list(players)
    rc = int(np.argmin(n_bins))
    W, bc = n_bins[rc], binsizes[rc]
    game = window_players(spec, ds.n_feats, ds.i_max, W, width)      # (refusals before anything is loaded)
    names = game[4]
    P = len(names)
    exact = P <= 16
    if interactions is not None:
        interaction_index(interactions, who)
        if not exact:
            raise ValueError("%s: interactions: %d players; the index is computed by the exact game of at most 16 players: choose a "
                             "larger width" % (who, P))
    if dividends and not exact:
        raise ValueError("%s: dividends: %d players; the dividends are those of the exact game of at most 16 players: choose a larger width"
                         % (who, P))
    perms = None if exact else shapley_permutations(P, n_perm, seed)
    col0 = promoter_col0(ds)
    for ids, _, d, args, donor, _ in _batches(who, model, ds, genes, chunk, binsizes, store, dn, donor_store):
        B = len(ids)
        kw = dict(players=spec, width=width, scale=scale, donor=donor, flip=[ds.genes[g]["tss"][2] != "+" for g in ids])
        inter, div, mass = None, None, None
        if exact:
            phi, inter, info, div, mass = _exact_game(model, "mark_window", args, kw, interactions, dividends)
            absent = info["erased" if donor is None else "donor"].cpu().numpy()
            se = np.zeros(phi.shape, dtype=np.float32)
        else:
            phi, info = model.mark_window_shapley_sampled(*args, permutations=perms, **kw)
            phi, absent, se = phi.cpu().numpy(), info["absent"].cpu().numpy(), info["stderr"].cpu().numpy()
        logits = info["logits"].cpu().numpy()
        pm = d["promoter_pad_masks"][bc].reshape(B, -1, W)
        pm = pm[:, pm.shape[1] // 2].cpu().numpy() == 0                       # the centre row of a full [L, L] mask, or the compact row
        cm = d["pcre_pad_masks"][bc].reshape(B, ds.i_max, -1, W)
        cm = cm[:, :, cm.shape[2] // 2].cpu().numpy() == 0
        for i, g in enumerate(ids):
            regions = {0: _gene_region(ds, g, 0, col0)}
            regions.update({1 + j: tuple(p) for j, p in enumerate(ds.genes[g]["pcres"][:ds.i_max])})
            n_real = {}
            for rho in regions:
                real = np.flatnonzero(pm[i] if rho == 0 else cm[i, rho - 1])
                n_real[rho] = int(real[-1] - real[0] + 1) if real.size else 0
            windows, null = window_player_coordinates(game, regions, n_real, bc)
            out = dict(gene_id=g, estimator="exact" if exact else "sampled", phi=phi[i].copy(), stderr=se[i].copy(), logits=logits[i].copy(),
                       absent=absent[i].copy(), players=list(names), windows=windows, null=null)
            if not exact:
                out["permutations"] = perms.copy()
            yield _optional_keys(out, i, None, inter, div, mass)


def mark_fine_window_shapley(model, dataset, donor_dataset=None, genes=None, region="promoter", zoom=1, coarse_width=1, width=2, players="windows",
                             n_perm=64, seed=0, scale=0.0, target=None, bsz=None, store=None, donor_store=None, interactions=None,
                             dividends=False):
    """Shapley values of FINE window players for the genes of a ChromoformerDataset: which 200 bp of this peak?  Per batch the coarse
    window game runs first (model.mark_window_shapley over `region` at `coarse_width` coarsest bins per player, exact with at most 16
    players, else sampled); per gene the `zoom` coarse windows with the largest |phi| at logit `target` (default: the last) are chosen,
    and inside each the fine game is played: players = fine_window_players(players, n_feats, width, ...) tiling the coarse window, each
    gene at its own start (model.mark_fine_window_shapley, or _sampled above 16 players with n_perm orders from `seed`).  Without
    `donor_dataset` an absent player's raw signal inside its window is scaled by `scale` (0 erases it); with one -- the same genes over
    the same regions in another cell type (same_regions runs first) -- it takes the donor's signal, in both games.  A generator over
    `genes` in chunks of at most min(bsz, model.max_batch) genes; per gene it yields a dict:

        gene_id         the id
        region          (chrom, start, end) of the region, None if the gene does not have it (everything below is then empty)
        coarse_phi      float32 [n_cwin, n_out]: the coarse game's values of the region's real coarse windows
        coarse_windows  [(chrom, start, end)]: those windows
        zoom            int64 [k']: the chosen coarse windows, most important first (k' = min(zoom, n_cwin))
        players         the names of the fine players with a real window, rank 0's first, then rank 1's, ...
        windows         [(chrom, start, end)]: each such player's window in genomic coordinates, the end clipped to the region
        rank, index     int64 [n] each: the rank of the coarse window the player lies in and its index among the fine game's players
        phi             float32 [n, n_out]: their values, in logit space; per rank they sum to logits - absent[rank] up to rounding
        stderr          float32 [n, n_out], or None when the fine game was exact
        logits          float32 [n_out]: the prediction
        absent          float32 [k', n_out]: per rank, every fine player absent
        exact           whether the fine game was exact
        interactions    with interactions="sii" / "sti": per rank a float32 [n_r, n_r, n_out], the pairwise Shapley interaction index of
                        that rank's fine players with a real window, in their order above; the fine game then makes one
                        model.mark_fine_window_shapley_interactions call in place of model.mark_fine_window_shapley (the coarse game is
                        unchanged).  The index has no sampled estimator: more than 16 fine players raise ValueError
        dividends, mass with dividends=True: per rank a float32 [2^P, n_out] over ALL P players of the fine game (bit p = the player of
                        `index` p; a set that holds a player without a real window is 0), and the scale of the rounding error
                        (dividend_bound); the exact fine game only: more than 16 fine players raise ValueError

    Strand, coordinates and the region's length come from the dataset's metadata: '-' strand promoters are stored mirrored (window 0 is
    still the genomic start) and the short last bin of a pCRE is weighted by the samples it holds.  Features, stores, parameters and
    the effect on a pending backward: as mark_window_shapley."""
    from .data import promoter_col0
    ds, dn = dataset, donor_dataset
    who = "mark_fine_window_shapley"
    binsizes, n_bins, genes, chunk = _open(who, model, ds, genes, bsz, dn)
    S, F = ds.i_max, ds.n_feats
    region = _region_index(who, region, S)
    zoom, coarse_width, width = int(zoom), int(coarse_width), int(width)
    if zoom < 1:
        raise ValueError("%s: zoom = %d: at least 1 coarse window" % (who, zoom))
    if coarse_width < 1 or width < 1:
        raise ValueError("%s: coarse_width = %d, width = %d: at least 1 bin each" % (who, coarse_width, width))
    rf, rc = int(np.argmin(binsizes)), int(np.argmin(n_bins))
    Lf, bf, W, bc = n_bins[rf], binsizes[rf], n_bins[rc], binsizes[rc]
    Rc = Lf // W
    spec = players if isinstance(players, str) else list(players)
    n_fw = -(-(coarse_width * Rc) // width)
    game = fine_window_players(spec, F, width, n_fw)      # (refusals before anything is loaded)
    names = game[3]
    P = len(names)
    exact = P <= 16
    if interactions is not None:
        interaction_index(interactions, who)
        if not exact:
            raise ValueError("%s: interactions: %d fine players; the index is computed by the exact game of at most 16 players: choose a "
                             "larger width or a smaller coarse_width" % (who, P))
    if dividends and not exact:
        raise ValueError("%s: dividends: %d fine players; the dividends are those of the exact game of at most 16 players: choose a larger "
                         "width or a smaller coarse_width" % (who, P))
    perms = None if exact else shapley_permutations(P, n_perm, seed)
    coarse = [(list(range(F)), [region], (g, min(g + coarse_width, W))) for g in range(0, W, coarse_width)]
    Pc = len(coarse)
    cperms = None if Pc <= 16 else shapley_permutations(Pc, n_perm, seed)
    target = model.n_out - 1 if target is None else int(target)
    col0 = promoter_col0(ds)
    for ids, _, _, args, donor, _ in _batches(who, model, ds, genes, chunk, binsizes, store, dn, donor_store):
        flip = [region == 0 and ds.genes[g]["tss"][2] != "+" for g in ids]
        regs = [_gene_region(ds, g, region, col0) for g in ids]
        lengths = [r[2] - r[1] if r else 0 for r in regs]
        if cperms is None:
            cphi, info = model.mark_window_shapley(*args, players=coarse, scale=scale, donor=donor, flip=flip)
        else:
            cphi, info = model.mark_window_shapley_sampled(*args, players=coarse, permutations=cperms, scale=scale, donor=donor, flip=flip)
        cphi, logits = cphi.cpu().numpy(), info["logits"].cpu().numpy()
        per, ranks = [], []
        for i, r in enumerate(regs):
            n_cw = min(-(-(-(-(r[2] - r[1]) // bc)) // coarse_width), Pc) if r else 0
            z = np.argsort(-np.abs(cphi[i, :n_cw, target]), kind="stable")[:zoom].astype(np.int64)
            ranks.append(z)
            cwins = [(r[0], r[1] + g * coarse_width * bc, min(r[1] + (g + 1) * coarse_width * bc, r[2])) for g in range(n_cw)] if r else []
            per.append(dict(gene_id=ids[i], region=r, coarse_phi=cphi[i, :n_cw].copy(), coarse_windows=cwins, zoom=z, players=[], windows=[], rank=np.zeros(0, np.int64),
                            index=np.zeros(0, np.int64),
                            phi=np.zeros((0, model.n_out), np.float32), stderr=None if exact else np.zeros((0, model.n_out), np.float32),
                            logits=logits[i].copy(), absent=np.zeros((0, model.n_out), np.float32), exact=exact))
            if interactions is not None:
                per[-1]["interactions"] = []
            if dividends:
                per[-1]["dividends"], per[-1]["mass"] = [], []
        for rank in range(max([len(z) for z in ranks] + [0])):
            # a gene with fewer real coarse windows than ranks starts past its region: null players, left out below
            start = [int(z[rank]) * coarse_width * Rc if rank < len(z) else Lf for z in ranks]
            kw = dict(region=region, players=spec, width=width, n_windows=n_fw, start=start, lengths=lengths, scale=scale, donor=donor, flip=flip)
            inter, div = None, None
            if exact:
                phi, inter, info, div, mass = _exact_game(model, "mark_fine_window", args, kw, interactions, dividends)
                absent, se = info["erased" if donor is None else "donor"].cpu().numpy(), None
            else:
                phi, info = model.mark_fine_window_shapley_sampled(*args, permutations=perms, **kw)
                phi, absent, se = phi.cpu().numpy(), info["absent"].cpu().numpy(), info["stderr"].cpu().numpy()
            for i, r in enumerate(regs):
                if rank >= len(ranks[i]):
                    continue
                first = r[1] + start[i] * bf
                real = [p for p in range(P) if first + int(game[1][p]) * bf < r[2]]
                per[i]["players"] += [names[p] for p in real]
                per[i]["windows"] += [(r[0], first + int(game[1][p]) * bf, min(first + int(game[2][p]) * bf, r[2])) for p in real]
                per[i]["rank"] = np.concatenate([per[i]["rank"], np.full(len(real), rank, np.int64)])
                per[i]["index"] = np.concatenate([per[i]["index"], np.array(real, np.int64)])
                per[i]["phi"] = np.concatenate([per[i]["phi"], phi[i, real]])
                if not exact:
                    per[i]["stderr"] = np.concatenate([per[i]["stderr"], se[i, real]])
                per[i]["absent"] = np.concatenate([per[i]["absent"], absent[i][None]])
                if inter is not None:
                    per[i]["interactions"].append(inter[i][np.ix_(real, real)].copy())
                if div is not None:
                    per[i]["dividends"].append(div[i].copy())
                    per[i]["mass"].append(mass[i].copy())
        for p in per:
            yield p
