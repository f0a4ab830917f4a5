"""The greedy player selection of cf_backselect.h (model.mark_backselect, model.backselect) restated in plain numpy: the pick rule with
its tie and NaN handling, the path, and the threshold arithmetic in float32 in the kernel's operation order.  One gene at a time."""
import numpy as np

F = np.float32


def direction_of(nobody, everybody, target=0, direction=0):
    """s: +1 if everybody[target] >= nobody[target] else -1 (a NaN compares false: -1); a non-zero `direction` overrides it."""
    return int(direction) if direction else (1 if F(everybody[target]) >= F(nobody[target]) else -1)


def pick(vals, s):
    """The candidate with the largest key s * v (float32), scanned in ascending index with strict >; a NaN key counts as -inf."""
    with np.errstate(invalid="ignore"):
        key = (F(s) * np.asarray(vals, dtype=F)).astype(F)
    key = np.where(np.isnan(key), F(-np.inf), key)
    best = 0
    for c in range(1, len(key)):
        if key[c] > key[best]:
            best = c
    return best


def candidates(cur, P, mode):
    """The players one move away from the set `cur` (a Python int), ascending: its members (backward) or its non-members (forward)."""
    return [p for p in range(P) if (cur >> p & 1) == (0 if mode == "forward" else 1)]


def greedy(value, P, mode="backward", direction=0, target=0):
    """The path on a set function value(word) -> [n_out] -> (order [P], values [P + 1, n_out] float32, s, rows): rows[0] is [nobody,
    everybody], rows[1 + t] the P - t candidates' values of round t = 0 .. P - 2."""
    full = (1 << P) - 1
    nobody, everybody = np.asarray(value(0), dtype=F), np.asarray(value(full), dtype=F)
    s = direction_of(nobody, everybody, target, direction)
    cur = 0 if mode == "forward" else full
    order, values, rows = [], [np.asarray(value(cur), dtype=F)], [np.stack([nobody, everybody])]
    for t in range(P - 1):
        cand = candidates(cur, P, mode)
        vals = np.stack([np.asarray(value(cur ^ (1 << p)), dtype=F) for p in cand])
        rows.append(vals)
        c = pick(vals[:, target], s)
        order.append(cand[c])
        cur ^= 1 << cand[c]
        values.append(vals[c])
    order.append(candidates(cur, P, mode)[0])
    values.append(everybody if mode == "forward" else nobody)
    return np.array(order, dtype=np.int32), np.stack(values), s, rows


def replay(rows, P, mode="backward", direction=0, target=0):
    """Every pick re-derived from one gene's evaluated rows (rows[0] [2, n_out], rows[1 + t] [P - t, n_out]) under the tie and NaN rule
    -> (order, values, s).  No model is asked: the rows are the device's own."""
    nobody, everybody = rows[0][0], rows[0][1]
    s = direction_of(nobody, everybody, target, direction)
    cur = 0 if mode == "forward" else (1 << P) - 1
    order, values = [], [everybody if mode == "backward" else nobody]
    for t in range(P - 1):
        cand = candidates(cur, P, mode)
        vals = np.asarray(rows[1 + t])
        assert len(vals) == len(cand), (t, len(vals), len(cand))
        c = pick(vals[:, target], s)
        order.append(cand[c])
        cur ^= 1 << cand[c]
        values.append(vals[c])
    order.append(candidates(cur, P, mode)[0])
    values.append(nobody if mode == "backward" else everybody)
    return np.array(order, dtype=np.int32), np.stack(values).astype(F), s


def visited(order, P, mode="backward"):
    """Per round t = 0 .. P - 2 the candidate words (Python ints, ascending player) of a path with this order."""
    cur = 0 if mode == "forward" else (1 << P) - 1
    out = []
    for t in range(P - 1):
        out.append([cur ^ (1 << p) for p in candidates(cur, P, mode)])
        cur ^= 1 << int(order[t])
    return out


def finish(values, order, s, mode="backward", frac=0.9, threshold=None, target=0):
    """-> (thr float32, size, subset bool [P]).  thr = nobody + frac * (everybody - nobody) in float32, one rounding per operation, or the
    given threshold; a set is sufficient when s * (v - thr) >= 0 in float32 (a NaN is not); size is the smallest k whose k-player set on
    the path is sufficient, counted from the small end; the set of everybody is sufficient by definition."""
    values = np.asarray(values, dtype=F)
    P = len(order)
    nobody, everybody = (values[0], values[P]) if mode == "forward" else (values[P], values[0])
    with np.errstate(invalid="ignore", over="ignore"):
        thr = F(threshold) if threshold is not None else F(nobody[target] + F(F(frac) * F(everybody[target] - nobody[target])))
        size = P
        for k in range(P):
            v = values[k if mode == "forward" else P - k][target]
            if F(F(s) * F(v - thr)) >= 0:
                size = k
                break
    subset = np.zeros(P, dtype=bool)
    members = order[:size] if mode == "forward" else order[P - size:]
    subset[np.asarray(members, dtype=np.int64)] = True
    return thr, size, subset
