"""numpy restatement of the hypervolume subset selection inside the Pareto
front: participation, the greedy rounds with the exact (two
objectives) and the Monte-Carlo key, and the surrogate loss that follows.
Test infrastructure only.  Every product, difference and sum is formed as the
rule writes it, in float64, so a device result can be compared bit for bit.

Also the ground truth the estimators are checked against: the 2-d sweep
hypervolume and inclusion-exclusion over a small set of boxes.
"""
import itertools

import numpy as np

import pareto_oracle as PO
from draw_replay import uniforms

STREAM = 0x60000000
AUTO, EXACT, MC = 0, 1, 2


def uniform_table(seed, S, M):
    """u[S, M]: u[s, m] is component m % 4 of uniforms(seed, gi=s, STREAM, it=m // 4)."""
    u = np.empty((S, M))
    gi = np.arange(S, dtype=np.uint64)
    for it in range((M + 3) // 4):
        us = uniforms(seed, gi, STREAM, it)
        for c in range(4):
            if 4 * it + c < M:
                u[:, 4 * it + c] = us[c]
    return u


def participants(Y, by, r):
    """(part bool[n], w[M, n]): complete, nondominated, finite, strictly below r."""
    Y = np.asarray(Y, dtype=np.float64)
    r = np.asarray(r, dtype=np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        w = r[:, None] - Y
        part = PO.complete_rows(Y) & (np.asarray(by) == 0) & np.isfinite(Y).all(axis=0) \
            & (w > 0).all(axis=0)
    return part, w


def volumes(w):
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        v = w[0].copy()
        for m in range(1, w.shape[0]):
            v = v * w[m]
    return v


def is_exact(M, method):
    if method not in (AUTO, EXACT, MC):
        raise ValueError('method')
    if method == EXACT and M != 2:
        raise ValueError('the exact method needs two objectives')
    return method == EXACT or (method == AUTO and M == 2)


def hv_select(Y, by, r, n_pick=32, n_samples=1024, seed=0, method=AUTO, trace=None):
    """(picks int32[n_pick], keys float64[n_pick], counts int32[n_pick], R):
    rows in pick order (-1 from round R on), the key of each pick as the
    device holds it (the Monte-Carlo key is vol * alive, not divided by S; 0
    from round R on) and its alive samples (-1 on the exact path and from
    round R on).  ``trace``: a list that receives every round's key[n] (the
    round that ends the selection included)."""
    Y = np.asarray(Y, dtype=np.float64)
    M, n = Y.shape
    assert M >= 2 and 1 <= n_pick <= 256
    assert n_samples % 64 == 0 and 64 <= n_samples <= 4096
    r = np.asarray(r, dtype=np.float64)
    assert r.shape == (M,) and np.isfinite(r).all()
    exact = is_exact(M, method)
    part, w = participants(Y, by, r)
    vol = volumes(w)
    picks = np.full(n_pick, -1, dtype=np.int32)
    keys = np.zeros(n_pick)
    counts = np.full(n_pick, -1, dtype=np.int32)
    live = part.copy()                      # takes part, not picked, not dead
    rows = np.flatnonzero(part)
    if exact:
        gain = np.where(part, vol, 0.0)
        right = np.full(n, r[0])
        top = np.full(n, r[1])
    else:
        u = uniform_table(seed, n_samples, M)
        # z[i][s, m] = y + u * w: a rounded product, then a rounded sum
        z = {i: Y[:, i][None, :] + u * w[:, i][None, :] for i in rows}
        alive = {i: np.ones(n_samples, dtype=bool) for i in rows}
        cnt = np.where(part, n_samples, 0).astype(np.int64)
    R = n_pick
    for t in range(n_pick):
        if t > 0:
            p = picks[t - 1]
            yp = Y[:, p]
            for i in rows:
                if not live[i]:
                    continue
                if exact:
                    if yp[0] == Y[0, i] and yp[1] == Y[1, i]:
                        live[i] = False
                        gain[i] = 0.0
                        continue
                    if yp[0] > Y[0, i] and yp[0] < right[i]:
                        right[i] = yp[0]
                    if yp[1] > Y[1, i] and yp[1] < top[i]:
                        top[i] = yp[1]
                    with np.errstate(over='ignore'):
                        gain[i] = (right[i] - Y[0, i]) * (top[i] - Y[1, i])
                else:
                    alive[i] &= ~(yp[None, :] <= z[i]).all(axis=1)
                    cnt[i] = alive[i].sum()
        key = np.zeros(n)
        for i in rows:
            if not live[i]:
                continue
            if exact:
                key[i] = gain[i]
            elif cnt[i] > 0:
                with np.errstate(over='ignore'):
                    key[i] = vol[i] * float(cnt[i])
        assert (key >= 0).all()
        if trace is not None:
            trace.append(key.copy())
        best = int(np.argmax(key)) if n else 0          # (the first of the largest: the lower row)
        if not key[best] > 0:
            R = t
            break
        picks[t] = best
        keys[t] = key[best]
        counts[t] = -1 if exact else cnt[best]
        live[best] = False
    return picks, keys, counts, R


def hv_surrogate(by, of, ok, picks, R):
    """s = dominated_by (n + 1) + sec; sec = t for pick t, max(R, n - dominates)
    for the other rows of the front, n - dominates elsewhere; +inf pending."""
    n = len(by)
    assert (n + 1) ** 2 < 2 ** 53
    by64, of64 = by.astype(np.int64), of.astype(np.int64)
    sec = n - of64
    front = by64 == 0
    sec[front] = np.maximum(sec[front], R)
    for t in range(R):
        sec[picks[t]] = t
    assert (sec >= 0).all() and (sec <= n).all()
    s = (by64 * (n + 1) + sec).astype(np.float64)
    s[~np.asarray(ok)] = np.inf
    return s


def hv_rank(Y, r, n_pick=32, n_samples=1024, seed=0, method=AUTO, fast=True):
    """(dominated_by, dominates, s, picks, keys, counts, R) of ``Y[M, n]``."""
    Y = np.asarray(Y, dtype=np.float64)
    by, of = (PO.pareto_counts_fast if fast else PO.pareto_counts)(Y)
    ok = PO.complete_rows(Y)
    if Y.shape[0] == 1:                                 # a total order: the setting is ignored
        return by, of, PO.surrogate(by, of, ok), np.full(n_pick, -1, np.int32), \
            np.zeros(n_pick), np.full(n_pick, -1, np.int32), 0
    picks, keys, counts, R = hv_select(Y, by, r, n_pick, n_samples, seed, method)
    return by, of, hv_surrogate(by, of, ok, picks, R), picks, keys, counts, R


def default_reference(Y):
    """Per objective over the finite values of complete rows: hi + 0.1 (hi - lo),
    hi + 1 when hi == lo; None without a complete row."""
    Y = np.asarray(Y, dtype=np.float64)
    ok = PO.complete_rows(Y)
    if not ok.any():
        return None
    r = []
    for m in range(Y.shape[0]):
        v = Y[m, ok]
        v = v[np.isfinite(v)]
        if len(v) == 0:
            r.append(1.0)
            continue
        hi, lo = float(v.max()), float(v.min())
        r.append(hi + 1.0 if hi == lo else hi + 0.1 * (hi - lo))
    return tuple(r)


# ------------------------------------------------------------------ ground truth
def hv2d(points, r):
    """The area dominated by 2-d points inside the box below r, by a sweep."""
    pts = sorted((float(a), float(b)) for a, b in points if a < r[0] and b < r[1])
    area, top = 0.0, float(r[1])
    for a, b in pts:                                    # ascending y0: a staircase of new lows
        if b < top:
            area += (r[0] - a) * (top - b)
            top = b
    return area


def hv_inclusion_exclusion(points, r):
    """The volume of the union of the boxes [p, r], any dimension (small sets)."""
    pts = [np.asarray(p, dtype=np.float64) for p in points]
    r = np.asarray(r, dtype=np.float64)
    total = 0.0
    for k in range(1, len(pts) + 1):
        for sub in itertools.combinations(pts, k):
            side = r - np.max(sub, axis=0)
            total += (-1) ** (k + 1) * float(np.prod(np.maximum(side, 0.0)))
    return total
