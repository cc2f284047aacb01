"""numpy restatement of the exact three-objective key of the hypervolume
subset selection (method code 3 of tpe_plan_set_hv).  Test
infrastructure only.  Participation, w, vol, the pick rule, R and the
surrogate column are those of ``hv_oracle``; only the key of a live row in
round t >= 1 is new.  Round 0 keeps ``vol_i`` as the key, as the device does
(k_hv_init_exact3 writes it); it has the bits of the one-slab form
``(r[2] - y[2]) * ((r[0] - y[0]) * (r[1] - y[1]))``, a product being commutative.

The key of row i given the picks p_0 .. p_{t-1}, every operation in float64 as
written (no fused multiply-add), max and min as comparisons (``a > b ? a : b``,
``d < h ? d : h``), so signed zeros take one road:

  X order: the picks ascending in objective 0, ties by pick round;
  Z order: ascending in objective 2, ties by pick round; zrank(p) its place.
  c_p[m] = max(y_p[m], y_i[m]) clips pick p into row i's box.
  Slab j = 0 .. t spans [lo_j, hi_j] along objective 2: lo_0 = y_i[2],
  lo_j = hi_{j-1}, hi_j = c[2] of the j-th pick in Z, hi_t = r[2]; h_j = hi_j - lo_j.
  In slab j walk the picks with zrank < j in X order from cur_x = y_i[0],
  cur_h = r[1] - y_i[1], A = +0.0:
      A = A + (c_a[0] - cur_x) * cur_h;  cur_x = c_a[0];
      cur_h = min(cur_h, c_a[1] - y_i[1])
  and close with A = A + (r[0] - cur_x) * cur_h.
  key = +0.0, then for j ascending and only where h_j > 0: key = key + h_j * A_j.

A difference that overflows (|r - y| beyond the largest double) is outside the
rule: 0 * inf would be NaN.  Products may overflow to +inf, as vol may.
"""
import numpy as np

import hv_oracle as HO
import pareto_oracle as PO

EXACT3 = 3


def orders(P):
    """(xrank[t], zrank[t]) of the picks' objectives P[3, t]: the number of
    picks that come before each one in X and in Z."""
    t = P.shape[1]
    q = np.arange(t)
    first = q[None, :] < q[:, None]                     # [k, q]: q was picked before k

    def rank(v):
        return ((v[None, :] < v[:, None]) | ((v[None, :] == v[:, None]) & first)).sum(axis=1)
    return rank(P[0]), rank(P[2])


def exact3_keys(Y, rows, r, picks):
    """key[len(rows)] of ``rows`` given the rows picked so far (in pick order).
    Arrays are [slab, row]: the walk's step for pick a touches the slabs above
    zrank(a), a contiguous block."""
    Y = np.asarray(Y, dtype=np.float64)
    t, R = len(picks), len(rows)
    P = Y[:, picks]
    xrank, zrank = orders(P)
    y0, y1, y2 = Y[0, rows], Y[1, rows], Y[2, rows]
    with np.errstate(over='ignore', invalid='ignore'):
        pz = np.empty(t)
        pz[zrank] = P[2]
        cz = np.where(pz[:, None] > y2[None, :], pz[:, None], y2[None, :])
        hi = np.vstack([cz, np.full((1, R), r[2])])
        lo = np.vstack([y2[None, :], cz])
        h = hi - lo
        cur_x = np.tile(y0, (t + 1, 1))
        cur_h = np.tile(r[1] - y1, (t + 1, 1))
        A = np.zeros((t + 1, R))
        for a in np.argsort(xrank):                     # the picks in X order
            s = slice(int(zrank[a]) + 1, None)          # the slabs pick a reaches
            c0 = np.where(P[0, a] > y0, P[0, a], y0)
            c1 = np.where(P[1, a] > y1, P[1, a], y1)
            A[s] = A[s] + (c0 - cur_x[s]) * cur_h[s]
            cur_x[s] = c0
            d = c1 - y1
            cur_h[s] = np.where(d < cur_h[s], d, cur_h[s])
        A = A + (r[0] - cur_x) * cur_h
        key = np.zeros(R)
        for j in range(t + 1):
            m = h[j] > 0
            key[m] = key[m] + h[j, m] * A[j, m]
    return key


def hv3_select(Y, by, r, n_pick=32, trace=None):
    """``hv_oracle.hv_select`` with the exact three-objective key:
    (picks, keys, counts, R), counts all -1."""
    Y = np.asarray(Y, dtype=np.float64)
    r = np.asarray(r, dtype=np.float64)
    assert Y.shape[0] == 3 and r.shape == (3,) and np.isfinite(r).all()
    assert 1 <= n_pick <= 256
    n = Y.shape[1]
    part, w = HO.participants(Y, by, r)
    vol = HO.volumes(w)
    picks = np.full(n_pick, -1, dtype=np.int32)
    keys = np.zeros(n_pick)
    counts = np.full(n_pick, -1, dtype=np.int32)
    live = part.copy()
    R = n_pick
    for t in range(n_pick):
        key = np.zeros(n)
        rows = np.flatnonzero(live)
        if t == 0:
            key[rows] = vol[rows]
        elif len(rows):
            key[rows] = exact3_keys(Y, rows, r, picks[:t])
        assert (key >= 0).all()
        if trace is not None:
            trace.append(key.copy())
        best = int(np.argmax(key)) if n else 0          # (the first of the largest: the lower row)
        if not key[best] > 0:
            R = t
            break
        picks[t] = best
        keys[t] = key[best]
        live[best] = False
    return picks, keys, counts, R


def hv3_rank(Y, r, n_pick=32, fast=True):
    """(dominated_by, dominates, s, picks, keys, counts, R), as ``hv_oracle.hv_rank``."""
    Y = np.asarray(Y, dtype=np.float64)
    by, of = (PO.pareto_counts_fast if fast else PO.pareto_counts)(Y)
    picks, keys, counts, R = hv3_select(Y, by, r, n_pick)
    return by, of, HO.hv_surrogate(by, of, PO.complete_rows(Y), picks, R), picks, keys, counts, R
