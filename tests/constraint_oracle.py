"""numpy restatement of the constrained-dominance rule.

``G[C, n]``: trial i is feasible when every ``G[c, i] <= 0``.  Its violation is
``((0.0 + max0(G[0, i])) + max0(G[1, i])) + ...`` in ascending c, ``max0(g) = g
if g > 0 else 0.0``, and +inf when any ``G[c, i]`` is NaN.  Completeness is
``pareto_oracle``'s and reads ``Y`` alone.  For complete rows, j c-dominates i
when ``v[j] < v[i]``, or when both are 0 and j Pareto-dominates i.
"""
import numpy as np

import pareto_oracle as PO


def history(n, M, C, feasible=None):
    """(Y[M, n], G[C, n]): ties, -0.0 / +0.0, duplicate rows and, from 16 rows on, pending
    rows and NaN, +-inf and overflowing constraints; ``feasible``: every row / no row."""
    rng = np.random.default_rng(10000 * M + 100 * C + n)
    Y = rng.choice([-1.0, 0.0, 0.5, 2.0], size=(M, n))
    G = rng.choice([-2.0, -0.0, 0.0, 0.5, 0.5, 3.0], size=(C, n))
    if n >= 16:
        Y[0, 3], Y[M - 1, 4], Y[0, 5], Y[0, n - 1] = np.nan, np.inf, -np.inf, np.nan
        Y[:, 9] = Y[:, 10]
        G[0, 6], G[C - 1, 7], G[0, 8], G[0, 3] = np.nan, np.inf, -np.inf, 1.0
        G[:, 9] = G[:, 10] = -1.0                       # a feasible duplicate pair
        G[:, n - 2] = 1e308                             # the sum overflows from C = 2 on
    if feasible is True:
        G = -np.abs(G)
        G[np.isnan(G)] = -np.inf
    elif feasible is False:
        G[0] = np.abs(G[0]) + 0.25
    return Y, G


def violation(G):
    G = np.asarray(G, dtype=np.float64)
    v = np.zeros(G.shape[1])
    with np.errstate(over='ignore', invalid='ignore'):
        for c in range(G.shape[0]):                     # ascending c, one rounded sum each
            v = v + np.where(G[c] > 0, G[c], 0.0)
    v[np.isnan(G).any(axis=0)] = np.inf
    return v


def constraint_rank(Y, G):
    """(v, dominated_by, dominates, s) of ``Y[M, n]`` under ``G[C, n]``."""
    Y = np.asarray(Y, dtype=np.float64)
    n = Y.shape[1]
    v = violation(G)
    ok = PO.complete_rows(Y)
    feas = ok & (v == 0)
    by = np.zeros(n, dtype=np.int32)
    of = np.zeros(n, dtype=np.int32)
    for i in np.flatnonzero(ok):
        dom = ok & (v < v[i])                           # j violates less
        if feas[i]:
            yi = Y[:, i:i + 1]
            with np.errstate(invalid='ignore'):
                dom |= feas & (Y <= yi).all(axis=0) & (Y < yi).any(axis=0)
        by[i] = dom.sum()
        of[dom] += 1
    return v, by, of, PO.surrogate(by, of, ok)
