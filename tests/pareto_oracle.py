"""numpy restatement of the Pareto ranking rule: the double
loop, the two counts and the surrogate loss.  Test infrastructure only.

Every objective is minimised.  A row of ``Y[M, n]`` is complete when none of
its objectives is NaN or +inf, pending otherwise.  For complete rows, j
dominates i when ``Y[m, j] <= Y[m, i]`` for every m and ``Y[m, j] < Y[m, i]``
for some m (IEEE comparison: -0.0 == +0.0, -inf an ordinary value).
"""
import numpy as np


def complete_rows(Y):
    Y = np.asarray(Y, dtype=np.float64)
    return ~(np.isnan(Y) | (Y == np.inf)).any(axis=0)


def dominates(a, b):
    """Row a dominates row b (two complete rows, as 1-d arrays)."""
    return bool((a <= b).all() and (a < b).any())


def pareto_counts(Y):
    """(dominated_by int32[n], dominates int32[n]) by the double loop."""
    Y = np.asarray(Y, dtype=np.float64)
    n = Y.shape[1]
    ok = complete_rows(Y)
    by = np.zeros(n, dtype=np.int32)
    of = np.zeros(n, dtype=np.int32)
    for i in range(n):
        if not ok[i]:
            continue
        for j in range(n):
            if ok[j] and dominates(Y[:, j], Y[:, i]):
                by[i] += 1
                of[j] += 1
    return by, of


def pareto_counts_fast(Y):
    """The same counts with the inner loop vectorised (larger n)."""
    Y = np.asarray(Y, dtype=np.float64)
    n = Y.shape[1]
    ok = complete_rows(Y)
    by = np.zeros(n, dtype=np.int32)
    of = np.zeros(n, dtype=np.int32)
    for i in np.flatnonzero(ok):
        yi = Y[:, i:i + 1]
        with np.errstate(invalid='ignore'):
            dom = ok & (Y <= yi).all(axis=0) & (Y < yi).any(axis=0)     # j dominates i
        by[i] = dom.sum()
        of[dom] += 1
    return by, of


def surrogate(by, of, ok):
    """s = dominated_by (n + 1) + (n - dominates); +inf for a pending row."""
    n = len(by)
    assert (n + 1) ** 2 < 2 ** 53
    s = (by.astype(np.int64) * (n + 1) + (n - of.astype(np.int64))).astype(np.float64)
    s[~np.asarray(ok)] = np.inf
    return s


def pareto_rank(Y, fast=False):
    """(dominated_by, dominates, s) of ``Y[M, n]``."""
    by, of = (pareto_counts_fast if fast else pareto_counts)(Y)
    return by, of, surrogate(by, of, complete_rows(Y))
