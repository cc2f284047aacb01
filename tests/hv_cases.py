"""Objective matrices for the hypervolume subset selection tests (host and
GPU): a mutually nondominated front on the unit simplex, dominated rows behind
it, and the rows the rule singles out -- a duplicated front row whose copies
differ in the sign of a zero, a front row outside the reference point, NaN and
+inf (pending) rows and a -inf row (complete, excluded from the selection).
Test infrastructure only."""
import numpy as np

REF = 1.1                # the reference point of every case, per objective


def make_case(seed, M, n, frac_front=0.6):
    """(Y[M, n], r[M]).  n >= 8: every special row is present; smaller n: a
    plain front."""
    rng = np.random.RandomState(seed)
    k = n if n < 8 else max(6, int(frac_front * n))
    g = rng.gamma(1.0, size=(M, k)) + 1e-3
    Y = np.empty((M, n))
    Y[:, :k] = g / g.sum(axis=0)                        # on the simplex: nondominated
    for j in range(k, n):                               # behind a front row
        Y[:, j] = Y[:, rng.randint(k)] + 0.3 * rng.rand(M) + 1e-3
    r = np.full(M, REF)
    if n < 8:
        return Y, r
    a = int(np.argmin(Y[0, :k]))                        # (lowering the lowest changes no dominance)
    Y[:, [0, a]] = Y[:, [a, 0]]
    Y[0, 0] = 0.0                                       # the best of objective 0 ...
    Y[:, 1] = Y[:, 0]
    Y[0, 1] = -0.0                                      # ... twice: equal rows, another zero
    Y[:, 2] = -0.1                                      # a front row outside r
    Y[0, 2] = REF + 0.4
    Y[:, 3] = np.nan                                    # pending
    Y[0, n - 1] = np.nan                                # pending (one objective missing)
    Y[1, n - 2] = np.inf                                # pending
    Y[:, n - 3] = 2.0                                   # complete, not finite: no part in the selection
    Y[0, n - 3] = -np.inf
    perm = rng.permutation(n)
    return np.ascontiguousarray(Y[:, perm]), r


def outside_case(seed, M, n):
    """Every front row lies outside r in objective 0: R = 0."""
    Y, r = make_case(seed, M, n)
    r = r.copy()
    r[0] = -5.0
    return Y, r
