"""c-TPE in numpy over the existing oracles: each model's good-side count, the
per-model lpdfs of whole configurations under the oracle's fits, and the acquisition."""
import math

import numpy as np

from oracle import tpe_oracle as O
from oracle_algo import oracle_hps

BIG_GAMMA = 1e9     # with gamma_cap = nb the oracle's split takes exactly nb rows


def counts(losses, G, gamma=0.25, gamma_cap=25):
    """(nb[C + 1], ghat[C + 1], live) by the rule as written, row by row."""
    losses, G = np.asarray(losses, dtype=np.float64), np.asarray(G, dtype=np.float64)
    n, C = losses.size, G.shape[0]
    complete = [math.isfinite(l) for l in losses]
    n_c = sum(complete)
    plain = max(0, min(int(math.ceil(gamma * math.sqrt(n))), gamma_cap))
    nb = [plain]
    order = sorted(range(n), key=lambda i: (losses[i], i))      # the stable loss order
    for rank, i in enumerate(order, 1):
        if complete[i] and all(G[c][i] <= 0 for c in range(C)):
            nb[0] = max(plain, rank)
            break
    for c in range(C):
        feasible = sum(1 for i in range(n) if complete[i] and G[c][i] <= 0)
        nb.append(min(max(feasible, plain), n_c))
    ghat = [min(b, n_c) / n_c for b in nb]
    live = [m for m in range(C + 1) if m == 0 or ghat[m] < 1.0]
    return np.array(nb, dtype=np.int32), np.array(ghat), live


def keys(losses, G):
    """Every model's key column: the losses, then G with +inf where pending or NaN."""
    losses, G = np.asarray(losses, dtype=np.float64), np.asarray(G, dtype=np.float64)
    dead = ~np.isfinite(losses)[None, :] | np.isnan(G)
    return np.concatenate([losses[None, :], np.where(dead, np.inf, G)])


def model_lliks(cs, key, nb, hist_vals, hist_active, vals, active, prior_weight=1.0):
    """(llik_b, llik_a)[P, M] under the oracle's fit of the history split on ``key`` at ``nb``."""
    hps = oracle_hps(cs)
    tids = np.arange(key.size)
    lb, la = np.full(vals.shape, np.nan), np.full(vals.shape, np.nan)
    for i, lab in enumerate(cs.labels):
        on, at = hist_active[i] == 1, active[i] == 1
        if not at.any():
            continue
        bo, ao = O.split_observations(tids[on], hist_vals[i][on], tids, key, BIG_GAMMA, int(nb),
                                      kind='stable')
        with np.errstate(all='ignore'):
            r = O.score_hp(hps[lab]['dist'], hps[lab]['args'], bo, ao, prior_weight, vals[i][at],
                           kind='stable')
        lb[i, at], la[i, at] = r['llik_b'], r['llik_a']
    return lb, la


def log_ratio(ghat, T):
    """L = log(ghat + (1 - ghat) exp(-T)), evaluated as the engine states it."""
    T = np.asarray(T, dtype=np.float64)
    with np.errstate(all='ignore'):
        u = np.full(T.shape, np.log(ghat))
        v = np.log1p(-ghat) - T
        hi, lo = np.where(u > v, u, v), np.where(u > v, v, u)
        return np.where(hi == np.inf, np.inf, hi + np.log1p(np.exp(lo - hi)))


def acquisition(ghat_live, T):
    """acq[M] from the live models' ghat and totals T[n_live, M], in order."""
    acq = np.zeros(np.asarray(T).shape[1])
    for g, t in zip(ghat_live, T):
        acq = acq - log_ratio(g, t)
    return acq
