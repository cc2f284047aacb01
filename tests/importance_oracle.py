"""Importances from two fitted mixtures (include/tpe_engine.h states the rule) in
float64 numpy: the nodes and weights of an hp, the lpdfs of the existing oracle at them, the
integrand and the engine's fixed summation order.  A mixture is (w, mu, sigma), or p for the
categorical kinds, as ``Plan.mixture`` and ``oracle.tpe_oracle`` hand them out."""
import functools
import math

import numpy as np

from oracle import tpe_oracle as O

TILE = 256
_C = [1.0 / math.factorial(j) for j in range(14)]
_LN2_HI, _LN2_LO = float.fromhex('0x1.62e42fee00000p-1'), float.fromhex('0x1.a39ef35793c76p-33')


def node_exp(y):
    """exp(y) by the rule's fixed sequence of separately rounded operations."""
    k = np.rint(y * 1.4426950408889634)
    r = (y - k * _LN2_HI) - k * _LN2_LO
    p = np.full_like(y, _C[13])
    for j in range(12, -1, -1):
        p = p * r + _C[j]
    return np.ldexp(p, k.astype(np.int64))


def _stride(first, count, G, q=1.0):
    count = min(max(count, 0.0), 2.0 ** 52)
    s = math.ceil(count / G) if count > G else 1.0
    i = np.arange(int(math.ceil(count / s)), dtype=np.float64)
    return q * (first + i * s), np.full(i.size, float(s)), int(s)


def nodes(dist, args, below, above, G):
    """(x, w, s): the hp's nodes, their weights, and the lattice stride (1: every value)."""
    if dist in ('randint', 'categorical'):
        return _stride(0.0, float(len(below)), G)
    fk, _, ps, low, high, q, _ = O.posterior_spec(dist, args, 1.0)
    lo, hi = low, high
    if low is None:
        (b, a), r = (below[1], above[1]), 6.0 * ps
        lo, hi = min(b[0], a[0]) - r, max(b[-1], a[-1]) + r
    if q is None:
        h = (hi - lo) / G
        y = lo + (np.arange(G, dtype=np.float64) + 0.5) * h
        x = node_exp(y) if fk == 'lgmm' else y
        return x, (h * x if fk == 'lgmm' else np.full(G, h)), 1
    if fk == 'lgmm':
        lo, hi = math.exp(lo), math.exp(hi)
    j0, j1 = math.ceil(lo / q - 0.5), math.floor(hi / q + 0.5)
    if fk == 'lgmm':
        j0 = max(j0, 0.0)
    if low is not None:
        j0 += q * j0 + q / 2.0 < lo
        j1 -= q * j1 - q / 2.0 > hi
    return _stride(float(j0), float(j1) - float(j0) + 1.0, G, q)


def lpdfs(dist, args, below, above, x):
    """(lb, la): the oracle's log densities of the two mixtures at the nodes."""
    with np.errstate(all='ignore'):
        if dist in ('randint', 'categorical'):
            return O.categorical_lpdf(x, below), O.categorical_lpdf(x, above)
        fk, _, _, low, high, q, _ = O.posterior_spec(dist, args, 1.0)
        f = O.lgmm_lpdf if fk == 'lgmm' else O.gmm_lpdf
        return f(x, *below, low=low, high=high, q=q), f(x, *above, low=low, high=high, q=q)


def tiled_sum(v):
    """The engine's order: per tile of 256 the tree v[t] += v[t + s], then tiles ascending."""
    t = np.zeros(-(-v.size // TILE) * TILE)
    t[:v.size] = v
    t = t.reshape(-1, TILE)
    s = TILE // 2
    while s:
        t[:, :s] += t[:, s:2 * s]
        s //= 2
    return functools.reduce(lambda a, b: a + b, t[:, 0].tolist(), 0.0)


def integrate(lb, la, w, ghat, rtol=0.0):
    """dict(D, mass, S = sum |f|, B): the importance of one (model, hp) from its log densities;
    B bounds the change of D when l and g move by rtol (max(1, |lb|) + max(1, |la|)) each."""
    with np.errstate(all='ignore'):
        hi = np.maximum(lb, la)
        on = hi != -np.inf
        hi = np.where(on, hi, 0.0)
        ea, eb = np.where(on, np.exp(lb - hi), 0.0), np.where(on, np.exp(la - hi), 0.0)
        den = np.where(on, ghat * ea + (1.0 - ghat) * eb, 1.0)
        we = w * np.exp(hi)
        f = np.where(on, we * ((ea - eb) * (ea - eb)) / den, 0.0)
        qw = np.where(on, we * den, 0.0)
        mag = [np.maximum(1.0, np.where(np.isfinite(a), np.abs(a), 0.0)) for a in (lb, la)]
        b = np.where(on, rtol * (mag[0] + mag[1]) * we * (ea + eb) ** 2 / den, 0.0)
    c = (1.0 - ghat) * (1.0 - ghat)
    return dict(D=0.0 if ghat == 1.0 else c * tiled_sum(f), mass=tiled_sum(qw),
                S=float(np.abs(f).sum()), B=c * float(b.sum()))


def importance(dist, args, below, above, ghat, G=1024):
    x, w, _ = nodes(dist, args, below, above, G)
    return integrate(*lpdfs(dist, args, below, above, x), w, ghat)
