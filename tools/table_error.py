#!/usr/bin/env python
"""numpy emulation of the Chebyshev tables of the large-draw scorer
(k_table_build): for every bounded continuous hp of a history and
both sides of its split, the panels, their 16-node interpolants of the
linear-domain mixture g(y') and the per-panel certificate, then the measured
relative error at random points of each panel against the certified bound.

    python tools/table_error.py                 # the test shape (tests/test_gpu_table.py)
    python tools/table_error.py --gap u:-1.5:1.5
    python tools/table_error.py --cfg4 --every 7

--gap LABEL:LO:HI moves the history values of LABEL inside (LO, HI) out of the
interval (an empty gap: the edge components widen, the panels beside them lose
their certificate).  Prints one line per (hp, side) and exits 0.
"""
import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import tpe_oracle as O  # noqa: E402

NODES = 16
MAX_PANELS = 64
L2E = 1.4426950408889634
L16 = math.log2(math.factorial(16))
LOG2_CRAMER = math.log2(1.086435)
BAR = -28.0


def _lse2(t, axis=-1):
    """log2 sum 2^t along axis."""
    m = np.max(t, axis=axis, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    return np.squeeze(m, axis) + np.log2(np.sum(np.exp2(t - m), axis=axis))


def terms(w, mu, sigma, center):
    """(cc, a2, mu') of the log2-domain terms t_k = cc - a2 (y' - mu')^2."""
    sp = np.maximum(sigma, 1e-12)
    cc = L2E * (np.log(w) - np.log(sp * math.sqrt(2.0 * math.pi)))
    return cc, 0.5 * L2E / (sp * sp), mu - center


def log2_g(y, cc, a2, m):
    return _lse2(cc[None, :] - a2[None, :] * (y[:, None] - m[None, :]) ** 2)


def build(w, mu, sigma, low, high, center):
    """Panels of one mixture: dict(P, y_lo, width, M[P], coef[P, 16],
    log2_err[P], log2_glb[P], ok[P]) or None when it takes no table."""
    cc, a2, m = terms(w, mu, sigma, center)
    y_lo, y_hi = low - center, high - center
    sig = math.sqrt(0.5 * L2E / a2.max())
    Pd = math.ceil((y_hi - y_lo) / (2.0 * sig))
    if not 1 <= Pd <= MAX_PANELS:
        return None
    P = int(Pd)
    width = (y_hi - y_lo) / P
    H = 0.5 * width
    j = np.arange(NODES)
    xn = np.cos(np.pi * (2 * j + 1) / 32.0)
    T = np.cos(np.pi * np.outer(np.arange(NODES), 2 * j + 1) / 32.0) * (2.0 / NODES)
    T[0] *= 0.5
    out = dict(P=P, y_lo=y_lo, width=width, M=np.zeros(P), coef=np.zeros((P, NODES)),
               log2_err=np.zeros(P), log2_glb=np.zeros(P), ok=np.zeros(P, dtype=bool))
    for p in range(P):
        pl, ph = y_lo + width * p, y_lo + width * (p + 1)
        lg = log2_g(pl + H + H * xn, cc, a2, m)
        M = math.ceil(lg.max())
        f = np.exp2(lg - M)
        c = T @ f
        d = np.maximum(0.0, np.maximum(pl - m, m - ph))
        df = np.maximum(m - pl, ph - m)
        e = _lse2(cc + 8.0 * np.log2(2.0 * a2 / L2E) - 0.5 * a2 * d * d)
        le = LOG2_CRAMER + 0.5 * L16 + e + 16.0 * math.log2(H) - 15.0 - L16
        lr = M + math.log2(np.abs(c).sum()) - 46.0
        glb = _lse2(cc - a2 * df * df)
        out['M'][p], out['coef'][p] = M, c
        out['log2_err'][p], out['log2_glb'][p] = max(le, lr) + 1.0, glb
        out['ok'][p] = bool(np.isfinite(le) and np.isfinite(glb) and (f > 0).all() and
                            max(le, lr) + 1.0 <= glb + BAR)
    return out


def evaluate(tab, y):
    u = (y - tab['y_lo']) / tab['width']
    p = np.clip(np.floor(u), 0, tab['P'] - 1).astype(int)
    t = np.clip(2.0 * (u - p) - 1.0, -1.0, 1.0)
    c = tab['coef'][p]
    b1 = np.zeros_like(t)
    b2 = np.zeros_like(t)
    for k in range(NODES - 1, 0, -1):
        b1, b2 = 2.0 * t * b1 + (c[:, k] - b2), b1
    return tab['M'][p] + np.log2(t * b1 + (c[:, 0] - b2))


def report(label, side, w, mu, sigma, low, high, center, rs, pts=200):
    tab = build(w, mu, sigma, low, high, center)
    if tab is None:
        print('%-4s %-5s K=%-5d no table (panel count out of range)' % (label, side, w.size))
        return None
    cc, a2, m = terms(w, mu, sigma, center)
    worst = 0.0
    for p in range(tab['P']):
        y = tab['y_lo'] + tab['width'] * (p + rs.rand(pts))
        worst = max(worst, float(np.max(np.abs(np.exp2(evaluate(tab, y) - log2_g(y, cc, a2, m)) - 1.0))))
    cert = float(np.exp2((tab['log2_err'] - tab['log2_glb']).max()))
    bad = int((~tab['ok']).sum())
    print('%-4s %-5s K=%-5d panels=%-3d measured=%.2e certified<=%.2e (bar %.2e) uncertified=%d'
          % (label, side, w.size, tab['P'], worst, cert, 2.0 ** BAR, bad))
    return tab


def test_shape(n=6000, gap=None):
    """History of tests/test_gpu_table.py: uniform(-5, 5) 'u', loguniform 'lu'
    (and a normal that takes no table), RandomState(11) / (12)."""
    rs = np.random.RandomState(11)
    cols = {'u': rs.uniform(-5, 5, n), 'n': rs.normal(0.5, 2.0, n),
            'lu': np.exp(rs.uniform(math.log(1e-3), math.log(10), n))}
    if gap:
        cols[gap[0]] = apply_gap(cols[gap[0]], gap[1], gap[2], log=gap[0] == 'lu')
    losses = np.random.RandomState(12).rand(n)
    specs = {'u': ('uniform', (-5.0, 5.0)), 'lu': ('loguniform', (math.log(1e-3), math.log(10)))}
    return losses, cols, specs


def apply_gap(v, lo, hi, log=False):
    """Values inside (lo, hi) move out of it by the gap's width, away from its
    middle (lo, hi in the fitted domain: log x for a loguniform)."""
    x = np.log(v) if log else v.copy()
    mid, wd = 0.5 * (lo + hi), hi - lo
    ins = (x > lo) & (x < hi)
    x = np.where(ins & (x < mid), x - wd, np.where(ins, x + wd, x))
    return np.exp(x) if log else x


def run(losses, cols, specs, every=1):
    rs = np.random.RandomState(5)
    tids = np.arange(losses.size)
    tabs = {}
    for i, (label, (dist, args)) in enumerate(specs.items()):
        if i % every:
            continue
        fk, pm, ps, low, high, q, tr = O.posterior_spec(dist, args, 1.0)
        bo, ao = O.split_observations(tids, cols[label], tids, losses, 0.25, kind='stable')
        for side, obs in (('below', bo), ('above', ao)):
            w, mu, sg = O.parzen_fit(O.transform_obs(obs, tr, low), 1.0, pm, ps, kind='stable')
            tabs[label, side] = report(label, side, np.asarray(w), np.asarray(mu), np.asarray(sg),
                                       low, high, pm, rs)
    return tabs


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument('--n', type=int, default=6000)
    ap.add_argument('--gap', default=None, help='LABEL:LO:HI')
    ap.add_argument('--cfg4', action='store_true', help="bench.py config 4's history")
    ap.add_argument('--every', type=int, default=1, help='every n-th hp')
    a = ap.parse_args()
    if a.cfg4:
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        import bench
        dom, losses, vals, act = bench.build_workload('cfg4')
        cols = {h.label: vals[h.index] for h in dom.space.hps}
        specs = {h.label: ('uniform', (-5.0, 5.0)) for h in dom.space.hps}
    else:
        gap = None
        if a.gap:
            lab, lo, hi = a.gap.split(':')
            gap = (lab, float(lo), float(hi))
        losses, cols, specs = test_shape(a.n, gap)
    run(losses, cols, specs, a.every)


if __name__ == '__main__':
    main()
