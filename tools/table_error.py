#!/usr/bin/env python
"""numpy emulation of the Chebyshev tables of the large-draw scorer
(k_table_build): for every bounded continuous hp of a history and
both sides of its split, the panels, their 16-node interpolants of the
linear-domain mixture g(y') and the per-panel certificate, then the measured
relative error at random points of each panel against the certified bound.

    python tools/table_error.py                 # the test shape (tests/test_gpu_table.py)
    python tools/table_error.py --gap u:-1.5:1.5
    python tools/table_error.py --cfg4 --every 7
    python tools/table_error.py --prefilter          # and --cfg4 --every 37, --low-edge
    python tools/table_error.py --drawprune          # and --cfg4 --only 0,42,76, --shape band
    python tools/table_error.py --fit-set pw-zero --drawprune    # or --gamma 1 --gamma-cap 200 ...

--gap LABEL:LO:HI moves the history values of LABEL inside (LO, HI) out of the
interval (an empty gap: the edge components widen, the panels beside them lose
their certificate).  Prints one line per (hp, side) and exits 0.

--prefilter adds, per hp with two certified tables, the emulation of the table
pass's prefilter (bound lattice, hot intervals, bucketed wave tiles) on
--draws draws of the below mixture: cells hot, wave tiles passing, hot wave
tiles missed (which must be 0).  --low-edge takes a history whose good trials
cluster at the lower bound instead of the test shape; --shape NAME another of
the named histories (NAMED: high-edge, band, ties, comb), which the CPU and
the GPU tests of the prefilter share.

--drawprune adds the emulation of the pruning sorted draw (k_draw_sorted_prune,
DESIGN 5.6) on the same draws and bucketing: per hp the share of the wave
tiles the draw keeps (beside the exact filter's passing share), the share of
the elements it ranks, and the hot wave tiles it drops (which must be 0).
--only I,J,... takes just those hps.

--gamma, --gamma-cap, --prior-weight and --lf are the fit parameters of
tpe_plan_fit (defaults 0.25, 25, 1.0, 25); --fit-set NAME takes those of one
of the named sets (FIT_SETS), which the CPU and the GPU tests of the table
path away from the default fit share.
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


def terms(w, mu, sigma, center, pacc=1.0):
    """(cc, a2, mu') of the log2-domain terms t_k = cc - a2 (y' - mu')^2.
    pacc: the truncation mass make_coef folds into a GMM's constants (an
    LGMM's carry none: 1)."""
    sp = np.maximum(sigma, 1e-12)
    cc = L2E * (np.log(w) - np.log(sp * math.sqrt(2.0 * math.pi)) - math.log(pacc))
    return cc, 0.5 * L2E / (sp * sp), mu - center


def log2_g(y, cc, a2, m):
    return _lse2(cc[None, :] - a2[None, :] * (y[:, None] - m[None, :]) ** 2)


def build(w, mu, sigma, low, high, center, pacc=1.0):
    """Panels of one mixture: dict(P, y_lo, width, M[P], coef[P, 16],
    log2_err[P], log2_glb[P], ok[P]) or None when it takes no table."""
    cc, a2, m = terms(w, mu, sigma, center, pacc)
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


# ---- the prefilter of the table pass (k_table_bound / k_table_pilot /
# tab_prefilter): bound lattice, hot intervals, bucketed waves ----
CELLS = 4096          # kBndCells
HOT_IV = 8            # kHotIv
WIDEN = 2.0 ** -20    # kBndWiden
PILOT_WAVES = 64      # kPilotWaves
TIE = 2.0 ** -16      # kTabTie
SORT_BLOCK, BUCKETS, WAVE = 8192, 256, 128
LN2 = 0.6931471805599453
_K = np.arange(NODES, dtype=np.float64)
_K2 = _K * _K
_K4 = _K2 * (_K2 - 1.0) / 3.0


def _panel(tab, y):
    u = (y - tab['y_lo']) / tab['width']
    p = np.clip(np.floor(u), 0, tab['P'] - 1).astype(int)
    return p, np.clip(2.0 * (u - p) - 1.0, -1.0, 1.0)


def _clenshaw(c, t):
    b1 = np.zeros_like(t)
    b2 = np.zeros_like(t)
    for k in range(NODES - 1, 0, -1):
        b1, b2 = 2.0 * t * b1 + (c[:, k] - b2), b1
    return t * b1 + (c[:, 0] - b2)


def score(tb, ta, y):
    """The table score as the map computes it: ((M_b - M_a) + log2(s_b / s_a)) ln 2,
    y' clamped into the tables' range by the panel coordinates."""
    y = np.asarray(y, dtype=np.float64)
    pb, tbv = _panel(tb, y)
    pa, tav = _panel(ta, y)
    sb, sa = _clenshaw(tb['coef'][pb], tbv), _clenshaw(ta['coef'][pa], tav)
    return ((tb['M'][pb] - ta['M'][pa]) + np.log2(sb / sa)) * LN2


def _next_edge(tab, x):
    j = np.floor((x - tab['y_lo']) / tab['width']) + 1.0
    e = tab['y_lo'] + j * tab['width']
    return np.where(e > x, e, tab['y_lo'] + (j + 1.0) * tab['width'])


def _bound_side(tab, xa, xb):
    p, _ = _panel(tab, 0.5 * (xa + xb))
    c = tab['coef'][p]
    inv_w = 1.0 / tab['width']
    ta = np.clip(2.0 * ((xa - tab['y_lo']) * inv_w - p) - 1.0, -1.0, 1.0)
    tb = np.clip(2.0 * ((xb - tab['y_lo']) * inv_w - p) - 1.0, -1.0, 1.0)
    a = np.abs(c)
    s0, s1, s2 = a.sum(1), (a * _K2).sum(1), (a * _K4).sum(1)
    va, vb = _clenshaw(c, ta), _clenshaw(c, tb)
    d1, d2 = s1 * 2.0 * inv_w, s2 * 4.0 * inv_w * inv_w
    e = s0 * 2.0 ** -46 + s1 * 2.0 ** -40
    h = xb - xa
    return dict(va=va, vb=vb, d1=d1, d2=d2, e=e, lo=np.minimum(va, vb) - h * h * 0.125 * d2 - e,
                M=tab['M'][p])


def bound_lattice(tb, ta, cells=CELLS):
    """U[c] >= the table score anywhere in cell c of `cells` equal cells of
    [y_lo, y_hi] (k_table_bound): per piece between panel edges the end-point
    scores plus (piece width)^2 / 8 max|S''| plus the rounding slack; +inf
    where no bound holds."""
    y_lo = tb['y_lo']
    y_hi = y_lo + tb['width'] * tb['P']
    cw = (y_hi - y_lo) / cells
    c = np.arange(cells, dtype=np.float64)
    a0 = np.maximum(y_lo, y_lo + cw * (c - WIDEN))
    b0 = np.minimum(y_hi, y_lo + cw * (c + 1.0 + WIDEN))
    a0[0], b0[-1] = y_lo, y_hi
    U = np.full(cells, -np.inf)
    ok = a0 < b0
    x = a0.copy()
    with np.errstate(all='ignore'):
        for _ in range(8):
            act = ok & (x < b0)
            if not act.any():
                break
            xs = x[act]
            nx = np.minimum(b0[act], np.minimum(_next_edge(tb, xs), _next_edge(ta, xs)))
            B, A = _bound_side(tb, xs, nx), _bound_side(ta, xs, nx)
            la, lb, dm = np.log2(B['va'] / A['va']), np.log2(B['vb'] / A['vb']), B['M'] - A['M']
            sa, sb = (dm + la) * LN2, (dm + lb) * LN2
            gb, ga = B['d1'] / B['lo'], A['d1'] / A['lo']
            curv = B['d2'] / B['lo'] + gb * gb + A['d2'] / A['lo'] + ga * ga
            slack = (2.0 * (B['e'] / B['lo'] + A['e'] / A['lo']) +
                     2.0 ** -40 * (1.0 + np.abs(dm) + np.abs(la) + np.abs(lb)))
            h = nx - xs
            u = np.maximum(sa, sb) + h * h * 0.125 * curv + slack
            good = (B['lo'] > 0) & (A['lo'] > 0) & np.isfinite(u) & ~np.isnan(sa) & ~np.isnan(sb)
            idx = np.flatnonzero(act)
            ok[idx] &= good
            U[idx] = np.fmax(U[idx], u)
            x[idx] = nx
    ok &= ~(x < b0)
    return np.where(ok, U, np.inf)


def hot_intervals(U, L0, y_lo, y_hi, tie=TIE):
    """k_table_pilot's intervals: the cells with !(U < T0), each widened by one
    cell on both sides, merged into at most HOT_IV closed y' intervals (the
    nearest runs first).  Returns (intervals, hot cell mask)."""
    cells = U.size
    cw = (y_hi - y_lo) / cells
    if not np.isfinite(L0):
        return [(-np.inf, np.inf)], np.ones(cells, dtype=bool)
    with np.errstate(all='ignore'):
        T0 = L0 - tie * max(1.0, abs(L0))
        hot = ~(U < T0)
    runs = []
    d = np.diff(np.concatenate([[0], hot.astype(np.int8), [0]]))
    for c, e in zip(np.flatnonzero(d == 1), np.flatnonzero(d == -1)):   # cells c .. e - 1
        a0, a1 = max(c - 1, 0), min(e, cells - 1)
        if runs and a0 <= runs[-1][1] + 1:
            runs[-1][1] = a1
            continue
        runs.append([a0, a1])
        if len(runs) > HOT_IV:
            gaps = [runs[j][0] - runs[j - 1][1] for j in range(1, len(runs))]
            j = 1 + int(np.argmin(gaps))
            runs[j - 1][1] = runs[j][1]
            del runs[j]
    return [(-np.inf if a == 0 else y_lo + cw * a, np.inf if b == cells - 1 else y_lo + cw * (b + 1))
            for a, b in runs], hot


def hot_runs(hot):
    """The pilot's runs before it merges any: runs of the hot cell mask after
    each is widened by one cell on both sides and touching ones are joined."""
    d = hot.copy()
    d[:-1] |= hot[1:]
    d[1:] |= hot[:-1]
    return int((np.diff(np.concatenate([[0], d.astype(np.int8)])) == 1).sum())


def draw_below(w, mu, sigma, low, high, center, n, rs):
    """n draws of the truncated mixture, as y' (rejection, numpy's stream)."""
    out = np.empty(0)
    p = np.asarray(w) / np.sum(w)
    while out.size < n:
        k = rs.choice(p.size, size=2 * n, p=p)
        x = rs.normal(np.asarray(mu)[k], np.asarray(sigma)[k])
        out = np.concatenate([out, x[(x >= low) & (x < high)]])
    return out[:n] - center


def bucketed_waves(y, y_lo, y_hi):
    """The draw's value bucketing (k_draw_sorted): sort blocks of SORT_BLOCK
    candidates, each grouped stably into BUCKETS equal-width buckets of
    [y_lo, y_hi]; wave tiles are WAVE consecutive candidates of the result.
    Returns (y in bucketed order, list of (begin, end) per wave tile)."""
    out = np.empty_like(y)
    for b0 in range(0, y.size, SORT_BLOCK):
        blk = y[b0:b0 + SORT_BLOCK]
        key = np.clip(np.floor((blk - y_lo) / (y_hi - y_lo) * BUCKETS), 0, BUCKETS - 1)
        out[b0:b0 + blk.size] = blk[np.argsort(key, kind='stable')]
    return out, [(i, min(i + WAVE, y.size)) for i in range(0, y.size, WAVE)]


def prefilter(tb, ta, y, tie=TIE, cells=CELLS):
    """The whole prefilter on bucketed candidates y (one launch): dict with
    the lattice U, the hot cell mask, the intervals, per wave tile its best
    score `wmax` and whether it is pruned, the slot's tab_max and the
    threshold T(tab_max) of k_tie_gather."""
    y_lo = tb['y_lo']
    y_hi = y_lo + tb['width'] * tb['P']
    U = bound_lattice(tb, ta, cells)
    yb, waves = bucketed_waves(y, y_lo, y_hi)
    sc = score(tb, ta, yb)
    wmax = np.array([sc[a:b].max() for a, b in waves])
    L0 = wmax[:PILOT_WAVES].max()
    iv, hot = hot_intervals(U, L0, y_lo, y_hi, tie)
    yc = np.clip(yb, y_lo, y_hi)
    pruned = np.ones(len(waves), dtype=bool)
    for i, (a, b) in enumerate(waves):
        mn, mx = yc[a:b].min(), yc[a:b].max()
        pruned[i] = not any(mx >= lo and mn <= hi for lo, hi in iv)
    tab_max = wmax.max()
    return dict(U=U, hot=hot, intervals=iv, wmax=wmax, pruned=pruned, L0=L0, tab_max=tab_max,
                thr=tab_max - tie * max(1.0, abs(tab_max)))


def draw_prune(tb, ta, y, tie=TIE, cells=CELLS):
    """The pruning draw on the candidates y of one launch (draw order), on top
    of prefilter(): sort block 0 is the pilot's and kept whole; in every other
    block a bucket is hot when one of its elements' clamped y' lies in a hot
    interval (a NaN counts), a wave tile is kept iff its position range meets
    that of a non-empty hot bucket, and a bucket is live -- its elements are
    ranked -- iff its position range meets a kept tile.  Adds `kept` per wave
    tile, `live` (share of the elements behind block 0 that are ranked) and
    `dropped_hot`, the wave tiles dropped although their best score reaches
    k_tie_gather's threshold."""
    r = prefilter(tb, ta, y, tie, cells)
    y_lo = tb['y_lo']
    y_hi = y_lo + tb['width'] * tb['P']
    n = y.size
    kept = np.ones((n + WAVE - 1) // WAVE, dtype=bool)
    live = 0
    for b0 in range(SORT_BLOCK, n, SORT_BLOCK):
        blk = y[b0:b0 + SORT_BLOCK]
        key = np.clip(np.floor((blk - y_lo) / (y_hi - y_lo) * BUCKETS), 0, BUCKETS - 1).astype(int)
        yc = np.clip(blk, y_lo, y_hi)
        hit = np.isnan(blk)
        for lo, hi in r['intervals']:
            hit |= (yc >= lo) & (yc <= hi)
        cnt = np.bincount(key, minlength=BUCKETS)
        base = np.cumsum(cnt) - cnt
        full = cnt > 0
        t0, t1 = base // WAVE, np.where(full, (base + cnt - 1) // WAVE, base // WAVE)
        hotb = full & (np.bincount(key[hit], minlength=BUCKETS) > 0)
        keep = np.zeros((blk.size + WAVE - 1) // WAVE, dtype=bool)
        for b in np.flatnonzero(hotb):
            keep[t0[b]:t1[b] + 1] = True
        ck = np.concatenate([[0], np.cumsum(keep)])
        liveb = full & (ck[np.minimum(t1 + 1, keep.size)] - ck[np.minimum(t0, keep.size)] > 0)
        live += int(cnt[liveb].sum())
        kept[b0 // WAVE:b0 // WAVE + keep.size] = keep
    hot_tiles = ~(r['wmax'] < r['thr'])
    return dict(r, kept=kept, live=live / max(1, n - min(n, SORT_BLOCK)),
                dropped_hot=int((hot_tiles & ~kept).sum()))


def _fmaf(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 is exact in fp64."""
    return np.float32(np.float64(a) * np.float64(b) + np.float64(c))


_ERFCINV_C = [2.81022636e-08, 3.43273939e-07, -3.5233877e-06, -4.39150654e-06, 0.00021858087,
              -0.00125372503, -0.00417768164, 0.246640727, 1.50140941]
_ERFCINV_T = [-0.000200214257, 0.000100950558, 0.00134934322, -0.00367342844, 0.00573950773,
              -0.0076224613, 0.00943887047, 1.00167406, 2.83297682]


def erfcinv_fast_emul(y):
    """erfcinv_fast (tpe_draw.hpp) on fp64 y in (0, 1], its fp32 steps in fp32:
    w = -ln(y (2 - y)) from the two mantissas' log2 (numpy's log2 for
    v_log_f32), both polynomials by fused multiply-adds, p (1 - y) in fp64;
    beyond w = 36 the fp64 erfcinv (scipy for OCML's)."""
    from scipy.special import erfcinv
    f = np.float32
    y = np.asarray(y, dtype=np.float64)
    m1, e1 = np.frexp(y)
    m2, e2 = np.frexp(2.0 - y)
    l2 = f(f(np.log2(m1.astype(f)) + np.log2(m2.astype(f))) + (e1 + e2).astype(f))
    w = f(f(-0.6931471805599453) * l2)
    wc = f(w - f(2.5))
    pc = np.full(y.shape, f(_ERFCINV_C[0]), dtype=f)
    for c in _ERFCINV_C[1:]:
        pc = _fmaf(pc, wc, f(c))
    with np.errstate(invalid='ignore'):
        wt = f(np.sqrt(w) - f(3.0))
    pt = np.full(y.shape, f(_ERFCINV_T[0]), dtype=f)
    for c in _ERFCINV_T[1:]:
        pt = _fmaf(pt, wt, f(c))
    out = np.where(w < f(5.0), pc, pt).astype(np.float64) * (1.0 - y)
    far = ~(w <= f(36.0))
    out[far] = erfcinv(y[far])
    return out


def erfcinv_grid(per_decade=20000):
    """A dense grid of y = 2 q in (0, 1]: log-spaced from 1e-17 (past the
    w > 36 hand-off) to 1, the approach to 1 from below, and the w = 5 and
    w = 36 switches themselves."""
    y = [np.logspace(-17, 0, 17 * per_decade + 1),
         1.0 - np.logspace(-16, -0.31, 16 * per_decade),
         np.linspace(0.5, 1.0, 8 * per_decade),
         1.0 - np.sqrt(1.0 - np.exp(-np.linspace(4.99, 5.01, per_decade))),
         1.0 - np.sqrt(1.0 - np.exp(-np.linspace(35.9, 36.1, per_decade)))]
    y = np.concatenate(y)
    return np.unique(y[(y > 0.0) & (y <= 1.0)])


def invert_error():
    """max |x drawn - x true| / sigma of draw_bounded_invert over erfcinv_grid:
    x = mu +- sqrt2 sigma erfcinv(2 q) in every mode of the table, so the
    error in sigma is sqrt2 |erfcinv_fast - erfcinv| whichever tail the mode
    inverts.  Per range of w: (label, max error, y at the maximum)."""
    from scipy.special import erfcinv
    y = erfcinv_grid()
    err = math.sqrt(2.0) * np.abs(erfcinv_fast_emul(y) - erfcinv(y))
    w = -np.log(y * (2.0 - y))
    rows = []
    for lab, sel in (('w < 5 (central)', w < 5.0),
                     ('5 <= w <= %.2f (screened tail)' % SCREEN_W_MAX, (w >= 5.0) & (w <= SCREEN_W_MAX)),
                     ('%.2f < w <= 36 (tail, never cold)' % SCREEN_W_MAX, (w > SCREEN_W_MAX) & (w <= 36.0)),
                     ('w > 36 (fp64 hand-off, never cold)', w > 36.0)):
        i = int(np.argmax(np.where(sel, err, -1.0)))
        rows.append((lab, float(err[i]), float(y[i])))
    return rows


# The screened draw (tpe_screen.hip): a draw whose tail probability q is under
# SCREEN_Q_MIN is always inverted (erfcinv_fast's tail polynomial drifts from
# w = 16 on, to ~1 sigma at w = 36), and the zone edges are widened by
# SCREEN_MARGIN sigma: at least 16 times invert_error()'s maximum over
# w <= SCREEN_W_MAX (the 16: v_log_f32 / v_sqrt_f32 against numpy's by an ulp)
SCREEN_Q_MIN = 2.0 ** -24
SCREEN_W_MAX = -math.log(2.0 * SCREEN_Q_MIN * (2.0 - 2.0 * SCREEN_Q_MIN))
SCREEN_MARGIN = 1.6e-5


def draw_table(w, mu, sigma, low, high):
    """build_table's per-component constants of a bounded mixture: (pick
    weights, base, mass, mode)."""
    from scipy.special import erfc
    w, mu, sigma = (np.asarray(v, dtype=np.float64) for v in (w, mu, sigma))
    s2 = 1.4142135623730951 * sigma
    za, zb = (low - mu) / s2, (high - mu) / s2
    mode = np.where(za >= 0.0, 1, np.where(zb <= 0.0, 2, 0))
    base = np.where(mode == 1, 0.5 * erfc(za), 0.5 * erfc(-za))
    mass = np.where(mode == 1, base - 0.5 * erfc(zb), 0.5 * erfc(-zb) - base)
    mass = np.where(mass > 0.0, mass, 0.0)
    return w * mass, base, mass, mode


def draw_invert_emul(base, mass, mode, mu, sigma, low, high, u1):
    """draw_bounded_invert (GMM, not quantized) with erfcinv_fast_emul: the
    value of component constants (arrays, broadcast against u1)."""
    um = u1 * mass
    pu, pp = base - um, base + um
    lower = (mode != 1) & ((mode == 2) | (pp < 0.5))
    q = np.where(mode == 1, pu, np.where(lower, pp, 1.0 - pp))
    with np.errstate(all='ignore'):
        e = erfcinv_fast_emul(np.where(q > 0.0, 2.0 * q, 1.0))
        e = np.where(q > 0.0, e, np.inf)
        x = np.where(lower, -1.0, 1.0) * (1.4142135623730951 * sigma) * e + mu
    x = np.where(x >= low, x, low)
    return np.where(x < high, x, np.nextafter(high, -np.inf))


def zone_crossed(u1, base, mass, mode, z, tail, up):
    """tpe_screen.hip's zone_crossed, operation for operation (arrays)."""
    um = u1 * mass
    pu, pp = base - um, base + um
    q1 = 1.0 - pp
    rho = 1e-13
    t_hi, t_lo = tail * (1.0 + rho), tail * (1.0 - rho)
    phi = (mode == 2) | ((mode == 0) & (z < 0.0))
    above = np.where(mode == 1, pu < t_lo, np.where(phi, pp > t_hi, (pp >= 0.5) & (q1 < t_lo)))
    below = np.where(mode == 1, pu > t_hi, np.where(phi, pp < t_lo, (pp < 0.5) | (q1 > t_hi)))
    ok_lo = (mode == 1) | (pp >= SCREEN_Q_MIN)
    deep_hi = np.where(mode == 1, pu < SCREEN_Q_MIN,
                       (mode == 0) & (pp >= 0.5) & (q1 < SCREEN_Q_MIN))
    return deep_hi | (ok_lo & np.where(up, above, ~below))


def zone_thresholds(zlo, zhi, base, mass, mode, mu, sigma, margin=None, integer=False):
    """k_draw_zone's u1 thresholds thr[K][2 (nz - 1)] of the disjoint value
    zones [zlo[i], zhi[i]] (ascending, the first from -inf, the last to +inf):
    component k's draw is cold in gap g iff thr[k][2g] <= u1 < thr[k][2g + 1].
    integer: its thrI = thr 2^53 as uint64 (2^53: none), for U1 = u1 2^53."""
    from scipy.special import erfc
    margin = SCREEN_MARGIN if margin is None else margin
    nz, K = len(zlo), len(mu)
    E = 2 * (nz - 1)
    e = np.arange(E)
    up = (e % 2 == 0)[None, :]
    edge = np.where(up, np.asarray(zhi, dtype=np.float64)[e // 2][None, :],
                    np.asarray(zlo, dtype=np.float64)[np.minimum(e // 2 + 1, nz - 1)][None, :])
    b, m, md, mu_, sg = (np.broadcast_to(np.asarray(v)[:, None], (K, E)) for v in
                         (base, mass, mode, mu, sigma))
    eps = np.finfo(np.float64).eps
    delta = margin * sg + 8.0 * eps * (np.abs(edge) + np.abs(mu_))
    v = np.where(up, edge + delta, edge - delta)
    z = (v - mu_) / (1.4142135623730951 * sg)
    tail = np.where((md == 1) | ((md == 0) & (z >= 0.0)), 0.5 * erfc(z), 0.5 * erfc(-z))
    lo = np.zeros((K, E), dtype=np.uint64)
    hi = np.full((K, E), 1 << 53, dtype=np.uint64)
    for _ in range(54):
        mid = (lo + hi) >> np.uint64(1)
        c = zone_crossed(mid.astype(np.float64) * 2.0 ** -53, b, m, md, z, tail, up)
        act = lo < hi
        hi = np.where(act & c, mid, hi)
        lo = np.where(act & ~c, mid + np.uint64(1), lo)
    bad = ~((m > 0.0) & np.isfinite(m) & np.isfinite(b) & (sg > 0.0) & np.isfinite(sg) &
            np.isfinite(mu_) & ~np.isnan(tail))
    thr_i = np.maximum.accumulate(np.where(bad, np.uint64(1 << 53), lo), axis=1)
    return thr_i if integer else thr_i.astype(np.float64) * 2.0 ** -53


def screen_gap(thr_k, u1):
    """The screen's class of draws u1 of one component (its thresholds): the
    gap number of a cold draw, -1 for one that is inverted."""
    c = (u1[:, None] >= thr_k[None, :]).sum(axis=1)
    return np.where(c % 2 == 1, c // 2, -1)


ONE53 = 1 << 53
FUSE_TAB = 32          # kFuseTab: the pick ladder's table


def u53_int(u):
    """U of a uniform u = U 2^-53 (u53's integer; exact)."""
    return (np.asarray(u, dtype=np.float64) * 2.0 ** 53).astype(np.uint64)


def pick_predicate(cdf, j, U):
    """The draw's own test of component j at U0 = U: cdf[j] <= fl(u0 cdf_last),
    u0 = U 2^-53 exact, one rounding in the product."""
    cdf = np.asarray(cdf, dtype=np.float64)
    u0 = np.asarray(U, dtype=np.uint64).astype(np.float64) * 2.0 ** -53
    with np.errstate(invalid='ignore'):
        return cdf[j] <= u0 * cdf[-1]


def pick_cdf_emul(cdf, U0):
    """pick_cdf: the first k with cdf[k] > t, capped at K - 1 (binary search)."""
    cdf = np.asarray(cdf, dtype=np.float64)
    t = np.asarray(U0, dtype=np.uint64).astype(np.float64) * 2.0 ** -53 * cdf[-1]
    lo = np.zeros(t.shape, dtype=np.int64)
    hi = np.full(t.shape, cdf.size - 1, dtype=np.int64)
    while (lo < hi).any():
        act = lo < hi
        mid = (lo + hi) >> 1
        le = cdf[mid] <= t
        lo = np.where(act & le, mid + 1, lo)
        hi = np.where(act & ~le, mid, hi)
    return lo


def pick_ladder_emul(cdf, U0, cap=FUSE_TAB):
    """pick_cdf_ladder<cap>, step for step."""
    cdf = np.asarray(cdf, dtype=np.float64)
    K = cdf.size
    t = np.asarray(U0, dtype=np.uint64).astype(np.float64) * 2.0 ** -53 * cdf[-1]
    pad = np.concatenate([cdf, np.zeros(cap - K)])
    lo = np.zeros(t.shape, dtype=np.int64)
    step = cap // 2
    while step > 0:
        j = lo + step
        ok = (j <= K - 1) & (pad[np.minimum(j, cap) - 1] <= t)
        lo = np.where(ok, j, lo)
        step >>= 1
    return lo


def pick_thresholds(cdf):
    """k_draw_zone's pick boundaries B[K] (uint64): for j < K - 1 the smallest
    U in [0, 2^53] with cdf[j] <= fl(U 2^-53 cdf_last), by the 53-step
    bisection on the float predicate; B[K - 1] = 2^53.  With a nondecreasing
    cdf the pick of U0 is #{j < K - 1 : U0 >= B[j]}."""
    cdf = np.asarray(cdf, dtype=np.float64)
    K = cdf.size
    B = np.full(K, ONE53, dtype=np.uint64)
    j = np.arange(K - 1)
    lo = np.zeros(K - 1, dtype=np.uint64)
    hi = np.full(K - 1, ONE53, dtype=np.uint64)
    for _ in range(54):
        act = lo < hi
        mid = (lo + hi) >> np.uint64(1)
        c = pick_predicate(cdf, j, mid)
        hi = np.where(act & c, mid, hi)
        lo = np.where(act & ~c, mid + np.uint64(1), lo)
    B[:K - 1] = lo
    return B


def guide_table(cdf, gbits):
    """k_draw_zone's guide over the 2^gbits buckets of the top bits of U0:
    dict with B (pick_thresholds), k_lo[b] = #{j : B[j] <= the bucket's first
    U0}, c[b] = the boundaries strictly inside the bucket, and valid: cdf
    finite, nondecreasing, cdf_last > 0 and no bucket with two distinct
    interior boundaries."""
    cdf = np.asarray(cdf, dtype=np.float64)
    B = pick_thresholds(cdf)
    bj = B[:-1]
    sh = np.uint64(53 - gbits)
    s0 = np.arange(1 << gbits, dtype=np.uint64) << sh
    s1 = s0 + (np.uint64(1) << sh)
    k_lo = (bj[None, :] <= s0[:, None]).sum(axis=1)
    inside = (bj[None, :] > s0[:, None]) & (bj[None, :] < s1[:, None])
    c = inside.sum(axis=1)
    two = np.zeros(s0.size, dtype=bool)
    for b in np.flatnonzero(c > 1):
        two[b] = np.unique(bj[inside[b]]).size > 1
    ok = bool(np.isfinite(cdf).all() and (np.diff(cdf) >= 0.0).all() and cdf[-1] > 0.0)
    return dict(B=B, k_lo=k_lo, c=c, gbits=gbits, valid=ok and not two.any(), two=two)


def guide_pick(g, U0):
    """The integer pick: k_lo + (U0 >= B[k_lo] ? c : 0) of U0's bucket."""
    U0 = np.asarray(U0, dtype=np.uint64)
    b = (U0 >> np.uint64(53 - g['gbits'])).astype(np.int64)
    kl = g['k_lo'][b]
    return kl + np.where(U0 >= g['B'][kl], g['c'][b], 0)


def draw_picks(w, mu, sigma, low, high, n, rs, integers=False):
    """n draws of the table sampler: (component, u1, value); integers: and
    (U0, U1), the 53-bit integers of the pick's and the inversion's uniforms."""
    pw, base, mass, mode = draw_table(w, mu, sigma, low, high)
    cdf = np.cumsum(pw)
    u0 = rs.random_sample(n)
    k = np.minimum(np.searchsorted(cdf, u0 * cdf[-1], side='right'), cdf.size - 1)
    u1 = np.floor(rs.random_sample(n) * 2.0 ** 53) * 2.0 ** -53
    mu, sigma = np.asarray(mu), np.asarray(sigma)
    x = draw_invert_emul(base[k], mass[k], mode[k], mu[k], sigma[k], low, high, u1)
    return (k, u1, x, u53_int(u0), u53_int(u1)) if integers else (k, u1, x)


def _block_bytes(x, lo, hi):
    scale = BUCKETS / (hi - lo) if hi > lo else 0.0
    return np.clip(((x - lo) * scale).astype(np.int64), 0, BUCKETS - 1)


def _block_layout(key, hit, n):
    """sorted_block_prune_body's layout from the bucket bytes and the hot
    flags: (counts, bases, keep per wave tile, live per bucket)."""
    cnt = np.bincount(key, minlength=BUCKETS)
    base = np.cumsum(cnt) - cnt
    full = cnt > 0
    t0, t1 = base // WAVE, np.where(full, (base + cnt - 1) // WAVE, base // WAVE)
    hotb = full & (np.bincount(key[hit], minlength=BUCKETS) > 0)
    keep = np.zeros((n + WAVE - 1) // WAVE, dtype=bool)
    for b in np.flatnonzero(hotb):
        keep[t0[b]:t1[b] + 1] = True
    ck = np.concatenate([[0], np.cumsum(keep)])
    live = full & (ck[np.minimum(t1 + 1, keep.size)] - ck[np.minimum(t0, keep.size)] > 0)
    return cnt, base, keep, live


def draw_zones(pilot, intervals, y_lo, y_hi, center, tiles, zone_max=6, tail=WAVE, halves=None):
    """k_draw_zone's value zones (zlo, zhi) from the pilot's sort block (draw
    order) and the hot intervals in y'; None: the slot is not screened.
    tail: the low tail ends at the tail-th smallest value of the first wave
    tile of the bucket-sorted pilot, the high tail starts at the tail-th
    largest of its last (128: the tiles' maximum and minimum).  halves: the
    widening in half tiles of 64 positions (the device's default rule);
    None: in `tiles` whole tiles."""
    key = _block_bytes(pilot, pilot.min(), pilot.max())
    t = pilot[np.argsort(key, kind='stable')].reshape(-1, WAVE)
    first, last = np.sort(t[0]), np.sort(t[-1])
    z = [(-np.inf, first[tail - 1]), (last[WAVE - tail], np.inf)]
    if halves is not None:
        t, tiles = t.reshape(-1, WAVE // 2), halves
    tmin, tmax = t.min(axis=1), t.max(axis=1)
    nt = tmin.size
    eps = np.finfo(np.float64).eps
    for l, h in intervals:
        a = -np.inf if l <= y_lo else (l + center) - 8.0 * eps * (abs(l) + abs(center))
        b = np.inf if h >= y_hi else (h + center) + 8.0 * eps * (abs(h) + abs(center))
        reach = np.flatnonzero(tmax >= a)
        tf = int(reach[0]) if reach.size else nt
        reach = np.flatnonzero(tmin <= b)
        tl = int(reach[-1]) if reach.size else -1
        za, zb = a, b
        if a != -np.inf:
            w = tf - tiles
            za = -np.inf if w < 0 else min(a, tmin[w]) if w < nt else a
        if b != np.inf:
            w = tl + tiles
            zb = np.inf if w >= nt else max(b, tmax[w]) if w >= 0 else b
        z.append((za, zb))
    z.sort(key=lambda p: p[0])
    out = [list(z[0])]
    for a, b in z[1:]:
        if a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    while len(out) > zone_max:
        g = int(np.argmin([out[i + 1][0] - out[i][1] for i in range(len(out) - 1)]))
        out[g][1] = out[g + 1][1]
        del out[g + 1]
    if len(out) < 2:
        return None
    return np.array([a for a, _ in out]), np.array([b for _, b in out])


def draw_screen(tb, ta, mix, low, high, center, k, u1, x, tiles=2, tie=TIE, cells=CELLS,
                integers=None, gbits=9, tail=WAVE, halves=None):
    """The screened draw on the draws (k, u1, x) of one launch (draw_picks),
    block by block behind the pilot's, beside the full computation on all
    elements: dict with `blocks`, `fallback` (blocks that would run the full
    body), `exact` (share of the screened blocks' elements inverted) and
    `mismatch`: the blocks that do not fall back and whose key range, kept
    mask, live buckets, their counts and bases, or the bucket bytes of the
    inverted elements differ from the full computation's (must be empty).
    integers = (U0, U1): the integer screen -- the component from the guide
    pick of U0 (k only draws x), the class from U1 against thrI; a slot whose
    guide is not valid is not screened (`valid` False, no blocks).
    tail, halves: draw_zones'.  `lists`: per screened block, the inverted
    elements of each of its eight waves (k_draw_sorted_screen_run's lists)."""
    w, mu, sigma = mix
    r = prefilter(tb, ta, x - center, tie, cells)
    y_lo = tb['y_lo']
    y_hi = y_lo + tb['width'] * tb['P']
    out = dict(blocks=0, fallback=0, exact=0.0, mismatch=[], lists={})
    zones = draw_zones(x[:SORT_BLOCK], r['intervals'], y_lo, y_hi, center, tiles, tail=tail,
                       halves=halves)
    if zones is None:
        return out
    zlo, zhi = zones
    pw, base, mass, mode = draw_table(w, mu, sigma, low, high)
    thr = zone_thresholds(zlo, zhi, base, mass, mode, np.asarray(mu), np.asarray(sigma),
                          integer=integers is not None)
    if integers is None:
        c = (u1[:, None] >= thr[k]).sum(axis=1)
    else:
        g = guide_table(np.cumsum(pw), gbits)
        out['valid'] = g['valid']
        if not g['valid']:
            return out
        ki = guide_pick(g, integers[0])
        out['pick_mismatch'] = int((ki != k).sum())
        c = (integers[1][:, None] >= thr[ki]).sum(axis=1)
    cold, gap = c % 2 == 1, c // 2
    yc = np.clip(x - center, y_lo, y_hi)
    hit = np.isnan(x)
    for lo_i, hi_i in r['intervals']:
        hit |= (yc >= lo_i) & (yc <= hi_i)
    nex = nscr = 0
    for b0 in range(SORT_BLOCK, x.size, SORT_BLOCK):
        s = slice(b0, b0 + SORT_BLOCK)
        xb, cb, gb, hb = x[s], cold[s], gap[s], hit[s]
        out['blocks'] += 1
        ex = ~cb
        if not ex.any() or xb[ex].min() > zhi[0] or xb[ex].max() < zlo[-1] or (hb & cb).any():
            out['fallback'] += 1       # (a hot cold element cannot happen: counted, never hidden)
            if (hb & cb).any():
                out['mismatch'].append((b0, 'hot element screened out'))
            continue
        lo, hi = xb[ex].min(), xb[ex].max()
        full = _block_layout(_block_bytes(xb, xb.min(), xb.max()), hb, xb.size)
        key = np.where(cb, _block_bytes(zhi[np.where(cb, gb, 0)], lo, hi), _block_bytes(xb, lo, hi))
        cnt, bas, keep, live = _block_layout(key, hb, xb.size)
        bad = False
        for g in np.unique(gb[cb]):
            p0, p1 = int(_block_bytes(zhi[g], lo, hi)), int(_block_bytes(zlo[g + 1], lo, hi))
            bad |= bool(live[p0:p1 + 1].any())
        if bad:
            out['fallback'] += 1
            continue
        nscr += xb.size
        nex += int(ex.sum())
        per = -(-xb.size // (8 * 64)) * 64     # (bucket_bases' rows of a wave)
        out['lists'][b0 // SORT_BLOCK] = [int(ex[v * per:(v + 1) * per].sum()) for v in range(8)]
        same = (lo == xb.min() and hi == xb.max() and (keep == full[2]).all() and
                (live == full[3]).all() and (cnt[live] == full[0][live]).all() and
                (bas[live] == full[1][live]).all() and
                (key[ex] == _block_bytes(xb, xb.min(), xb.max())[ex]).all())
        if not same:
            out['mismatch'].append((b0, 'layout'))
    out['exact'] = nex / max(1, nscr)
    return out


def report_drawscreen(losses, cols, specs, every=1, draws=1 << 18, only=None, tiles=2, tail=WAVE,
                      halves=None, **fit):
    """Per hp with two certified tables: blocks, fallback blocks and the share
    of inverted elements of the screened draw's emulation."""
    for i, (label, (dist, args)) in enumerate(specs.items()):
        if i % every or (only is not None and i not in only):
            continue
        cp = certified_pair(losses, cols, label, dist, args, **fit)
        if cp is None or dist != 'uniform':
            print('%-6s not screened' % label)
            continue
        tb, ta, mix, (low, high, center) = cp
        k, u1, x = draw_picks(*mix, low, high, draws, np.random.RandomState(1000 + i))
        r = draw_screen(tb, ta, mix, low, high, center, k, u1, x, tiles, tail=tail, halves=halves)
        print('%-6s blocks %4d fallback %4d inverted %.4f mismatches %d'
              % (label, r['blocks'], r['fallback'], r['exact'], len(r['mismatch'])))


def report_erfcinv():
    rows = invert_error()
    for lab, e, y in rows:
        print('erfcinv_fast %-40s max |x - x_ref| / sigma %.3e at y = %.6e' % (lab, e, y))
    worst = max(e for _, e, _ in rows[:2])
    print('screened range: max %.3e, 16 x = %.3e, SCREEN_MARGIN %.3e' % (worst, 16.0 * worst,
                                                                          SCREEN_MARGIN))
    return worst


def pacc_of(family, w, mu, sigma, low, high):
    """The truncation mass in a side's table constants: a GMM's p_accept
    (make_coef), 1 for an LGMM (its lpdf applies none)."""
    return float(O._truncation_mass(w, mu, sigma, low, high)) if family == 'gmm' else 1.0


# Named fit parameters (tpe_plan_fit's gamma, gamma_cap, prior_weight, lf) on
# the test shape (N = 6000), with the split and mixture sizes they give there:
# K_below = n_below + 1 picks the draw kernels (<= 32 the small LDS draw table,
# <= 2048 the large one, above it no sorted draw and no tables), a tiny K_below
# leaves a below table of one or two panels, prior_weight 0 a -inf coefficient
# on the widest component, and prior_weight / lf change every weight.
def _fit_set(gamma, gamma_cap, prior_weight, lf, n_below, n=6000):
    return dict(gamma=gamma, gamma_cap=gamma_cap, prior_weight=prior_weight, lf=lf,
                n_below=n_below, K_below=n_below + 1, K_above=n - n_below + 1)


FIT_KEYS = ('gamma', 'gamma_cap', 'prior_weight', 'lf')
FIT_SETS = {
    'default': _fit_set(0.25, 25, 1.0, 25, 20),
    'wide-below': _fit_set(1.0, 200, 1.0, 25, 78),
    'huge-below': _fit_set(16.0, 2000, 1.0, 25, 1240),
    'over-cap': _fit_set(32.0, 2500, 1.0, 25, 2479),
    'few-below': _fit_set(0.02, 25, 1.0, 25, 2),
    'prior-only': _fit_set(0.0, 25, 1.0, 25, 0),
    'pw-small': _fit_set(0.25, 25, 1e-3, 25, 20),
    'pw-big': _fit_set(0.25, 25, 50.0, 25, 20),
    'pw-zero': _fit_set(0.25, 25, 0.0, 25, 20),
    'lf-off': _fit_set(0.25, 25, 1.0, 0, 20),
    'lf-long': _fit_set(1.0, 200, 0.5, 3000, 78),
}


def fit_params(name):
    """The four fit parameters of a named set, as keyword arguments."""
    return {k: FIT_SETS[name][k] for k in FIT_KEYS}


def mixtures(losses, cols, label, dist, args, gamma=0.25, gamma_cap=25, prior_weight=1.0, lf=25):
    """Both sides' (w, mu, sigma) of one hp, and (low, high, centre)."""
    tids = np.arange(losses.size)
    with np.errstate(all='ignore'):    # (prior_weight 0 takes log(0))
        fk, pm, ps, low, high, q, tr = O.posterior_spec(dist, args, prior_weight)
        bo, ao = O.split_observations(tids, cols[label], tids, losses, gamma, gamma_cap,
                                      kind='stable')
        fit = [tuple(np.asarray(v) for v in O.parzen_fit(O.transform_obs(obs, tr, low), prior_weight,
                                                          pm, ps, lf=lf, kind='stable'))
               for obs in (bo, ao)]
    return fit, (low, high, pm)


def certified_pair(losses, cols, label, dist, args, gamma=0.25, gamma_cap=25, prior_weight=1.0,
                   lf=25):
    """(tb, ta, below mixture, (low, high, centre)) of an hp whose two tables
    are certified, else None."""
    fit, (low, high, pm) = mixtures(losses, cols, label, dist, args, gamma, gamma_cap, prior_weight,
                                    lf)
    fam = O.posterior_spec(dist, args, prior_weight)[0]
    with np.errstate(all='ignore'):
        tabs = [build(w, mu, sg, low, high, pm, pacc_of(fam, w, mu, sg, low, high))
                for w, mu, sg in fit]
    if any(t is None or not t['ok'].all() for t in tabs):
        return None
    return tabs[0], tabs[1], fit[0], (low, high, pm)


def low_edge_shape(n=6000):
    """A history whose EI maximum sits at `low`: the good trials cluster at the
    lower bound of a uniform(-5, 5) (config 4's hp 0 behaves like this)."""
    rs = np.random.RandomState(31)
    v = rs.uniform(-5, 5, n)
    losses = (v + 5.0) / 10.0 + 0.05 * rs.rand(n)
    return losses, {'e': v}, {'e': ('uniform', (-5.0, 5.0))}


def high_edge_shape(n=6000):
    """The mirror of low_edge_shape: the EI maximum sits at `high`."""
    rs = np.random.RandomState(31)
    v = rs.uniform(-5, 5, n)
    losses = (5.0 - v) / 10.0 + 0.05 * rs.rand(n)
    return losses, {'e': v}, {'e': ('uniform', (-5.0, 5.0))}


def band_shape(n=6000):
    """99 % of the trials in a band a quarter unit wide, the good ones at its
    low end: narrow components beside wide ones, the certified error closest
    to the bar of the named histories (above: 3.1e-9 against 3.7e-9; both
    tables stay certified -- with the mask drawn after v one panel does not)."""
    rs = np.random.RandomState(1)
    mask = rs.rand(n) < 0.01
    v = rs.uniform(-5, 5, n)
    w = np.where(mask, v, 0.25 + 0.25 * rs.rand(n))
    losses = np.abs(w - 0.3) + 0.01 * rs.rand(n)
    return losses, {'e': w}, {'e': ('uniform', (-5.0, 5.0))}


def ties_shape(n=6000):
    """Values rounded to the half unit and clipped to [-5, 4.5], random
    losses: a panel of the above table is not certified (no lattice)."""
    rs = np.random.RandomState(2)
    v = np.clip(np.round(rs.uniform(-5, 5, n) * 2.0) / 2.0, -5.0, 4.5)
    losses = rs.rand(n)
    return losses, {'e': v}, {'e': ('uniform', (-5.0, 5.0))}


def comb_shape(n=6000, gap=0.28, period=0.7, seed=3):
    """A comb: no trial in the first `gap` of every `period`, random losses.
    Both tables are certified and the score has a local maximum per tooth, so
    a wide tie window leaves more hot runs than HOT_IV."""
    rs = np.random.RandomState(seed)
    v = rs.uniform(-5, 5, 4 * n)
    v = v[np.mod(v + 5.0, period) > gap][:n]
    assert v.size == n
    losses = rs.rand(n)
    return losses, {'e': v}, {'e': ('uniform', (-5.0, 5.0))}


NAMED = {'low-edge': low_edge_shape, 'high-edge': high_edge_shape, 'band': band_shape,
         'ties': ties_shape, 'comb': comb_shape}


def report_prefilter(losses, cols, specs, every=1, draws=1 << 18, **fit):
    rs = np.random.RandomState(7)
    for i, (label, (dist, args)) in enumerate(specs.items()):
        if i % every:
            continue
        pair = certified_pair(losses, cols, label, dist, args, **fit)
        if pair is None:
            print('%-4s prefilter: no certified pair, every wave tile scored' % label)
            continue
        tb, ta, (w, mu, sg), (low, high, pm) = pair
        with np.errstate(all='ignore'):
            r = prefilter(tb, ta, draw_below(w, mu, sg, low, high, pm, draws, rs))
        missed = int((r['pruned'] & ~(r['wmax'] < r['thr'])).sum())
        print('%-4s prefilter: cells hot %d / %d (%.2f %%), intervals %d, wave tiles passing %d / %d '
              '(%.2f %%), hot wave tiles %d, missed %d'
              % (label, int(r['hot'].sum()), r['hot'].size, 100.0 * r['hot'].mean(),
                 len(r['intervals']), int((~r['pruned']).sum()), r['pruned'].size,
                 100.0 * (~r['pruned']).mean(), int((~(r['wmax'] < r['thr'])).sum()), missed))
        assert missed == 0, 'a hot wave tile was pruned'


def report_drawprune(losses, cols, specs, every=1, draws=1 << 18, only=None, **fit):
    rs = np.random.RandomState(7)
    out = {}
    for i, (label, (dist, args)) in enumerate(specs.items()):
        if (i % every) if only is None else (i not in only):
            continue
        pair = certified_pair(losses, cols, label, dist, args, **fit)
        if pair is None:
            print('%-4s drawprune: no certified pair, every wave tile written' % label)
            continue
        tb, ta, (w, mu, sg), (low, high, pm) = pair
        with np.errstate(all='ignore'):
            r = draw_prune(tb, ta, draw_below(w, mu, sg, low, high, pm, draws, rs))
        out[label] = r
        print('%-4s drawprune: wave tiles kept %d / %d (%.2f %%), exact filter passing %.2f %%, '
              'elements ranked %.2f %%, hot wave tiles dropped %d'
              % (label, int(r['kept'].sum()), r['kept'].size, 100.0 * r['kept'].mean(),
                 100.0 * (~r['pruned']).mean(), 100.0 * r['live'], r['dropped_hot']))
        assert r['dropped_hot'] == 0, 'a hot wave tile was dropped'
    return out


def report(label, side, w, mu, sigma, low, high, center, rs, pts=200):
    with np.errstate(all='ignore'):
        tab = build(w, mu, sigma, low, high, center)   # (pacc 1: a constant factor of g)
    if tab is None:
        print('%-4s %-5s K=%-5d no table (panel count out of range)' % (label, side, w.size))
        return None
    with np.errstate(all='ignore'):
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


def run(losses, cols, specs, every=1, gamma=0.25, gamma_cap=25, prior_weight=1.0, lf=25):
    rs = np.random.RandomState(5)
    tabs = {}
    for i, (label, (dist, args)) in enumerate(specs.items()):
        if i % every:
            continue
        fit, (low, high, pm) = mixtures(losses, cols, label, dist, args, gamma, gamma_cap,
                                        prior_weight, lf)
        for side, (w, mu, sg) in zip(('below', 'above'), fit):
            tabs[label, side] = report(label, side, w, mu, sg, low, high, pm, rs)
    return tabs


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument('--n', type=int, default=6000)
    ap.add_argument('--gap', default=None, help='LABEL:LO:HI')
    ap.add_argument('--cfg4', action='store_true', help="bench.py config 4's history")
    ap.add_argument('--every', type=int, default=1, help='every n-th hp')
    ap.add_argument('--prefilter', action='store_true', help='report the prefilter emulation')
    ap.add_argument('--drawprune', action='store_true', help='report the pruning-draw emulation')
    ap.add_argument('--only', default=None, help='--drawprune: comma-separated hp numbers')
    ap.add_argument('--low-edge', action='store_true', help='good trials clustered at low')
    ap.add_argument('--shape', choices=sorted(NAMED), help='another named history')
    ap.add_argument('--draws', type=int, default=1 << 18, help='--prefilter: draws per hp')
    ap.add_argument('--gamma', type=float, default=0.25)
    ap.add_argument('--gamma-cap', type=int, default=25)
    ap.add_argument('--prior-weight', type=float, default=1.0)
    ap.add_argument('--lf', type=int, default=25)
    ap.add_argument('--fit-set', choices=sorted(FIT_SETS), help='the fit parameters of a named set')
    ap.add_argument('--drawscreen', action='store_true', help='report the screened-draw emulation')
    ap.add_argument('--tiles', type=int, default=2, help='--drawscreen: zone widening in pilot tiles')
    ap.add_argument('--tail', type=int, default=WAVE,
                    help="--drawscreen: the tail zones' rank in the pilot's end tiles (1 .. 128)")
    ap.add_argument('--halves', type=int, default=None,
                    help='--drawscreen: zone widening in half tiles (instead of --tiles)')
    ap.add_argument('--erfcinv', action='store_true',
                    help="only report erfcinv_fast's emulated error (the screened draw's margin)")
    a = ap.parse_args()
    if a.erfcinv:
        report_erfcinv()
        return
    fit = fit_params(a.fit_set) if a.fit_set else dict(
        gamma=a.gamma, gamma_cap=a.gamma_cap, prior_weight=a.prior_weight, lf=a.lf)
    if a.cfg4:
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        import bench
        dom, losses, vals, act = bench.build_workload('cfg4')
        cols = {h.label: vals[h.index] for h in dom.space.hps}
        specs = {h.label: ('uniform', (-5.0, 5.0)) for h in dom.space.hps}
    elif a.low_edge or a.shape:
        losses, cols, specs = NAMED[a.shape or 'low-edge'](a.n)
    else:
        gap = None
        if a.gap:
            lab, lo, hi = a.gap.split(':')
            gap = (lab, float(lo), float(hi))
        losses, cols, specs = test_shape(a.n, gap)
    if a.drawscreen:
        only = None if a.only is None else {int(x) for x in a.only.split(',')}
        report_drawscreen(losses, cols, specs, a.every, a.draws, only, a.tiles, a.tail, a.halves,
                          **fit)
        return
    if not (a.drawprune and a.only):
        run(losses, cols, specs, a.every, **fit)
    if a.prefilter:
        report_prefilter(losses, cols, specs, a.every, a.draws, **fit)
    if a.drawprune:
        only = None if a.only is None else {int(x) for x in a.only.split(',')}
        report_drawprune(losses, cols, specs, a.every, a.draws, only, **fit)


if __name__ == '__main__':
    main()
