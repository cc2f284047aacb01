"""Annealing search on the MI355X engine -- ``anneal.suggest`` drop-in
(hyperopt/anneal.py:43-417).

One suggestion walks the hyperparameters in the reference interpreter's order
(``CompiledSpace.draw_order``: reverse-sorted labels, condition parents
first).  An active hyperparameter with T observations (history rows in which
it is active; pending and failed rows, loss +inf, count) takes an *anchor*
row: the first row of the suggestion's anchor list ``best`` that has it
active, else a fresh one -- rank ``clip(g - 1, 0, T - 1)``, g geometric with
mean ``avg_best_idx``, among its rows in ascending (loss, row) order, appended
to ``best`` -- and draws its value from its prior narrowed around the
anchor's value by ``shrink = 1 / (1 + T * shrink_coef)``.  T = 0 draws from
the prior.  Equal losses are ordered by row (the reference's numpy argsort is
unstable there; DESIGN section 3, "Tie hazard").

``rng_stream='philox'`` (default): the device path.  The columnar history is
pushed as ``tpe.suggest`` pushes it and one ``tpe_plan_anneal`` call serves
every id of ``new_ids`` (suggestion s keyed by ``tpe.batch_seeds(seed, S)[s]``,
each with its own anchor list).  There is no CPU fallback on this path.

``rng_stream='numpy'``: the reference's ``RandomState(seed + new_id)`` stream
replayed on the host (``rng.geometric`` and the pyll samplers with the
shifted parameters), one id per call like the reference: its suggestions value
for value.

The pure pieces -- ``shrink``, ``loss_order``, ``reuse_anchor``,
``choose_anchor``, ``rank_from_uniform``, ``value_params`` and
``value_from_uniforms`` -- are the host statement of what the kernels compute.
"""
from __future__ import annotations

import math

import numpy as np

from . import rstream

_default_avg_best_idx = 2.0
_default_shrink_coef = 0.1

BOUNDED = ('uniform', 'quniform', 'loguniform', 'qloguniform')
NORMAL = ('normal', 'qnormal', 'lognormal', 'qlognormal')
CATEGORICAL = ('randint', 'categorical')


# --------------------------------------------------------------------------
# pure pieces
# --------------------------------------------------------------------------
def shrink(T, shrink_coef):
    """Fraction of the prior width left after T observations (anneal.py:140-149)."""
    return 1.0 / (1.0 + T * shrink_coef)


def loss_order(losses):
    """History rows in ascending (loss, row) order."""
    return np.argsort(np.asarray(losses, dtype=np.float64) + 0.0, kind='stable')


def reuse_anchor(best, active_col):
    """The first row of the anchor list in which the hp is active, else None
    (anneal.py:158-169)."""
    for row in best:
        if active_col[row]:
            return int(row)
    return None


def choose_anchor(order, active_col, rank):
    """The rank-th row, in loss order, among the rows with the hp active
    (anneal.py:171-178 with a stable sort)."""
    order = np.asarray(order)
    rows = order[np.asarray(active_col)[order] != 0]
    return int(rows[rank])


def rank_from_uniform(u, avg_best_idx, T):
    """Clipped rank of a fresh anchor from a uniform u in [0, 1): geometric(p =
    1 / avg_best_idx) on {1, 2, ...} by inversion, g = ceil(log1p(-u) /
    log1p(-p)) (g = 1 when p >= 1), rank = clip(g - 1, 0, T - 1)."""
    p = 1.0 / avg_best_idx
    g = 1.0 if p >= 1.0 else math.ceil(math.log1p(-u) / math.log1p(-p))
    return int(min(max(g - 1.0, 0.0), float(T - 1)))


def value_params(dist, args, v, shr):
    """The shifted sampler parameters of one hp around the anchor value ``v``
    (anneal.py:232-408): ('uniform', low, high) for the bounded kinds (log
    space for the log kinds), ('normal', mu, sigma) for the normal kinds,
    ('p', p[upper]) for randint / categorical.  ``v`` None: the prior's."""
    if dist in BOUNDED:
        low, high = float(args[0]), float(args[1])
        if v is None:
            return ('uniform', low, high)
        mid = np.log(v) if 'log' in dist else v
        width = (high - low) * shr
        half = .5 * width
        mid = float(np.clip(mid, low + half, high - half))
        return ('uniform', mid - half, mid + half)
    if dist in NORMAL:
        mu, sigma = float(args[0]), float(args[1])
        if v is None:
            return ('normal', mu, sigma)
        if dist == 'lognormal':
            mu = float(np.log(v))
        elif dist == 'qlognormal':
            mu = float(np.log(1e-16 + v))     # anneal.py:391-393
        else:
            mu = float(v)
        return ('normal', mu, sigma * shr)
    if dist in CATEGORICAL:
        if dist == 'randint':
            upper = int(args[0])
            prior = 1.0 / upper
        else:
            prior = np.asarray(args[0], dtype=np.float64)
            upper = len(prior)
        if v is None:
            return ('p', np.zeros(upper) + prior)
        counts = np.bincount([int(v)], minlength=upper) / 1.0
        return ('p', (1 - shr) * counts + shr * prior)
    raise ValueError('unknown distribution %r' % dist)


def _quantize(dist, args, x):
    if dist in ('loguniform', 'qloguniform', 'lognormal', 'qlognormal'):
        x = np.exp(x)
    if dist.startswith('q'):
        q = float(args[2])
        x = np.round(x / q) * q
    return float(x)


def value_from_uniforms(dist, args, params, u, prior=False):
    """The device's value of one hp from its value uniforms ``u`` (one for the
    bounded and categorical kinds, two for the normal kinds; tpe_engine.h,
    tpe_plan_anneal) and ``value_params``: fp64, one rounding per operation."""
    kind = params[0]
    if kind == 'uniform':
        a, b = params[1], params[2]
        x = a + (b - a) * u[0]
        if not x < b:
            x = np.nextafter(b, -np.inf)
        return _quantize(dist, args, x)
    if kind == 'normal':
        z = math.sqrt(-2.0 * math.log(1.0 - u[0])) * math.cos(2.0 * math.pi * u[1])
        return _quantize(dist, args, params[1] + params[2] * z)
    p = params[1]
    if prior and dist == 'randint':
        return float(min(math.floor(u[0] * len(p)), len(p) - 1))
    tot = 0.0
    for c in range(len(p)):
        tot += float(p[c])
    t, acc = u[0] * tot, 0.0
    for c in range(len(p) - 1):
        acc += float(p[c])
        if t < acc:
            return float(c)
    return float(len(p) - 1)


# --------------------------------------------------------------------------
# suggest
# --------------------------------------------------------------------------
def _check(avg_best_idx, shrink_coef):
    if not (math.isfinite(avg_best_idx) and math.isfinite(shrink_coef) and
            avg_best_idx >= 1 and shrink_coef >= 0):
        raise ValueError('anneal: avg_best_idx >= 1 and shrink_coef >= 0, finite')


def suggest(new_ids, domain, trials, seed, avg_best_idx=_default_avg_best_idx,
            shrink_coef=_default_shrink_coef, rng_stream='philox', engine=None):
    """hyperopt/anneal.py:411-413, one document per id in ``new_ids``."""
    new_ids = list(new_ids)
    if rng_stream == 'numpy':
        new_id, = new_ids               # the reference accepts exactly one
        return _suggest_numpy(new_id, domain, trials, seed, avg_best_idx, shrink_coef)
    if rng_stream != 'philox':
        raise ValueError('rng_stream must be "philox" or "numpy"')
    if not new_ids:
        return []
    _check(avg_best_idx, shrink_coef)
    from . import tpe
    cs = domain.space
    st = tpe._state(domain)
    with st.lock:
        hist = st.history(domain, trials).sync(trials)
        plan = st.plan_for(domain, hist.n, engine or tpe.E.default_engine())
        hist.push(plan)
        if plan.anneal_order is None:
            plan.set_anneal_order([cs.by_label[lab].index for lab in cs.draw_order])
        res = plan.anneal(tpe.batch_seeds(seed, len(new_ids)), avg_best_idx, shrink_coef)
    picks = tpe._picks(cs, res)
    return [tpe._new_doc(domain, trials, cs, i, c) for i, c in zip(new_ids, picks)]


def suggest_batch(new_ids, domain, trials, seed, avg_best_idx=_default_avg_best_idx,
                  shrink_coef=_default_shrink_coef, rng_stream='philox', engine=None):
    """hyperopt/anneal.py:416-417: (idxs, vals) of all ids, per label."""
    new_ids = list(new_ids)
    cs = domain.space
    idxs, vals = {lab: [] for lab in cs.labels}, {lab: [] for lab in cs.labels}
    if rng_stream == 'numpy':
        docs = [suggest([i], domain, trials, seed, avg_best_idx, shrink_coef, 'numpy')[0]
                for i in new_ids]
    else:
        docs = suggest(new_ids, domain, trials, seed, avg_best_idx, shrink_coef, rng_stream,
                       engine)
    for doc in docs:
        for lab in cs.labels:
            idxs[lab].extend(doc['misc']['idxs'][lab])
            vals[lab].extend(doc['misc']['vals'][lab])
    return idxs, vals


def _draw_numpy(rng, h, params):
    """One pyll sampler call (hyperopt/pyll/stochastic.py:30-142, size 1)."""
    if params[0] == 'uniform':
        x = rng.uniform(params[1], params[2], size=1)[0]
    elif params[0] == 'normal':
        x = rng.normal(params[1], params[2], size=1)[0]
    else:
        return int(rstream.multinomial_draw(rng, params[1], 1)[0])
    return _quantize(h.dist, h.args, x)


def _suggest_numpy(new_id, domain, trials, seed, avg_best_idx, shrink_coef):
    """The reference's annealer on the host: RandomState(seed + new_id)
    (algobase.py:236-237), its draw calls in its order."""
    from . import tpe
    from .history import TrialHistory
    _check(avg_best_idx, shrink_coef)
    cs = domain.space
    _, losses, vals, active = TrialHistory(domain).sync(trials).columns()
    rng = np.random.RandomState(seed + new_id)
    order = loss_order(losses)
    best, chosen = [], {}
    for lab in cs.draw_order:
        if not cs.is_active(lab, chosen):
            continue
        h = cs.by_label[lab]
        col = active[h.index]
        T = int(np.count_nonzero(col))
        if T == 0:
            v = rstream.prior_draw(rng, h.dist, h.args, 1)[0]
            chosen[lab] = int(v) if h.is_categorical else float(v)
            continue
        row = reuse_anchor(best, col)
        if row is None:
            g = rng.geometric(1.0 / avg_best_idx, size=1) - 1
            row = choose_anchor(order, col, int(np.clip(g, 0, T - 1)[0]))
            best.append(row)
        v0 = vals[h.index, row]
        chosen[lab] = _draw_numpy(rng, h, value_params(h.dist, h.args, v0, shrink(T, shrink_coef)))
    return [tpe._new_doc(domain, trials, cs, new_id, chosen)]
