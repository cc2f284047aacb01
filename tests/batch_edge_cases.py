"""The fixtures of the pending batch's edge tests, shared by the host test
(which proves that each of them can tell a wrong rule from the right one) and
the GPU test (which then runs them on the device) -- TEST INFRASTRUCTURE ONLY.

One-hp histories: the space is ``{'x': <kind>}``, so the one group has one
dimension and the pending kernel is the whole score change.  Per kind there are
histories of 1, 2, 40 and 140 rows; the picks are crafted onto the edges of
``pending_record``'s sigma search (continuous kinds), walk the whole lattice
(quantized kinds) or take every option (categorical kinds), and an audience of
further configurations is scored every round and never picked.

``two_branch`` is the small case of the per-group bookkeeping, ``many_dists``
(tests/golden) one 11-hp group holding all eleven kinds; ``slot_case`` and
``kmax_case`` are the launch shapes past one pass of the pick kernel's slot
loop and at BATCH_MAX.

``replay`` restates the rounds of ``batch_oracle.run`` with every rule of the
update as a switch (``Rules``), from given sides if wanted: the host test's
mutants and the GPU test's tight check of the update arithmetic."""
import copy
import functools
import math

import numpy as np

from hyperopt_amd import hp, rand, tpe, Trials
from hyperopt_amd.base import Domain

from golden_io import load, load_json
from oracle import tpe_oracle as O
from oracle_algo import oracle_hps
import batch_cases as C
import batch_oracle as B
import group_oracle as G
import joint_oracle as J
import spaces

GAMMA, PRIOR_WEIGHT = C.GAMMA, C.PRIOR_WEIGHT
HIST_SEED, LOSS_SEED = 5, 6
SIZES = (1, 2, 40, 140)
MAX_LATTICE = 24

KINDS = {
    'uniform': lambda h: h.uniform('x', -5, 5),
    'loguniform': lambda h: h.loguniform('x', math.log(1e-3), math.log(10)),
    'quniform': lambda h: h.quniform('x', 0, 10, 3),
    'qloguniform': lambda h: h.qloguniform('x', 0, 3, 2),
    'normal': lambda h: h.normal('x', 4, 7),
    'lognormal': lambda h: h.lognormal('x', -2, 2),
    'qnormal': lambda h: h.qnormal('x', 0, 10, 2),
    'qlognormal': lambda h: h.qlognormal('x', 0, 2, 1),
    'randint': lambda h: h.randint('x', 10),
    'pchoice': lambda h: h.pchoice('x', [(.1, 0), (.6, 1), (.3, 2)]),
}
CONTINUOUS = ('uniform', 'loguniform', 'normal', 'lognormal')
QUANTIZED = ('quniform', 'qloguniform', 'qnormal', 'qlognormal')
CATEGORICAL = ('randint', 'pchoice')
LOG_KINDS = ('loguniform', 'qloguniform', 'lognormal', 'qlognormal')
EXACT_MU = ('uniform', 'normal')        # mu = x: the kinds of the tight replay

TWO_BRANCH_ROWS, TWO_BRANCH_AUDIENCE = 60, 40
# the seed of two_branch's prior-drawn configurations: chosen so that the
# oracle's six picks alternate branches (test_batch_edges_host.py)
TWO_BRANCH_SEED = 38
MANY_M, MANY_K = 257, 8
# the seed of many_dists' prior-drawn configurations: chosen so that every
# round is decided (test_batch_edges_host.test_every_many_dists_round_is_decided)
CONFIG_SEED = {'many_dists': 31}


def _space(name):
    if name == 'two_branch':
        return hp.choice('t', [{'u': hp.uniform('u', -1, 1)}, {'v': hp.normal('v', 0, 1)}])
    if name == 'many_dists':
        return spaces.many_dists_space(hp)
    return {'x': KINDS[name](hp)}


# ------------------------------------------------------------- the histories
@functools.lru_cache(maxsize=None)
def history(name, n=None):
    """(domain, losses, vals, active): ``n`` rows drawn from the prior with
    seed 5 and losses from RandomState(6); many_dists from tests/golden."""
    dom = Domain(lambda x: 0.0, _space(name))
    if name == 'many_dists':
        meta = load_json('suggest_meta.json')[name]
        d = load('suggest_%s.npz' % name)
        assert list(meta['labels']) == dom.space.labels
        out = dom, d['losses'], d['vals'], d['active']
    else:
        n = TWO_BRANCH_ROWS if name == 'two_branch' else n
        docs = rand.suggest(list(range(n)), dom, Trials(), HIST_SEED)
        trials = C.done(docs, np.random.RandomState(LOSS_SEED).rand(n))
        out = (dom,) + tuple(tpe.build_history(dom, trials)[1:])
    for a in out[1:]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def model(name, n=None):
    dom, losses, vals, active = history(name, n)
    h = oracle_hps(dom.space)
    return G.GroupModel([(lab, h[lab]) for lab in dom.space.labels], losses, vals, active,
                        GAMMA, PRIOR_WEIGHT)


def spec(kind):
    """``posterior_spec`` of a continuous or quantized kind."""
    h = model(kind, SIZES[0]).dims[0][1][0].h
    return O.posterior_spec(h['dist'], h['args'], PRIOR_WEIGHT)


def transform(kind, raw):
    """Raw values in the transformed space of the hp's fit."""
    _, _, _, low, _, _, tr = spec(kind)
    with np.errstate(all='ignore'):
        return O.transform_obs(np.asarray(raw, dtype=np.float64), tr, low)


def above_mus(kind, n):
    """The hp's sorted above mixture, the prior in it."""
    return model(kind, n).dims[0][1][0].marginal[1]


# ------------------------------------------------------------------ the picks
def _raw_of(kind, n, mu):
    """A raw value whose transform is ``mu``: the observation itself where
    ``mu`` is a fitted one (so that a tie is a tie bit for bit)."""
    if kind not in LOG_KINDS:
        return float(mu)
    d = model(kind, n).dims[0][1][0]
    hit = np.flatnonzero(d.obs == mu)
    if hit.size:
        rows = model(kind, n).rows[0][1]
        return float(history(kind, n)[2][0][rows[hit[0]]])
    return float(np.exp(mu))


def _continuous_picks(kind, n):
    mus = above_mus(kind, n)
    K, ps = mus.size, spec(kind)[2]
    out = [mus[0] - 0.3 * ps, mus[-1] + 0.3 * ps, mus[0] - 3 * ps, mus[-1] + 3 * ps]
    if K > 2:
        gaps = np.diff(mus)
        wide = int(np.argmax(gaps))
        narrow = int(np.argmin(np.where(gaps > 0, gaps, np.inf)))
        out += [0.5 * (mus[wide] + mus[wide + 1]), 0.5 * (mus[narrow] + mus[narrow + 1]),
                mus[narrow], mus[K // 2]]
    return [_raw_of(kind, n, mu) for mu in out]


def _thin(values, keep, cap):
    """At most ``cap`` of ascending values: both ends and those in ``keep``,
    the others evenly spread."""
    values = np.asarray(values, dtype=np.float64)
    if values.size <= cap:
        return list(values)
    must = np.flatnonzero(np.isin(values, keep) | (np.arange(values.size) % (values.size - 1) == 0))
    rest = np.setdiff1d(np.arange(values.size), must)
    rest = rest[np.round(np.linspace(0, rest.size - 1, cap - must.size)).astype(np.int64)]
    return list(values[np.union1d(must, rest)])


def _quantized_picks(kind, n):
    """The lattice from the lowest to the highest value the space can produce
    (a log kind's from 0), thinned to MAX_LATTICE picks with the ends of the
    above mixture kept.  An unbounded kind: from two steps below to two steps
    above the observed extremes, and the lattice values next to 1.2 prior_sigma
    outside the above mixture -- only there does the upper clip act on it."""
    _, _, ps, low, high, q, _ = spec(kind)
    lg = kind in LOG_KINDS
    mus = above_mus(kind, n)
    ends = np.exp(mus[[0, -1]]) if lg else mus[[0, -1]]
    far = []
    if low is not None:
        a, b = (np.exp(low), np.exp(high)) if lg else (low, high)
        lo, hi = np.round(a / q) * q, np.round(b / q) * q
    else:
        seen = history(kind, n)[2][0]
        lo, hi = seen.min() - 2 * q, seen.max() + 2 * q
        out = np.array([mus[0] - 1.2 * ps, mus[-1] + 1.2 * ps])
        far = [v for v in np.round((np.exp(out) if lg else out) / q) * q if v < lo or v > hi]
    if lg:
        lo = 0.0
    lattice = lo + q * np.arange(int(round((hi - lo) / q)) + 1)
    return sorted(_thin(lattice, np.round(ends / q) * q, MAX_LATTICE - len(far)) + far)


def picks(kind, n):
    """The crafted picks of a one-hp fixture, raw values."""
    if kind in CONTINUOUS:
        return _continuous_picks(kind, n)
    if kind in QUANTIZED:
        return _quantized_picks(kind, n)
    return [float(o) for o in range(model(kind, n).dims[0][1][0].pi.size)]


def _beside(kind, p, q):
    """Values whose upper, or lower, bound lies prior_sigma / 100 beside each
    pick in the transformed space: a sigma at the floor is many times smaller
    than q / 2 and shows in cdf(ub) - cdf(lb) only there."""
    d = spec(kind)[2] / 100.0
    if kind in LOG_KINDS:
        return [p * np.exp(d) - q / 2.0, p * np.exp(-d) + q / 2.0]
    return [p + d - q / 2.0, p - d + q / 2.0]


class Case(object):
    """vals[P, M], eligible[M] and k of one batch call under ``model``."""

    def __init__(self, name, model, vals, eligible, k):
        vals = np.ascontiguousarray(vals, dtype=np.float64)
        vals.setflags(write=False)
        eligible.setflags(write=False)
        self.name, self.model, self.vals, self.eligible, self.k = name, model, vals, eligible, k


@functools.lru_cache(maxsize=None)
def case(kind, n):
    """The picks (eligible), then the audience: the picks again, values next
    to them, and two values the kind rejects."""
    p = np.array(picks(kind, n))
    if kind in CATEGORICAL:
        aud = [p, [2.5, float(p.size)]]
    else:
        q = spec(kind)[5]
        aud = [p, p * (1 + 1e-3) + 1e-3]
        if q is not None:
            aud += [p - q, p + q] + _beside(kind, p, q)
        if kind in LOG_KINDS:
            aud.append([-3.0 * (q or 1.0), -7.5])
    x = np.concatenate([p] + [np.asarray(a, dtype=np.float64) for a in aud])
    eligible = np.arange(x.size) < p.size
    return Case('%s n=%d' % (kind, n), model(kind, n), x[None, :], eligible, int(p.size))


def prior_configs(name, m, seed):
    """vals[P, m]: prior draws of the fixture's space, NaN where inactive."""
    dom = history(name)[0]
    docs = rand.suggest(list(range(m)), dom, Trials(), seed)
    cfgs = [{lab: v[0] for lab, v in d['misc']['vals'].items() if v} for d in docs]
    return tpe.config_columns(dom.space, cfgs)[0]


@functools.lru_cache(maxsize=None)
def two_branch_case(seed=TWO_BRANCH_SEED):
    """Three configurations of either branch, alternating, are eligible; 40
    more prior draws are the audience."""
    vals = prior_configs('two_branch', 6 * TWO_BRANCH_AUDIENCE, seed)
    t = vals[history('two_branch')[0].space.labels.index('t')]
    b0, b1 = np.flatnonzero(t == 0)[:3], np.flatnonzero(t == 1)[:3]
    first = np.stack([b0, b1], axis=1).ravel()
    rest = np.setdiff1d(np.arange(vals.shape[1]), first)[:TWO_BRANCH_AUDIENCE]
    vals = vals[:, np.concatenate([first, rest])]
    return Case('two_branch', model('two_branch'), vals, np.arange(vals.shape[1]) < 6, 6)


@functools.lru_cache(maxsize=None)
def many_dists_case(seed=None):
    vals = prior_configs('many_dists', MANY_M, CONFIG_SEED['many_dists'] if seed is None else seed)
    return Case('many_dists', model('many_dists'), vals, np.ones(MANY_M, dtype=bool), MANY_K)


@functools.lru_cache(maxsize=None)
def oracle_run(case_):
    """The oracle's batch of a case."""
    return B.run(case_.model, case_.vals, case_.k, eligible=case_.eligible,
                 prior_weight=PRIOR_WEIGHT)


# ------------------------------------------------------------------ the rules
class Rules(object):
    """The rules of the pending update, one switch each; the defaults are the
    model's, a mutant changes one."""
    side = 'right'              # an equal mu_k is a left neighbour
    lower_clip = True           # sigma >= prior_sigma / min(divisor_cap, divisor_add + K)
    upper_clip = True           # sigma <= prior_sigma
    divisor_add = 2.0
    divisor_cap = 100.0
    alone = 0.5                 # the prior alone: sigma = alone * prior_sigma
    pick_neighbours = False     # earlier picks are neighbours in the sigma search
    count_ng = True             # W = S + prior_weight + n_g
    update_inactive = False     # a group inactive in the pick keeps its Ja
    cat_swap = False            # categorical: hit and miss entries swapped
    clip_q_bounds = True        # quantized: ub, lb clipped at high, low
    log_jacobian = True         # log kinds: the - log x of the density

    def __init__(self, **kw):
        for key, v in kw.items():
            assert hasattr(Rules, key), key
            setattr(self, key, v)


MUTANTS = {
    'searchsorted left': dict(side='left'),
    'no lower clip': dict(lower_clip=False),
    'no upper clip': dict(upper_clip=False),
    'divisor min(100, 1 + K)': dict(divisor_add=1.0),
    'no cap at 100': dict(divisor_cap=np.inf),
    'prior alone gives prior_sigma': dict(alone=1.0),
    'picks are neighbours': dict(pick_neighbours=True),
    'W without n_g': dict(count_ng=False),
    'inactive group updated': dict(update_inactive=True),
    'categorical hit and miss swapped': dict(cat_swap=True),
    'quantized bounds not clipped': dict(clip_q_bounds=False),
    'no - log x': dict(log_jacobian=False),
}
SIGMA_MUTANTS = tuple(MUTANTS)[:7]


def rule_sigma(mus, mu, prior_sigma, rules=Rules()):
    """``batch_oracle.pending_sigma_closed`` under ``rules``."""
    mus = np.asarray(mus, dtype=np.float64)
    K = mus.size
    if K == 1:
        return rules.alone * prior_sigma
    lo = int(np.searchsorted(mus, mu, side=rules.side))
    gaps = ([mu - mus[lo - 1]] if lo > 0 else []) + ([mus[lo] - mu] if lo < K else [])
    s = max(gaps)
    if rules.lower_clip:
        s = max(s, prior_sigma / min(rules.divisor_cap, rules.divisor_add + K))
    return min(s, prior_sigma) if rules.upper_clip else s


def sigma_class(mus, mu, prior_sigma):
    """The edges of the sigma search a pick at ``mu`` sits on, as a set of
    'lo=0', 'lo=K', 'tie', 'floor 2+K', 'floor 100', 'ceiling', 'K=1'."""
    mus = np.asarray(mus, dtype=np.float64)
    K = mus.size
    if K == 1:
        return {'K=1'}
    lo = int(np.searchsorted(mus, mu, side='right'))
    out = set()
    if lo == 0:
        out.add('lo=0')
    if lo == K:
        out.add('lo=K')
    if (mus == mu).any():
        out.add('tie')
    gaps = ([mu - mus[lo - 1]] if lo > 0 else []) + ([mus[lo] - mu] if lo < K else [])
    if max(gaps) < prior_sigma / min(100.0, 2.0 + K):
        out.add('floor 2+K' if 2.0 + K < 100.0 else 'floor 100')
    if max(gaps) > prior_sigma:
        out.add('ceiling')
    return out


def _pending_kernel(d, value, mus, rules, prior_weight):
    """(x -> log kappa(x; the pick), mu) of the above-side dim ``d`` for a
    pick's raw ``value``; ``mus`` the sorted mixture the sigma is searched in."""
    p = copy.copy(d)
    if d.cat:
        o = int(value)
        p.kappa = J.kappa([o], d.a, d.pi)[1:2]
        if rules.cat_swap:
            hit, miss = (1 + d.a * d.pi) / (1 + d.a), d.a * d.pi / (1 + d.a)
            p.kappa = np.where(np.arange(d.pi.size) == o, miss, hit)[None, :]
        return (lambda x: p.log_kernel(x)[:, 0]), None
    _, _, ps, low, _, _, tr = O.posterior_spec(d.h['dist'], d.h['args'], prior_weight)
    mu = float(O.transform_obs(np.array([value], dtype=np.float64), tr, low)[0])
    p.mu, p.sigma = np.array([mu]), np.array([rule_sigma(mus, mu, ps, rules)])
    if not rules.clip_q_bounds:
        p.low = p.high = None
    if not rules.log_jacobian and d.fk == 'lgmm' and d.q is None:
        return (lambda x: p.log_kernel(x)[:, 0] + np.log(x)), mu
    return (lambda x: p.log_kernel(x)[:, 0]), mu


class Replay(object):
    """scores[k, M]; per round t the state the scores were formed from:
    ja[k, G, M], and lk[k, G, M] / W[k, G], the kernel and the mass of the
    update that led to it (0 where there was none)."""

    def __init__(self, scores, ja, lk, W):
        self.scores, self.ja, self.lk, self.W = scores, ja, lk, W


def replay(model, vals, picks_, rules=Rules(), sides=None, mus=None,
           prior_weight=PRIOR_WEIGHT):
    """The rounds of ``batch_oracle.run(forced=picks_)`` in float64 numpy under
    ``rules``, the sigma from the closed form.  ``sides``: (J_below[G, M],
    J_above[G, M]) to start from instead of the oracle's; ``mus``: {hp index:
    sorted above mixture} instead of the oracle's."""
    vals = np.asarray(vals, dtype=np.float64)
    on = model.active(vals)
    jb, ja = B.sides(model, vals) if sides is None else (np.array(sides[0]), np.array(sides[1]))
    n_g = [0] * len(model.groups)
    last = [None] * len(model.groups)       # the group's last record
    extra = {}                              # hp index -> the earlier picks' mus
    lk_t, W_t = np.zeros(on.shape), np.zeros(len(model.groups))
    scores, jas, lks, Ws = [], [], [], []
    for p in picks_:
        p = int(p)
        with np.errstate(all='ignore'):
            scores.append(G.ordered_sum(np.where(on, jb - ja, 0.0)))
        jas.append(ja.copy())
        lks.append(lk_t)
        Ws.append(W_t)
        lk_t, W_t = np.zeros(on.shape), np.zeros(len(model.groups))
        for g, hp_ids in enumerate(model.groups):
            if on[g][p]:
                kernels = []
                for i, d in zip(hp_ids, model.dims[g][1]):
                    base = None if d.cat else (d.marginal[1] if mus is None else mus[i])
                    if rules.pick_neighbours and not d.cat:
                        base = np.sort(np.concatenate([base, extra.get(i, [])]))
                    f, mu = _pending_kernel(d, vals[i][p], base, rules, prior_weight)
                    kernels.append((i, f))
                    if mu is not None:
                        extra[i] = list(extra.get(i, [])) + [mu]
                last[g] = kernels
            elif not (rules.update_inactive and last[g] is not None):
                continue
            c = on[g]
            lk = np.zeros(int(c.sum()))
            with np.errstate(all='ignore'):
                for i, f in last[g]:
                    lk = lk + f(vals[i][c])
                W = model.S[g][1] + prior_weight + (n_g[g] if rules.count_ng else 0)
                ja[g][c] = np.logaddexp(ja[g][c] + np.log(W), lk) - np.log(W + 1.0)
            lk_t[g][c], W_t[g] = lk, W
            n_g[g] += 1
    return Replay(np.array(scores), np.array(jas), np.array(lks), np.array(Ws))


def tight_allowance(jb, rep, g=0):
    """[k, M]: 64 eps (t + 1) (|J_b| + |Ja_t| + |lk| + log(W + 1) + 1) on round
    t's scores of a one-group replay from the device's own sides.  A round has
    fewer than 8 rounded operations, each at most 2 ulp of a quantity inside
    the bracket, logaddexp does not amplify, and 4 is margin."""
    t = np.arange(rep.scores.shape[0])[:, None]
    return 64 * np.finfo(np.float64).eps * (t + 1) * (
        np.abs(jb)[None, :] + np.abs(rep.ja[:, g]) + np.abs(rep.lk[:, g]) +
        np.log(rep.W[:, g] + 1.0)[:, None] + 1.0)


# ----------------------------------------------------- the launch-shape cases
SHAPE_KIND, SHAPE_N = 'uniform', 40
BLOCK = 256                                 # kBtThreads: configurations per block of a round
SLOT_M, SLOT_K = 65536 + 300, 4             # 258 blocks: k_batch_pick's slot loop takes two passes
SLOT_BEST = 257 * BLOCK + 16
KMAX_M = 1100


@functools.lru_cache(maxsize=None)
def slot_case():
    """m = 65836 uniform draws of the one-hp ``uniform`` space; two
    configurations of block 0 and five each of blocks 256 and 257 are
    eligible, and the best of them -- the grid point of [-5, 5] that scores
    highest -- lies in block 257."""
    mdl = model(SHAPE_KIND, SHAPE_N)
    x = np.random.RandomState(8).uniform(-5, 5, SLOT_M)
    grid = np.linspace(-5, 5, 4001)
    x[SLOT_BEST] = grid[int(np.argmax(mdl.total(grid[None, :])))]
    eligible = np.zeros(SLOT_M, dtype=bool)
    eligible[[3, 200] + [256 * BLOCK + 50 * i for i in range(5)] +
             [257 * BLOCK + 8 * i for i in range(5)]] = True
    assert eligible[SLOT_BEST] and eligible.sum() == 12
    return Case('slots', mdl, x[None, :], eligible, SLOT_K)


@functools.lru_cache(maxsize=None)
def kmax_case(k):
    """1100 distinct values of the same space, all eligible."""
    x = np.random.RandomState(9).permutation(np.linspace(-5, 5, KMAX_M))
    return Case('kmax', model(SHAPE_KIND, SHAPE_N), x[None, :], np.ones(KMAX_M, dtype=bool), k)
