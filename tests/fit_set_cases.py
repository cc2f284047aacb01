"""One history and the named fit sets of the whole-configuration tests away
from the default fit (test_fit_sets_points_host.py for where the cases sit,
test_gpu_fit_sets_points.py on the device) -- TEST INFRASTRUCTURE ONLY: numpy,
the oracles and the package's host code; nothing here calls the engine.

History: N = 3000 prior trials (``rand.suggest``, HIST_SEED) of a 10-hp space
with seeded uniform losses -- past kMergeMax = 1024, so every fit is the large
tier of k_fit.  Unconditional: a uniform, a quniform (q = 1 over [0, 10]: 11
lattice values over 3000 rows), a lognormal, a qloguniform, a 5-way randint and
the two-way choice ``top``; under its branch 0 a normal and a quniform, under
branch 1 a loguniform and a 3-option pchoice.  Three groups: the six roots and
the two branches.

Fit sets: (gamma, gamma_cap, prior_weight, lf) by name; N_BELOW and COND_SIDES
give per set the split the oracle's n_below_count makes of it and what of it
the branches see, asserted below.

Configurations: M = 257 per set (the same for every set) -- 200 prior draws of
the space, then every lattice value of the two quantized roots, every option
of the randint and of the pchoice, both bounds of the bounded continuous hps,
the 8 history rows of lowest loss, and 14 history rows at the ends of the
quniform root's tie runs on the default split's above side (where a tie order
other than the row's shows).
"""
import functools

import numpy as np

import hyperopt_amd as H
from hyperopt_amd import hp, rand, tpe, Trials, trials_from_docs
from hyperopt_amd.base import Domain

from oracle import tpe_oracle as O
from oracle_algo import oracle_hps
import batch_oracle as B
import group_oracle as G
import joint_oracle as J

N, M, K_BATCH = 3000, 257, 8
N_PRIOR = 200
# (LOSS_SEED: the first from 62 on under which the default split's 14 below rows
# leave an option of the randint unseen -- unseen_randint_options)
HIST_SEED, LOSS_SEED, CONFIG_SEED = 61, 68, 63
TAB_CAP = 2048                  # kTabCap (draw_replay.TAB_CAP)
QU_LATTICE = np.arange(0.0, 11.0)
QLU_LATTICE = np.arange(2.0, 21.0, 2.0)      # rint(exp(u) / 2) 2 for u in (0, 3]
ROOTS = ('ln', 'qlu', 'qu', 'ri', 'top', 'u')
BRANCH = (('n0', 'q0'), ('lu1', 'pc1'))
BATCH_SETS = ('default', 'pw-small', 'pw-big', 'pw-zero', 'lf-short', 'lf-off', 'huge-below')


def space(hp_):
    return {'u': hp_.uniform('u', -2, 3), 'qu': hp_.quniform('qu', 0, 10, 1),
            'ln': hp_.lognormal('ln', 0, 1), 'qlu': hp_.qloguniform('qlu', 0, 3, 2),
            'ri': hp_.randint('ri', 5),
            'top': hp_.choice('top', [
                {'kind': 0, 'n0': hp_.normal('n0', 0, 2), 'q0': hp_.quniform('q0', -5, 5, 0.5)},
                {'kind': 1, 'lu1': hp_.loguniform('lu1', -3, 1),
                 'pc1': hp_.pchoice('pc1', [(.2, 'a'), (.5, 'b'), (.3, 'c')])}])}


# name -> (gamma, gamma_cap, prior_weight, lf)
FIT_SETS = {
    'default': (0.25, 25, 1.0, 25),
    'wide-below': (1.5, 200, 1.0, 25),
    'huge-below': (24.0, 1300, 1.0, 25),
    'over-cap': (48.0, 2100, 1.0, 25),
    'few-below': (0.02, 25, 1.0, 25),
    'prior-only': (0.0, 25, 1.0, 25),
    'pw-zero': (0.25, 25, 0.0, 25),
    'pw-small': (0.25, 25, 1e-3, 25),
    'pw-big': (0.25, 25, 50.0, 25),
    'lf-short': (1.5, 200, 0.5, 20),
    'lf-off': (1.5, 200, 0.5, 0),
}
NAMES = tuple(FIT_SETS)
# what a set is compared with to show that its parameter matters (the host
# test): the default fit, or the same split without the change
BASELINE = {name: FIT_SETS['default'] for name in NAMES}
BASELINE.update({'pw-small': (0.25, 25, 1.0, 25), 'pw-big': (0.25, 25, 1.0, 25),
                 'lf-short': (1.5, 200, 0.5, 25), 'lf-off': (1.5, 200, 0.5, 25)})
# root n_below per set
N_BELOW = {'default': 14, 'wide-below': 83, 'huge-below': 1300, 'over-cap': 2100, 'few-below': 2,
           'prior-only': 0, 'pw-zero': 14, 'pw-small': 14, 'pw-big': 14, 'lf-short': 83,
           'lf-off': 83}


def fit_kwargs(name):
    gamma, cap, pw, lf = FIT_SETS[name]
    return dict(gamma=gamma, gamma_cap=cap, prior_weight=pw, lf=lf)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def done(docs, losses):
    for d, l in zip(docs, losses):
        d['state'] = H.JOB_STATE_DONE
        d['result'] = {'status': 'ok', 'loss': float(l)}
    return trials_from_docs(docs)


def make_trials(n, hist_seed=HIST_SEED, loss_seed=LOSS_SEED):
    """(domain, trials) of n prior trials with seeded uniform losses."""
    dom = Domain(lambda x: 0.0, space(hp))
    docs = rand.suggest(list(range(n)), dom, Trials(), hist_seed)
    return dom, done(docs, np.random.RandomState(loss_seed).rand(n))


@functools.lru_cache(maxsize=None)
def history():
    """(domain, losses[N], vals[P, N], active[P, N]) of the history."""
    dom, trials = make_trials(N)
    _, losses, vals, active = tpe.build_history(dom, trials)
    assert losses.size == N and vals.shape == (10, N)
    assert tuple(dom.space.labels[i] for i in tpe.root_indices(dom.space)) == ROOTS
    return (dom,) + _frozen(losses, vals, active)


def labels():
    return history()[0].space.labels


@functools.lru_cache(maxsize=None)
def hp_list():
    """[(label, description)] in hp index order: the oracles' argument."""
    cs = history()[0].space
    h = oracle_hps(cs)
    return tuple((lab, h[lab]) for lab in cs.labels)


def _params(key):
    return FIT_SETS[key] if isinstance(key, str) else tuple(key)


@functools.lru_cache(maxsize=None)
def joint_model(key):
    """``joint_oracle.JointModel`` of a named set (or of a parameter tuple)."""
    gamma, cap, pw, lf = _params(key)
    _, losses, vals, _ = history()
    return J.JointModel(list(hp_list()), losses, vals, gamma, pw, lf, cap)


@functools.lru_cache(maxsize=None)
def group_model(key):
    gamma, cap, pw, lf = _params(key)
    _, losses, vals, active = history()
    return G.GroupModel(list(hp_list()), losses, vals, active, gamma, pw, lf, cap)


@functools.lru_cache(maxsize=None)
def below_mask(key):
    gamma, cap, _, _ = _params(key)
    mask = np.zeros(N, dtype=bool)
    mask[J.side_rows(history()[1], gamma, cap)[0]] = True
    return _frozen(mask)[0]


@functools.lru_cache(maxsize=None)
def side_sizes(key):
    """label -> (observations below, above) of a set: the hp's K is one more."""
    _, _, _, active = history()
    below = below_mask(key)
    return {lab: (int((active[i] == 1)[below].sum()), int((active[i] == 1)[~below].sum()))
            for i, lab in enumerate(labels())}


# ------------------------------------------------------- the marginal model
def marginal_fit(key, i):
    """(dist, [below, above], spec) of hp i under a set: per side the
    probabilities of a categorical hp (spec None), else the (w, mu, sigma) of
    its Parzen mixture (stable ties) and spec = (family, low, high, q) of
    ``posterior_spec``."""
    gamma, cap, pw, lf = _params(key)
    _, losses, vals, active = history()
    lab, h = hp_list()[i]
    on = active[i] == 1
    below = below_mask(key)
    obs = [vals[i][on & below], vals[i][on & ~below]]
    if h['dist'] in ('randint', 'categorical'):
        if h['dist'] == 'randint':
            upper, pp = int(h['args'][0]), None
        else:
            pp = np.asarray(h['args'][0], dtype=np.float64)
            upper = pp.size
        return h['dist'], [O.categorical_posterior(o, upper, pw, pp, lf) for o in obs], None
    fk, pm, ps, low, high, q, tr = O.posterior_spec(h['dist'], h['args'], pw)
    fits = [O.parzen_fit(O.transform_obs(o, tr, low), pw, pm, ps, lf=lf, kind='stable')
            for o in obs]
    return h['dist'], fits, (fk, low, high, q)


def marginal_lliks(key, cfg, cfg_active):
    """(llik_b, llik_a)[P, M] of the configurations' active values under the
    oracle's marginal fit of a set, NaN where inactive."""
    lb, la = np.full(cfg.shape, np.nan), np.full(cfg.shape, np.nan)
    for i in range(cfg.shape[0]):
        at = cfg_active[i] == 1
        if not at.any():
            continue
        dist, fits, spec = marginal_fit(key, i)
        with np.errstate(all='ignore'):
            for out, f in zip((lb, la), fits):
                if spec is None:
                    out[i, at] = O.categorical_lpdf(cfg[i][at], f)
                else:
                    fk, low, high, q = spec
                    lpdf = O.lgmm_lpdf if fk == 'lgmm' else O.gmm_lpdf
                    out[i, at] = lpdf(cfg[i][at], *f, low=low, high=high, q=q)
    return lb, la


def marginal_total(lb, la, cfg_active):
    with np.errstate(all='ignore'):
        return np.where(cfg_active == 1, lb - la, 0.0).sum(axis=0)


# -------------------------------------------------------- the configurations
def tie_run_rows():
    """14 history rows at the ends of the tie runs of ``qu`` on the default
    split's above side: the first and the last row of value 5 (the prior's
    mu, where the two ends get different sigmas), the first row of every
    other value and the last rows of values 0 and 10."""
    _, _, vals, _ = history()
    qu = vals[labels().index('qu')]
    above = ~below_mask('default')
    rows_of = lambda v: np.flatnonzero(above & (qu == v))
    out = [rows_of(5.0)[0], rows_of(5.0)[-1]]
    out += [rows_of(v)[0] for v in QU_LATTICE if v != 5.0]
    out += [rows_of(0.0)[-1], rows_of(10.0)[-1]]
    assert len(set(int(r) for r in out)) == 14
    return [int(r) for r in out]


@functools.lru_cache(maxsize=None)
def configs():
    """(vals[P, M] with NaN where inactive, active[P, M] uint8, what[M]): the
    configurations of every set and what each is ('prior', 'qu=3', ...)."""
    dom, losses, hv, ha = history()
    cs = dom.space
    lab = cs.labels.index
    docs = rand.suggest(list(range(M)), dom, Trials(), CONFIG_SEED)
    cfgs = [{l: v[0] for l, v in d['misc']['vals'].items() if v} for d in docs]
    vals = np.array(tpe.config_columns(cs, cfgs)[0])
    what = ['prior'] * N_PRIOR
    # the crafted ones start from the prior draws behind the first 200, of the
    # branch they need
    spare = {b: [j for j in range(N_PRIOR, M) if vals[lab('top'), j] == b] for b in (0, 1)}
    spare[None] = list(range(N_PRIOR, M))
    cols, turn = [], {0: 0, 1: 0, None: 0}

    def craft(name, value, branch=None):
        pool = spare[branch]
        c = vals[:, pool[turn[branch] % len(pool)]].copy()
        turn[branch] += 1
        c[lab(name)] = value
        cols.append(c)
        what.append('%s=%g' % (name, value))

    for v in QU_LATTICE:
        craft('qu', v)
    for v in QLU_LATTICE:
        craft('qlu', v)
    for v in range(5):
        craft('ri', float(v))
    for v in range(3):
        craft('pc1', float(v), 1)
    craft('u', -2.0), craft('u', 3.0)
    craft('q0', -5.0, 0), craft('q0', 5.0, 0)
    craft('lu1', float(np.exp(-3.0)), 1), craft('lu1', float(np.exp(1.0)), 1)
    hist = np.where(ha == 1, hv, np.nan)
    for r in np.argsort(losses, kind='stable')[:8]:
        cols.append(hist[:, r])
        what.append('best row %d' % r)
    for r in tie_run_rows():
        cols.append(hist[:, r])
        what.append('tie-run row %d' % r)
    assert N_PRIOR + len(cols) == M == len(what), len(cols)
    vals[:, N_PRIOR:] = np.array(cols).T
    active = tpe.active_columns(cs, vals)
    np.testing.assert_array_equal(active, ~np.isnan(vals))
    return _frozen(vals, active.astype(np.uint8)) + (tuple(what),)


def unseen_randint_options(key='pw-zero'):
    """(options no below row holds, options both sides hold) of ``ri``."""
    _, _, vals, _ = history()
    ri = vals[labels().index('ri')]
    below = below_mask(key)
    b, a = set(ri[below].astype(int)), set(ri[~below].astype(int))
    return sorted(set(range(5)) - b), sorted(b & a)


def klass(x):
    """0 finite, -1 / +1 the infinities, 2 NaN."""
    x = np.asarray(x, dtype=np.float64)
    return np.where(np.isnan(x), 2, np.where(np.isinf(x), np.sign(x), 0)).astype(int)


@functools.lru_cache(maxsize=None)
def batch_run(name):
    """The oracle's pending batch of K_BATCH over the configurations."""
    _, _, pw, lf = FIT_SETS[name]
    return B.run(group_model(name), np.ascontiguousarray(configs()[0]), K_BATCH, prior_weight=pw,
                 lf=lf)


# ------------------------------------------------- what the sets must reach
# observations (below, above) of the conditional hps per set: K is one more
COND_SIDES = {
    'default': ((5, 1461), (9, 1525)), 'wide-below': ((38, 1428), (45, 1489)),
    'huge-below': ((634, 832), (666, 868)), 'over-cap': ((1032, 434), (1068, 466)),
    'few-below': ((1, 1465), (1, 1533)), 'prior-only': ((0, 1466), (0, 1534)),
}
for _name, _like in (('pw-zero', 'default'), ('pw-small', 'default'), ('pw-big', 'default'),
                     ('lf-short', 'wide-below'), ('lf-off', 'wide-below')):
    COND_SIDES[_name] = COND_SIDES[_like]


def _assert_split():
    for name, (gamma, cap, pw, lf) in FIT_SETS.items():
        assert O.n_below_count(N, gamma, cap) == N_BELOW[name], name
    kb = {name: nb + 1 for name, nb in N_BELOW.items()}
    assert kb['default'] <= 32
    assert 65 <= kb['wide-below'] <= 256 and 65 <= kb['lf-short'] <= 256
    assert 1025 <= kb['huge-below'] <= TAB_CAP < kb['over-cap']
    assert N_BELOW['few-below'] == 2 and N_BELOW['prior-only'] == 0
    assert FIT_SETS['pw-zero'][2] == 0.0 and FIT_SETS['prior-only'][2] != 0.0
    assert FIT_SETS['pw-small'][2] == 1e-3 and FIT_SETS['pw-big'][2] == 50.0
    assert 0 < FIT_SETS['lf-short'][3] < N_BELOW['lf-short'] and FIT_SETS['lf-off'][3] == 0
    assert FIT_SETS['lf-off'][:3] == FIT_SETS['lf-short'][:3]
    assert N > 1024          # kMergeMax: the large tier of k_fit


_assert_split()


def assert_sets_reach():
    """The sizes on the history itself: the roots' and every conditional hp's
    observations per side, and what the table of the sets asks of them."""
    for name in NAMES:
        ss = side_sizes(name)
        nb = N_BELOW[name]
        assert all(ss[lab] == (nb, N - nb) for lab in ROOTS), name
        for labs, want in zip(BRANCH, COND_SIDES[name]):
            assert all(ss[lab] == want for lab in labs), (name, labs)
    cond = [lab for labs in BRANCH for lab in labs]
    assert all(side_sizes('huge-below')[lab][0] + 1 > 256 for lab in cond)
    over = side_sizes('over-cap')
    assert all(over[lab][0] + 1 <= TAB_CAP and over[lab][1] + 1 >= 2 for lab in cond)
    assert over['u'][1] + 1 >= 2
    # the below ramp of lf-short is on in every group
    assert all(side_sizes('lf-short')[lab][0] > FIT_SETS['lf-short'][3] for lab in cond)
    unseen, both = unseen_randint_options('pw-zero')
    assert unseen == [2] and both == [0, 1, 3, 4]
