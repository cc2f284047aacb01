"""Host side of multivariate TPE (no GPU): the joint model's anchor to the
reference -- a space with one unconditional hp gives the marginal lpdf
difference again --, the interaction it exists for, the ABI additions, and
the ``multivariate=`` plumbing of the four entry points over a stub plan."""
import os
import re

import numpy as np
import pytest

import hyperopt_amd as H
from hyperopt_amd import hp, rand, tpe, Trials, trials_from_docs
from hyperopt_amd import _engine as E
from hyperopt_amd.base import Domain

from oracle import tpe_oracle as O
import joint_oracle as J
import spaces

GAMMA, PRIOR_WEIGHT = 0.25, 1.0

# the eleven kinds, with many_dists' arguments
KINDS = {
    'uniform': ('uniform', (4, 7)), 'quniform': ('quniform', (0, 10, 3)),
    'loguniform': ('loguniform', (-2, 0)), 'qloguniform': ('qloguniform', (0, 3, 2)),
    'normal': ('normal', (4, 7)), 'qnormal': ('qnormal', (0, 10, 2)),
    'lognormal': ('lognormal', (-2, 2)), 'qlognormal': ('qlognormal', (0, 2, 1)),
    'randint': ('randint', (10,)), 'choice': ('randint', (3,)),
    'pchoice': ('categorical', ([.1, .9],)),
}
EXACT = ('normal', 'qnormal', 'lognormal', 'qlognormal', 'loguniform', 'randint', 'choice',
         'pchoice')
UP_TO_A_CONSTANT = ('uniform', 'quniform', 'qloguniform')


def _one_hp_case(kind, n, seed=0):
    dist, args = KINDS[kind]
    rng = np.random.RandomState(1000 * n + seed)
    vals = O.prior_sample(rng, dist, args, n).astype(np.float64)[None, :]
    losses = rng.uniform(size=n)
    cand = O.prior_sample(rng, dist, args, 64).astype(np.float64)
    return dict(dist=dist, args=args, conds=()), losses, vals, cand


def _marginal(h, losses, vals, cand):
    tids = np.arange(losses.size)
    bo, ao = O.split_observations(tids, vals[0], tids, losses, GAMMA, kind='stable')
    with np.errstate(all='ignore'):
        r = O.score_hp(h['dist'], h['args'], bo, ao, PRIOR_WEIGHT, cand, kind='stable')
    return r['llik_b'] - r['llik_a']


@pytest.mark.parametrize('n', [1, 2, 9, 60, 300])
@pytest.mark.parametrize('kind', sorted(KINDS))
def test_one_root_hp_gives_the_marginal_lpdf(kind, n):
    """Unbounded, log-continuous and categorical kinds: exactly score_hp's
    llik_b - llik_a; bounded kinds: up to one constant per fit (the two
    truncation masses the joint model leaves out)."""
    h, losses, vals, cand = _one_hp_case(kind, n)
    m = J.JointModel([('x', h)], losses, vals, GAMMA, PRIOR_WEIGHT)
    diff = m.joint(cand[None, :]) - _marginal(h, losses, vals, cand)
    assert np.isfinite(diff).all()
    print('%s n=%d: max |diff| %.3g, spread %.3g' % (kind, n, np.abs(diff).max(), np.ptp(diff)))
    if kind in EXACT:
        assert np.abs(diff).max() <= 1e-12
    else:
        assert kind in UP_TO_A_CONSTANT
        assert np.ptp(diff) <= 1e-12


@pytest.mark.parametrize('n', [1, 2, 9, 60, 300])
@pytest.mark.parametrize('kind', ['randint', 'pchoice'])
def test_categorical_smoothing_is_the_posterior(kind, n):
    """sum_k w_k kappa_k(c) == categorical_posterior, the property that fixes a."""
    h, losses, vals, _ = _one_hp_case(kind, n)
    m = J.JointModel([('x', h)], losses, vals, GAMMA, PRIOR_WEIGHT)
    pp = None if h['dist'] == 'randint' else np.asarray(h['args'][0])
    for s in range(2):
        d = m.dims[s][0]
        want = O.categorical_posterior(vals[0][m.rows[s]], d.pi.size, PRIOR_WEIGHT, pp)
        np.testing.assert_allclose(m.w[s] @ d.kappa, want, rtol=0, atol=1e-14)


def test_components_are_the_marginal_mixture():
    h, losses, vals, _ = _one_hp_case('quniform', 60)      # (ties: stable ranks)
    m = J.JointModel([('x', h)], losses, vals, GAMMA, PRIOR_WEIGHT)
    for s in range(2):
        d = m.dims[s][0]
        assert sorted(d.place.tolist()) == list(range(d.place.size))
        rows = np.concatenate([[-1], m.rows[s]])
        order = np.lexsort((rows, d.mu))
        for got, want in zip((d.w, d.mu, d.sigma), d.marginal):
            np.testing.assert_array_equal(got[order], want)
        np.testing.assert_allclose(m.w[s][1:], d.w[1:], rtol=1e-15)


def checkerboard():
    """32 trials on x, y ~ uniform(-1, 1): the two best at (0.8, 0.8) and
    (-0.8, -0.8), the 30 bad ones on the anti-diagonal, those nearest the
    centre first (the linear-forgetting ramp then down-weights four trials
    whose kernels do not reach +-0.8)."""
    t = np.linspace(-0.9, 0.9, 30)
    t = t[np.argsort(np.abs(t), kind='stable')]
    x = np.concatenate([[0.8, -0.8], t])
    y = np.concatenate([[0.8, -0.8], -t])
    losses = np.concatenate([[0.0, 0.1], 1.0 + np.arange(30) / 30.0])
    hps = [(l, dict(dist='uniform', args=(-1, 1), conds=())) for l in ('x', 'y')]
    return hps, losses, np.stack([x, y])


def test_checkerboard_interaction_is_visible_to_the_joint_model_only():
    hps, losses, vals = checkerboard()
    cfg = np.array([[0.8, 0.8], [0.8, -0.8]])       # columns: on / off the good diagonal
    m = J.JointModel(hps, losses, vals, GAMMA, PRIOR_WEIGHT)
    assert [r.tolist() for r in m.rows][0] == [0, 1]
    joint = m.joint(cfg)
    marg = sum(_marginal(h, losses, vals[i:i + 1], cfg[i]) for i, (_, h) in enumerate(hps))
    print('joint on / off %s, marginal on / off %s' % (joint, marg))
    assert joint[0] - joint[1] > 1
    assert abs(marg[0] - marg[1]) < 1e-3


def test_abi_additions():
    names = ('tpe_plan_joint_fit', 'tpe_plan_joint_get_mixture', 'tpe_plan_joint_score_points',
             'tpe_plan_joint_sample_points')
    hdr = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include',
                       'tpe_engine.h')
    declared = set(re.findall(r'\b(tpe_[a-z_]+)\s*\(', open(hdr).read()))
    for nm in names:
        assert nm in declared and nm in E.EXPORTS
    for meth in ('joint_fit', 'joint_mixture', 'joint_score_points', 'joint_score_points_device',
                 'joint_sample_points', 'joint_sample_points_device'):
        assert callable(getattr(E.Plan, meth))
    if os.path.exists(E.LIB_PATH):
        lib = E.load_library()
        for nm in names:
            assert getattr(lib, nm).argtypes is not None


class StubPlan(object):
    """Records which calls the entry points make."""

    def __init__(self, P):
        self.P, self.calls, self.engine = P, [], None

    def update_history(self, *a, **k):
        pass

    def fit(self, **k):
        self.calls.append('fit')

    def joint_fit(self):
        self.calls.append('joint_fit')

    def score_points(self, vals, want_terms=False, want_active=False):
        self.calls.append('score_points')
        m = vals.shape[1]
        out = (np.arange(m, dtype=float),) + ((np.ones((self.P, m)),) if want_terms else ()) + \
            ((tpe.active_columns(self.cs, vals).astype(np.uint8),) if want_active else ())
        return out[0] if len(out) == 1 else out

    def joint_score_points(self, vals, want_terms=False, want_active=False, want_joint=False):
        self.calls.append('joint_score_points')
        m = vals.shape[1]
        out = (-np.arange(m, dtype=float),) + ((np.zeros((self.P, m)),) if want_terms else ()) + \
            ((tpe.active_columns(self.cs, vals).astype(np.uint8),) if want_active else ()) + \
            ((np.full(m, 7.0),) if want_joint else ())
        return out[0] if len(out) == 1 else out

    def sample_points(self, seed, m, begin=0):
        self.calls.append(('sample_points', seed, m, begin))
        return np.zeros((self.P, m)), np.zeros(m)

    def joint_sample_points(self, seed, m, begin=0):
        self.calls.append(('joint_sample_points', seed, m, begin))
        return np.ones((self.P, m)), np.ones(m)


def _history(dom, n, seed=3):
    docs = rand.suggest(list(range(n)), dom, Trials(), seed)
    for i, doc in enumerate(docs):
        doc['state'] = H.JOB_STATE_DONE
        doc['result'] = {'status': 'ok', 'loss': float(i)}
    return trials_from_docs(docs)


@pytest.fixture
def stub(monkeypatch):
    dom = Domain(lambda x: 0.0, spaces.cond_space(hp))
    plan = StubPlan(len(dom.space.labels))
    plan.cs = dom.space
    monkeypatch.setattr(tpe._State, 'plan_for', lambda self, domain, n, engine: plan)
    monkeypatch.setattr(E, 'default_engine', lambda *a: None)
    return dom, plan, _history(dom, 6)


def test_multivariate_argument_reaches_the_joint_calls(stub):
    dom, plan, trials = stub
    cs = dom.space
    assert [cs.labels[i] for i in tpe.root_indices(cs)] == ['aa', 'top']
    pool = np.where(trials_vals(cs, trials)[1] == 1, trials_vals(cs, trials)[0], np.nan)
    dicts = tpe.columns_to_configs(cs, pool, ~np.isnan(pool))   # (a dict pool is scored from the host)
    # default: the marginal calls, and no joint fit
    tpe.score_configs(pool, dom, trials)
    tpe.sample_configs(5, dom, trials, 1)
    tpe.suggest_from_pool([10], dom, trials, 1, pool=dicts, n_startup_jobs=0,
                          skip_seen=False)
    assert [c if isinstance(c, str) else c[0] for c in plan.calls] == [
        'fit', 'score_points', 'fit', 'sample_points', 'fit', 'score_points']
    del plan.calls[:]
    ei, terms, active, joint = tpe.score_configs(pool, dom, trials, return_terms=True,
                                                 multivariate=True)
    assert plan.calls == ['fit', 'joint_fit', 'joint_score_points']
    assert (joint == 7.0).all() and (terms['aa'] == 0.0).all() and (terms['top'] == 0.0).all()
    assert sorted(terms) == cs.labels and active['top'].all()
    assert np.array_equal(tpe.score_configs(pool, dom, trials, multivariate=True), ei)
    del plan.calls[:]
    vals, total = tpe.sample_configs(5, dom, trials, 1, begin=9, multivariate=True)
    assert plan.calls == ['fit', 'joint_fit', ('joint_sample_points', tpe.batch_seeds(1, 1)[0], 5, 9)]
    assert (vals == 1.0).all() and (total == 1.0).all()
    del plan.calls[:]
    docs = tpe.suggest_from_pool([10], dom, trials, 1, pool=dicts, n_startup_jobs=0,
                                 skip_seen=False, multivariate=True)
    assert plan.calls == ['fit', 'joint_fit', 'joint_score_points']
    # the stub's joint totals fall with the index, its marginal ones rise
    got = {lab: v[0] for lab, v in docs[0]['misc']['vals'].items() if v}
    assert got == tpe.columns_to_configs(cs, pool[:, :1], ~np.isnan(pool[:, :1]))[0]


def trials_vals(cs, trials):
    _, _, vals, active = tpe.build_history(Domain(lambda x: 0.0, spaces.cond_space(hp)), trials)
    return vals, active


def test_multivariate_needs_every_root_value(stub):
    dom, plan, trials = stub
    st = tpe._state(dom)
    with st.lock:
        hist = st.history(dom, trials).sync(trials)
    i = dom.space.labels.index('aa')
    hist.active[i, 2] = 0
    try:
        with pytest.raises(ValueError, match="row 2 .*'aa'"):
            tpe._fit_for(st, dom, trials, hist, None, PRIOR_WEIGHT, GAMMA, multivariate=True)
        tpe._fit_for(st, dom, trials, hist, None, PRIOR_WEIGHT, GAMMA)     # (marginal: fine)
    finally:
        hist.active[i, 2] = 1


def test_suggest_joint_startup_ignores_multivariate():
    dom = Domain(lambda x: 0.0, spaces.cond_space(hp))
    a = tpe.suggest_joint([0, 1], dom, Trials(), 5, multivariate=True)
    b = tpe.suggest_joint([0, 1], dom, Trials(), 5)
    assert [d['misc']['vals'] for d in a] == [d['misc']['vals'] for d in b]
