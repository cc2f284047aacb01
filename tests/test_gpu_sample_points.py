"""Whole configurations drawn from the fitted model on the GPU
(tpe_plan_sample_points, tpe_plan_topk_points, tpe_plan_gather_points,
tpe.sample_configs, tpe.suggest_joint).

Every comparison here is exact.  A drawn value must be the bits tpe_sample
returns for the hp's below mixture with the same Philox key, stream and
offset; activity is the host's tpe.active_columns of the drawn values; scores
are tpe_plan_score_points' of the drawn array; the device's top-k is
tpe.rank_pool's order; suggest_joint's picks are the host rule's
(test_sample_host restates it) over tpe.sample_configs' output."""
import functools

import numpy as np
import pytest

import hyperopt_amd as H
from hyperopt_amd import fmin, hp, tpe, rand, Trials, trials_from_docs
from hyperopt_amd import _engine as E
from hyperopt_amd.base import Domain

from golden_io import load, load_json
import spaces
from test_sample_host import _restate

pytestmark = pytest.mark.gpu

GAMMA, PRIOR_WEIGHT = 0.25, 1.0
BLOCK = 256     # configurations per block of k_sample_points: 257 is the first m past it
SIZES = [1, 63, 64, 65, BLOCK + 1, 1000]


def nested_space(hp):
    # a choice inside a choice
    inner = hp.choice('b', [{'k': 0, 'y': hp.normal('y', 0, 1)},
                            {'k': 1, 'z': hp.quniform('z', 0, 10, 1)}])
    return {'a': hp.choice('a', [{'k': 0, 'x': hp.uniform('x', 0, 1)}, {'k': 1, 'inner': inner}]),
            'w': hp.loguniform('w', -3, 0)}


def cat300_space(hp):
    # more options than k_sample's 256 threads: the table's scan takes two
    # components per thread
    return {'c': hp.choice('c', list(range(300))), 'u': hp.uniform('u', -1, 1)}


def six_space(hp):
    # all-categorical: 6 distinct configurations
    return {'p': hp.choice('p', [0, 1]), 'q': hp.choice('q', [0, 1, 2])}


FIXTURES = {'many_dists': spaces.many_dists_space, 'cond': spaces.cond_space,
            'cfg3_small': spaces.cfg3_space}
SHAPES = {'many_dists': (11, 60), 'cond': (14, 120), 'cfg3_small': (50, 300)}
SMALL = {'nested': (nested_space, 40, 31), 'cat300': (cat300_space, 40, 32)}
NAMES = sorted(FIXTURES) + sorted(SMALL)
# (seed, begin) per space; the seeds give every conditional hp an active and an
# inactive configuration among 1000 (checked below)
DRAW = {'many_dists': (7, 0), 'cond': (8, 5), 'cfg3_small': (9, (1 << 32) + 3), 'nested': (10, 0),
        'cat300': (11, 17)}


def _done(docs, seed):
    for d, l in zip(docs, np.random.RandomState(seed).rand(len(docs))):
        d['state'] = H.JOB_STATE_DONE
        d['result'] = {'status': 'ok', 'loss': float(l)}
    return trials_from_docs(docs)


def _rand_trials(dom, n, seed):
    return _done(rand.suggest(list(range(n)), dom, Trials(), seed), seed + 100)


@functools.lru_cache(maxsize=None)
def _history(name):
    """(domain, losses, vals, active) of a space's history."""
    if name in FIXTURES:
        meta = load_json('suggest_meta.json')[name]
        d = load('suggest_%s.npz' % name)
        dom = Domain(lambda x: 0.0, FIXTURES[name](hp))
        assert list(meta['labels']) == dom.space.labels and d['vals'].shape == SHAPES[name]
        return dom, d['losses'], d['vals'], d['active']
    make, n, seed = SMALL[name]
    dom = Domain(lambda x: 0.0, make(hp))
    _, losses, vals, active = tpe.build_history(dom, _rand_trials(dom, n, seed))
    assert losses.size == n
    return dom, losses, vals, active


def _new_plan(name):
    dom, losses, vals, active = _history(name)
    hps, conds, pprior = dom.space.engine_tables()
    plan = E.Plan(E.default_engine(), hps, conds, pprior, max_trials=losses.size)
    plan.set_history(losses, vals, active)
    plan.fit(gamma=GAMMA, prior_weight=PRIOR_WEIGHT)
    return plan


_plan = functools.lru_cache(maxsize=None)(_new_plan)


def _fixture_trials(name):
    """A fresh domain and the Trials whose history is the fixture's."""
    meta = load_json('suggest_meta.json')[name]
    d = load('suggest_%s.npz' % name)
    dom = Domain(lambda x: 0.0, FIXTURES[name](hp))
    docs = rand.suggest(list(range(meta['n'])), dom, Trials(), meta['hist_seed'])
    for doc, l in zip(docs, d['losses']):
        doc['state'] = H.JOB_STATE_DONE
        doc['result'] = {'status': 'ok', 'loss': float(l)}
    return dom, trials_from_docs(docs)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b, msg=''):
    np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=msg)


def _reference_draws(name, seed, begin, m):
    """tpe_sample's draws of every hp's below mixture: [P, m]."""
    dom, _, _, _ = _history(name)
    plan = _plan(name)
    eng = plan.engine
    out = np.empty((plan.n_hp, m))
    for i, t in enumerate(dom.space.engine_tables()[0]):
        w, mu, sg = plan.mixture(i, 0)
        cat = t.family == E.CAT
        out[i] = eng.sample(t.family, w, None if cat else mu, None if cat else sg,
                            t.low if t.flags & E.HAS_LOW else None,
                            t.high if t.flags & E.HAS_HIGH else None,
                            t.q if t.flags & E.HAS_Q else None,
                            seed=seed, stream=i, offset=begin, n=m)
    return out


def _device_call(plan, seed, begin, m, ld):
    """sample_points_device into sentinel-filled buffers of row length ld."""
    eng = plan.engine
    P = plan.n_hp
    v = E.DeviceBuffer(eng, 8 * P * ld).upload(np.full((P, ld), -7.0))
    tot = E.DeviceBuffer(eng, 8 * ld).upload(np.full(ld, -7.0))
    trm = E.DeviceBuffer(eng, 8 * P * ld).upload(np.full((P, ld), -7.0))
    act = E.DeviceBuffer(eng, P * ld).upload(np.full((P, ld), 9, dtype=np.uint8))
    plan.sample_points_device(seed, begin, m, ld, v.ptr, tot.ptr, trm.ptr, act.ptr)
    return (v.download(np.empty((P, ld))), tot.download(np.empty(ld)),
            trm.download(np.empty((P, ld))), act.download(np.empty((P, ld), dtype=np.uint8)))


@pytest.mark.parametrize('m', SIZES)
@pytest.mark.parametrize('name', NAMES)
def test_values_activity_and_scores(name, m):
    dom, _, _, _ = _history(name)
    cs = dom.space
    plan = _plan(name)
    seed, begin = DRAW[name]
    ld = m + 9
    vals, total, terms, active = _device_call(plan, seed, begin, m, ld)
    # nothing past m is written
    assert (vals[:, m:] == -7.0).all() and (total[m:] == -7.0).all()
    assert (terms[:, m:] == -7.0).all() and (active[:, m:] == 9).all()
    vals, total, terms, active = vals[:, :m], total[:m], terms[:, :m], active[:, :m]
    # 1. values: tpe_sample's bits where active, NaN elsewhere
    assert set(np.unique(active)) <= {0, 1}
    on = active == 1
    ref = _reference_draws(name, seed, begin, m)
    _same(vals[on], ref[on], name)
    assert np.isnan(vals[~on]).all() and not np.isnan(vals[on]).any()
    # 2. activity is what the drawn values imply; inactive terms are +0.0
    np.testing.assert_array_equal(on, tpe.active_columns(cs, vals))
    assert (_bits(terms)[~on] == 0).all()
    # 3. the scores are score_points' of the drawn array
    want = plan.score_points(np.ascontiguousarray(vals), want_terms=True, want_active=True)
    _same(total, want[0], name)
    _same(terms, want[1], name)
    np.testing.assert_array_equal(active, want[2])
    assert np.isfinite(total).all()
    # the host entry point gives the same numbers
    host = plan.sample_points(seed, m, begin=begin, want_terms=True, want_active=True)
    for got, dev in zip(host, (vals, total, terms, active)):
        np.testing.assert_array_equal(got.view(np.uint8), np.ascontiguousarray(dev).view(np.uint8))
    if m == 1000:
        cond = np.array([t.cond_count > 0 for t in cs.engine_tables()[0]])
        assert on[~cond].all()
        assert on[cond].any(axis=1).all() and (~on[cond]).any(axis=1).all(), name
        if name == 'cat300':
            # the 300-option table is in use: options past the 256th are drawn
            assert vals[cs.labels.index('c')].max() >= 256


@pytest.mark.parametrize('name', ['cond', 'cat300'])
def test_chunks_and_seeds(name):
    plan = _plan(name)
    seed, _ = DRAW[name]
    kw = dict(want_terms=True, want_active=True)
    whole = plan.sample_points(seed, 300, begin=0, **kw)
    a = plan.sample_points(seed, 100, begin=0, **kw)
    b = plan.sample_points(seed, 200, begin=100, **kw)
    for w, x, y in zip(whole, a, b):
        np.testing.assert_array_equal(w.view(np.uint8),
                                      np.concatenate([x, y], axis=-1).view(np.uint8))
    again = plan.sample_points(seed, 300, begin=0, **kw)
    for w, x in zip(whole, again):
        np.testing.assert_array_equal(w.view(np.uint8), x.view(np.uint8))
    other = plan.sample_points(seed + 1, 300, begin=0, **kw)
    assert (_bits(other[0]) != _bits(whole[0])).mean() > 0.5
    assert (_bits(other[1]) != _bits(whole[1])).mean() > 0.5
    # device mode without the optional outputs
    eng = plan.engine
    v = E.DeviceBuffer(eng, 8 * plan.n_hp * 300)
    t = E.DeviceBuffer(eng, 8 * 300)
    plan.sample_points_device(seed, 0, 300, 300, v.ptr, t.ptr)
    _same(v.download(np.empty((plan.n_hp, 300))), whole[0])
    _same(t.download(np.empty(300)), whole[1])


def test_suggest_is_not_disturbed():
    dom, trials = _fixture_trials('cond')
    kw = dict(n_EI_candidates=64)
    first = tpe.suggest([500], dom, trials, 7, **kw)[0]['misc']['vals']
    plan = dom._tpe_state.plan
    a = plan.suggest([11], 4096)
    kept = plan.results().copy()
    vals, total = plan.sample_points(3, 500)
    np.testing.assert_array_equal(plan.results().view(np.uint8), kept.view(np.uint8))
    b = plan.suggest([11], 4096)
    np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
    assert tpe.suggest([500], dom, trials, 7, **kw)[0]['misc']['vals'] == first
    # and the draws are those of a plan that never suggested
    want = _plan('cond').sample_points(3, 500)
    _same(vals, want[0])
    _same(total, want[1])


def test_argument_checks():
    plan = _plan('cond')
    lib = plan.engine.lib
    buf = np.zeros(14 * 8)
    p = buf.ctypes.data
    bad = [(1, 0, -1, 4, p, p), (1, 0, 4, 3, p, p), (1, -1, 4, 4, p, p), (1, 0, 4, 4, None, p),
           (1, 0, 4, 4, p, None)]
    for seed, begin, m, ld, v, t in bad:
        assert lib.tpe_plan_sample_points(plan.p, seed, begin, m, ld, v, t, None, None, 0,
                                          None) == E.TPE_E_INVALID
    assert lib.tpe_plan_sample_points(plan.p, 1, 0, 0, 0, None, None, None, None, 0,
                                      None) == E.TPE_OK
    vals, total = plan.sample_points(1, 0)
    assert vals.shape == (14, 0) and total.shape == (0,)
    dom, losses, hv, ha = _history('cond')
    hps, conds, pprior = dom.space.engine_tables()
    raw = E.Plan(E.default_engine(), hps, conds, pprior, max_trials=losses.size)
    raw.set_history(losses, hv, ha)
    with pytest.raises(ValueError, match='not been fitted'):
        raw.sample_points(1, 4)
    # top-k and gather
    idx = np.zeros(8, dtype=np.int32)
    for k in (0, 4097, -1):
        assert lib.tpe_plan_topk_points(plan.p, p, None, 5000, k, idx.ctypes.data, 0,
                                        None) == E.TPE_E_INVALID
    assert lib.tpe_plan_topk_points(plan.p, p, None, -1, 1, idx.ctypes.data, 0,
                                    None) == E.TPE_E_INVALID
    assert lib.tpe_plan_topk_points(plan.p, p, None, 2 ** 31, 1, idx.ctypes.data, 0,
                                    None) == E.TPE_E_INVALID
    assert lib.tpe_plan_topk_points(plan.p, None, None, 8, 1, idx.ctypes.data, 0,
                                    None) == E.TPE_E_INVALID
    assert lib.tpe_plan_topk_points(plan.p, p, None, 8, 1, None, 0, None) == E.TPE_E_INVALID
    with pytest.raises(IndexError):
        plan.gather_points(np.zeros((14, 8)), [0, 8])
    with pytest.raises(ValueError):
        plan.gather_points(np.zeros((13, 8)), [0])
    assert plan.gather_points(np.zeros((14, 8)), []).shape == (14, 0)


def _crafted_totals(m, seed):
    """Totals with many exact ties, NaN, +-inf and both zeros."""
    rs = np.random.RandomState(seed)
    t = rs.randint(-3, 4, m).astype(np.float64) * 0.5
    t[rs.rand(m) < 0.1] = np.nan
    t[rs.rand(m) < 0.05] = np.inf
    t[rs.rand(m) < 0.05] = -np.inf
    t[rs.rand(m) < 0.1] = -0.0
    if m >= 64:
        t[5], t[6], t[40], t[41], t[7], t[8] = np.nan, -np.inf, -0.0, 0.0, np.inf, 1.5
        t[m - 1] = np.inf
    return t


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('m', [1, 64, 65, 4099])
def test_topk_equals_rank_pool(m, masked):
    plan = _plan('cond')
    eng = plan.engine
    total = _crafted_totals(m, m)
    if m == 4099:
        assert sum(np.isnan(total)) > 100 and (np.signbit(total) & (total == 0)).any()
    for k in sorted({1, 2, 64, min(m, 4096)}):
        if k > m:
            continue
        mask = None
        if masked:
            mask = np.random.RandomState(k).rand(m) < 0.7
            if mask.sum() < k:
                # all but the entry that ranks first (none to spare when k == m)
                mask[:] = True
                if k < m:
                    mask[tpe.rank_pool(total, mask, 1)[0]] = False
        want = tpe.rank_pool(total, np.ones(m, dtype=bool) if mask is None else mask, k)
        got = plan.topk_points(total, k, eligible=mask)
        assert got.dtype == np.int32
        np.testing.assert_array_equal(got, want, err_msg='m=%d k=%d' % (m, k))
        # the device entry point
        dt = E.DeviceBuffer(eng, 8 * m).upload(total)
        dm = E.DeviceBuffer(eng, m).upload(mask.astype(np.uint8)) if masked else None
        di = E.DeviceBuffer(eng, 4 * k)
        plan.topk_points(dt.ptr, k, eligible=dm.ptr if masked else None, m=m, out=di.ptr)
        np.testing.assert_array_equal(di.download(np.empty(k, dtype=np.int32)), want)
    # too few eligible entries
    if m < 4096:
        with pytest.raises(ValueError, match='eligible'):
            plan.topk_points(total, m + 1)
    few = np.zeros(m, dtype=bool)
    few[:m // 2] = True
    with pytest.raises(ValueError, match='eligible'):
        plan.topk_points(total, m // 2 + 1, eligible=few)
    dt = E.DeviceBuffer(eng, 8 * m).upload(total)
    dm = E.DeviceBuffer(eng, m).upload(few.astype(np.uint8))
    di = E.DeviceBuffer(eng, 4 * (m // 2 + 1))
    with pytest.raises(ValueError, match='eligible'):
        plan.topk_points(dt.ptr, m // 2 + 1, eligible=dm.ptr, m=m, out=di.ptr)


def test_gather_returns_the_picked_columns():
    plan = _plan('cond')
    eng = plan.engine
    vals, total = plan.sample_points(5, 777)
    idx = plan.topk_points(total, 64)
    _same(plan.gather_points(vals, idx), vals[:, idx])
    ld = 800
    wide = np.full((14, ld), -7.0)
    wide[:, :777] = vals
    dv = E.DeviceBuffer(eng, wide.nbytes).upload(wide)
    di = E.DeviceBuffer(eng, 4 * 64).upload(idx)
    do = E.DeviceBuffer(eng, 8 * 14 * 64 + 8).upload(np.full(14 * 64 + 1, -5.0))
    plan.gather_points(dv.ptr, di.ptr, k=64, ld=ld, out=do.ptr)
    out = do.download(np.empty(14 * 64 + 1))
    _same(out[:-1].reshape(14, 64), vals[:, idx])
    assert out[-1] == -5.0
    assert np.isnan(vals[:, idx]).any()     # (inactive slots travel as NaN)


def _values(docs):
    return [{lab: v[0] for lab, v in d['misc']['vals'].items() if v} for d in docs]


def test_sample_configs_is_the_plan_call():
    dom, trials = _fixture_trials('cond')
    cs = dom.space
    vals, ei = tpe.sample_configs(200, dom, trials, 5, begin=3)
    assert vals.shape == (14, 200) and ei.shape == (200,)
    want = dom._tpe_state.plan.sample_points(tpe.batch_seeds(5, 1)[0], 200, begin=3)
    _same(vals, want[0])
    _same(ei, want[1])
    # the domain's plan holds the fixture's history and fit
    ref = _plan('cond').sample_points(5, 200, begin=3)
    _same(vals, ref[0])
    _same(ei, ref[1])
    _same(ei, tpe.score_configs(vals, dom, trials))
    cfgs, ei2 = tpe.sample_configs(200, dom, trials, 5, begin=3, as_dicts=True)
    _same(ei2, ei)
    assert cfgs == tpe.columns_to_configs(cs, vals, ~np.isnan(vals))
    assert all(cs.is_active(lab, c) == (lab in c) for c in cfgs for lab in cs.labels)


def _feasible(c):
    with np.errstate(invalid='ignore'):
        return (c['aa'] < 0.6) & (c['top'] != 2)


def test_suggest_joint_picks_follow_the_rule():
    dom, trials = _fixture_trials('cond')
    cs = dom.space
    n, ids = 1000, [120, 121, 122]
    vals, ei = tpe.sample_configs(n, dom, trials, 21)
    _, _, hv, ha = tpe.build_history(dom, trials)
    every = np.ones(n, dtype=bool)
    want = _restate(ei, every, vals, hv, ha, 3, True)
    docs = tpe.suggest_joint(ids, dom, trials, 21, n_configs=n, n_startup_jobs=0)
    assert [d['tid'] for d in docs] == ids
    assert _values(docs) == tpe.columns_to_configs(cs, vals[:, want], ~np.isnan(vals[:, want]))
    assert want == tpe.rank_pool(ei, every, 3).tolist()      # (continuous draws: no duplicates)
    for d, nid in zip(docs, ids):
        c = _values([d])[0]
        assert d['misc']['idxs'] == {lab: ([nid] if lab in c else []) for lab in cs.labels}
    # under a predicate on two labels
    mask = _feasible({lab: vals[i] for i, lab in enumerate(cs.labels)})
    assert 0 < mask.sum() < n
    want_f = _restate(ei, mask, vals, hv, ha, 3, True)
    assert mask[want_f].all()
    docs = tpe.suggest_joint(ids, dom, trials, 21, n_configs=n, n_startup_jobs=0,
                             feasible=_feasible)
    got = _values(docs)
    assert got == tpe.columns_to_configs(cs, vals[:, want_f], ~np.isnan(vals[:, want_f]))
    assert all(c['aa'] < 0.6 and c['top'] != 2 for c in got)
    with pytest.raises(ValueError, match='feasible'):
        tpe.suggest_joint(ids, dom, trials, 21, n_configs=n, n_startup_jobs=0,
                          feasible=lambda c: np.ones(n))
    with pytest.raises(ValueError):
        tpe.suggest_joint(ids, dom, trials, 21, n_configs=n, n_startup_jobs=0,
                          feasible=lambda c: np.zeros(n, dtype=bool))


def _six_trials(drop, extra=()):
    """40 prior trials of the 6-configuration space without the
    configurations in ``drop``, then ``extra`` ones."""
    dom = Domain(lambda x: 0.0, six_space(hp))
    docs = [d for d in rand.suggest(list(range(40)), dom, Trials(), 41)
            if (d['misc']['vals']['p'][0], d['misc']['vals']['q'][0]) not in drop]
    cs = dom.space
    docs += [tpe._new_doc(dom, Trials(), cs, 100 + j, {'p': p, 'q': q})
             for j, (p, q) in enumerate(extra)]
    return dom, _done(docs, 43)


def test_duplicates_in_a_six_configuration_space():
    dom, trials = _six_trials(drop=())
    cs = dom.space
    assert len(trials) == 40
    vals, ei = tpe.sample_configs(256, dom, trials, 9)
    _, _, hv, ha = tpe.build_history(dom, trials)
    keys = [tuple(c) for c in vals.T]
    assert len(set(keys)) == 6
    kw = dict(n_configs=256, n_startup_jobs=0, skip_seen=False)
    every = np.ones(256, dtype=bool)
    got4 = _values(tpe.suggest_joint([0, 1, 2, 3], dom, trials, 9, **kw))
    assert len({(c['p'], c['q']) for c in got4}) == 4
    want4 = _restate(ei, every, vals, hv, ha, 4, False)
    assert got4 == tpe.columns_to_configs(cs, vals[:, want4], np.ones((2, 4), dtype=bool))
    got8 = _values(tpe.suggest_joint(list(range(8)), dom, trials, 9, **kw))
    assert len({(c['p'], c['q']) for c in got8[:6]}) == 6
    want8 = _restate(ei, every, vals, hv, ha, 8, False)
    assert [(c['p'], c['q']) for c in got8] == [tuple(int(x) for x in vals[:, j]) for j in want8]
    # the two fills are the best-ranked duplicates: of the configuration that ranks first
    order = tpe.rank_pool(ei, every, 256)
    assert want8[6:] == [j for j in order if j not in want8[:6]][:2]
    assert keys[want8[6]] == keys[want8[0]]
    # every configuration is a history row: nothing is left with skip_seen
    with pytest.raises(ValueError):
        tpe.suggest_joint([0], dom, trials, 9, n_configs=256, n_startup_jobs=0)


def test_skip_seen_drops_history_rows():
    unseen = [(0, 2), (1, 0)]
    dom, trials = _six_trials(drop=unseen)
    kw = dict(n_configs=256, n_startup_jobs=0)
    got = _values(tpe.suggest_joint([0, 1], dom, trials, 9, **kw))
    assert sorted((c['p'], c['q']) for c in got) == unseen
    vals, ei = tpe.sample_configs(256, dom, trials, 9)
    _, _, hv, ha = tpe.build_history(dom, trials)
    want = _restate(ei, np.ones(256, dtype=bool), vals, hv, ha, 2, True)
    assert [(c['p'], c['q']) for c in got] == [tuple(int(x) for x in vals[:, j]) for j in want]
    # three asked for: the third is a duplicate of a taken one, never a seen one
    got3 = _values(tpe.suggest_joint([0, 1, 2], dom, trials, 9, **kw))
    assert all((c['p'], c['q']) in unseen for c in got3)
    # one of the two copied into the history: only the other is left
    dom2, trials2 = _six_trials(drop=unseen, extra=[unseen[0]])
    got = _values(tpe.suggest_joint([0], dom2, trials2, 9, **kw))
    assert [(c['p'], c['q']) for c in got] == [unseen[1]]


def test_fmin_under_a_predicate():
    t = Trials()
    algo = functools.partial(tpe.suggest_joint, n_configs=512, feasible=_feasible,
                             n_startup_jobs=10)
    fmin(lambda x: float(np.sin(3 * x['aa'])), spaces.cond_space(hp), algo=algo, max_evals=30,
         trials=t, rstate=np.random.RandomState(3))
    assert len(t) == 30
    for tr in t.trials:
        v = tr['misc']['vals']
        assert v['aa'][0] < 0.6 and v['top'][0] != 2
