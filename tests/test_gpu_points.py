"""Whole configurations scored under the fitted model on the GPU
(tpe_plan_score_points, tpe.score_configs, tpe.suggest_from_pool) against the
stable-tie CPU oracle.

The configurations are the rows of the committed suggest fixtures (their own
histories scored as pools).  Tolerances are the project's 1e-6 bar on each lpdf
(gpu_util.RTOL) applied to the two lpdfs of a term,
    |d term|  <= 1e-6 (max(1, |llik_b|) + max(1, |llik_a|)),
and summed over a configuration's active hps for its total; the total must
also be the float64 sum of the returned terms in hp order, bit for bit."""
import functools

import numpy as np
import pytest

import hyperopt_amd as H
from hyperopt_amd import hp, tpe, rand, Trials, trials_from_docs
from hyperopt_amd import _engine as E
from hyperopt_amd.base import Domain

from golden_io import load, load_json
from gpu_util import RTOL
import spaces

pytestmark = pytest.mark.gpu

SPACES = {'cfg2': spaces.cfg2_space, 'many_dists': spaces.many_dists_space,
          'cond': spaces.cond_space, 'cfg3_small': spaces.cfg3_space}
SHAPES = {'cfg2': (20, 1000), 'many_dists': (11, 60), 'cond': (14, 120), 'cfg3_small': (50, 300)}
GAMMA, PRIOR_WEIGHT = 0.25, 1.0


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _fixture(name):
    meta = load_json('suggest_meta.json')[name]
    d = load('suggest_%s.npz' % name)
    dom = Domain(lambda x: 0.0, SPACES[name](hp))
    assert list(meta['labels']) == dom.space.labels
    assert d['vals'].shape == SHAPES[name]
    return meta, d, dom


def _oracle_lliks(cs, losses, hist_vals, hist_active, vals, active, gamma=GAMMA, gamma_cap=25):
    """(llik_b, llik_a)[P, M] of the configurations' active values under the
    oracle's fit of the history (stable ties), NaN where inactive."""
    from oracle import tpe_oracle as O
    from oracle_algo import oracle_hps
    hps = oracle_hps(cs)
    tids = np.arange(losses.size)
    lb = np.full(vals.shape, np.nan)
    la = np.full(vals.shape, np.nan)
    for i, lab in enumerate(cs.labels):
        on, at = hist_active[i] == 1, active[i] == 1
        if not at.any():
            continue
        bo, ao = O.split_observations(tids[on], hist_vals[i][on], tids, losses, gamma,
                                      gamma_cap, kind='stable')
        with np.errstate(all='ignore'):
            r = O.score_hp(hps[lab]['dist'], hps[lab]['args'], bo, ao, PRIOR_WEIGHT,
                           vals[i][at], kind='stable')
        lb[i, at], la[i, at] = r['llik_b'], r['llik_a']
    return lb, la


@functools.lru_cache(maxsize=None)
def _oracle(name):
    _, d, dom = _fixture(name)
    return _frozen(*_oracle_lliks(dom.space, d['losses'], d['vals'], d['active'], d['vals'],
                                  d['active']))


def _oracle_total(lb, la, active):
    with np.errstate(all='ignore'):
        return np.where(active == 1, lb - la, 0.0).sum(axis=0)


def _term_bound(lb, la, active):
    with np.errstate(all='ignore'):
        b = RTOL * (np.maximum(1.0, np.abs(lb)) + np.maximum(1.0, np.abs(la)))
    return np.where(active == 1, b, 0.0)


def _new_plan(cs, losses, vals, active, fit=True):
    hps, conds, pprior = cs.engine_tables()
    plan = E.Plan(E.default_engine(), hps, conds, pprior, max_trials=losses.size)
    plan.set_history(losses, vals, active)
    if fit:
        plan.fit(gamma=GAMMA, prior_weight=PRIOR_WEIGHT)
    return plan


@functools.lru_cache(maxsize=None)
def _plan(name):
    _, d, dom = _fixture(name)
    return _new_plan(dom.space, d['losses'], d['vals'], d['active'])


@functools.lru_cache(maxsize=None)
def _scored(name):
    """(total, terms, active) of the fixture's rows, computed once."""
    _, d, _ = _fixture(name)
    return _frozen(*_plan(name).score_points(d['vals'], want_terms=True, want_active=True))


def _fixture_trials(name):
    meta, d, dom = _fixture(name)
    dom = Domain(lambda x: 0.0, SPACES[name](hp))       # (a fresh plan per test)
    docs = rand.suggest(list(range(meta['n'])), dom, Trials(), meta['hist_seed'])
    for doc, l in zip(docs, d['losses']):
        doc['state'] = H.JOB_STATE_DONE
        doc['result'] = {'status': 'ok', 'loss': float(l)}
    return meta, d, dom, trials_from_docs(docs)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check_against_oracle(total, terms, active, lb, la, want_active, msg):
    np.testing.assert_array_equal(active, want_active, err_msg=msg)
    on = want_active == 1
    assert np.isfinite(lb[on]).all() and np.isfinite(la[on]).all(), msg
    # inactive: +0.0 exactly
    assert (_bits(terms)[~on] == 0).all(), msg
    err = np.abs(terms - np.where(on, lb - la, 0.0))
    bound = _term_bound(lb, la, want_active)
    print('%s: max |d term| / bound = %.3g, max |d total| = %.3g (bound %.3g)' % (
        msg, (err[on] / bound[on]).max(),
        np.abs(total - _oracle_total(lb, la, want_active)).max(), bound.sum(axis=0).max()))
    assert (err <= bound).all(), (msg, np.argwhere(err > bound)[:5])
    assert (np.abs(total - _oracle_total(lb, la, want_active)) <= bound.sum(axis=0)).all(), msg
    _check_total_is_the_sum(total, terms, msg)


def _check_total_is_the_sum(total, terms, msg=''):
    acc = np.zeros(terms.shape[1])
    with np.errstate(all='ignore'):
        for i in range(terms.shape[0]):
            acc = acc + terms[i]
    np.testing.assert_array_equal(_bits(total), _bits(acc), err_msg=msg)


def test_oracle_covers_every_active_term():
    """The four fixtures hold 23 780 active (hp, configuration) pairs; the
    oracle gives each of them a finite term, so no case is left out below."""
    n = 0
    for name in sorted(SPACES):
        _, d, dom = _fixture(name)
        lb, la = _oracle(name)
        on = d['active'] == 1
        assert np.isfinite(lb[on]).all() and np.isfinite(la[on]).all()
        np.testing.assert_array_equal(tpe.active_columns(dom.space, d['vals']), on)
        n += int(on.sum())
    assert n == 23780
    assert all(_term_bound(*_oracle(k), _fixture(k)[1]['active']).sum(axis=0).max() <= 1.3e-4
               for k in SPACES)


@pytest.mark.parametrize('name', sorted(SPACES))
def test_fixture_rows_match_oracle(name):
    _, d, _ = _fixture(name)
    total, terms, active = _scored(name)
    lb, la = _oracle(name)
    _check_against_oracle(total, terms, active, lb, la, d['active'], name)
    # the outputs are optional
    only = _plan(name).score_points(d['vals'])
    np.testing.assert_array_equal(_bits(only), _bits(total))


@pytest.mark.parametrize('name', sorted(SPACES))
def test_suggest_from_pool_top4_equals_oracle(name):
    meta, d, dom, trials = _fixture_trials(name)
    cs = dom.space
    lb, la = _oracle(name)
    want_total = _oracle_total(lb, la, d['active'])
    want = np.argsort(-want_total, kind='stable')[:4]
    gaps = -np.diff(np.sort(want_total)[::-1][:5])
    assert gaps.min() > 100 * 1.3e-4            # index equality is safe
    pool = np.where(d['active'] == 1, d['vals'], np.nan)
    ids = [meta['n'] + j for j in range(4)]
    algo = functools.partial(tpe.suggest_from_pool, pool=pool, skip_seen=False, n_startup_jobs=0)
    docs = algo(ids, dom, trials, 1)
    got = [{lab: v[0] for lab, v in doc['misc']['vals'].items() if v} for doc in docs]
    assert got == tpe.columns_to_configs(cs, d['vals'][:, want], d['active'][:, want])
    assert [doc['tid'] for doc in docs] == ids
    # the cached pool serves the next call; with skip_seen every row of this
    # pool is a history row
    assert [x['misc']['vals'] for x in algo(ids, dom, trials, 2)] == \
        [x['misc']['vals'] for x in docs]
    with pytest.raises(ValueError, match='eligible'):
        tpe.suggest_from_pool(ids, dom, trials, 1, pool=pool, n_startup_jobs=0)


def test_suggest_from_pool_skips_seen_rows():
    """Half the pool are history rows: the picks are the best of the rest."""
    meta, d, dom, trials = _fixture_trials('cond')
    cs = dom.space
    fresh_docs = rand.suggest(list(range(1000, 1060)), dom, Trials(), 77)
    fresh = [{lab: v[0] for lab, v in x['misc']['vals'].items() if v} for x in fresh_docs]
    hist = tpe.columns_to_configs(cs, d['vals'], d['active'])
    pool = hist[:60] + fresh
    total = tpe.score_configs(pool, dom, trials)
    want = 60 + np.argsort(-total[60:], kind='stable')[:3]
    docs = tpe.suggest_from_pool([120, 121, 122], dom, trials, 5, pool=pool, n_startup_jobs=0)
    got = [{lab: v[0] for lab, v in x['misc']['vals'].items() if v} for x in docs]
    assert got == [pool[j] for j in want]
    every = tpe.suggest_from_pool([120, 121, 122], dom, trials, 5, pool=pool, n_startup_jobs=0,
                                  skip_seen=False)
    want_all = np.argsort(-total, kind='stable')[:3]
    assert [{lab: v[0] for lab, v in x['misc']['vals'].items() if v} for x in every] == \
        [pool[j] for j in want_all]


def test_score_configs_dicts_and_terms():
    meta, d, dom, trials = _fixture_trials('cond')
    cs = dom.space
    cfgs = tpe.columns_to_configs(cs, d['vals'], d['active'])
    total, terms, active = tpe.score_configs(cfgs, dom, trials, return_terms=True)
    lb, la = _oracle('cond')
    t = np.stack([terms[lab] for lab in cs.labels])
    a = np.stack([active[lab] for lab in cs.labels]).astype(np.uint8)
    _check_against_oracle(total, t, a, lb, la, d['active'], 'score_configs')
    assert total.dtype == np.float64 and total.shape == (120,)
    np.testing.assert_array_equal(_bits(tpe.score_configs(cfgs, dom, trials)), _bits(total))
    # the array format gives the same numbers
    arr = np.where(d['active'] == 1, d['vals'], np.nan)
    np.testing.assert_array_equal(_bits(tpe.score_configs(arr, dom, trials)), _bits(total))
    # a dict that contradicts its own choices (checked against the device's mask)
    b = int(cfgs[0]['top'])
    bad = dict(cfgs[0])
    bad['zz%d' % ((b + 1) % 3)] = 0.0
    with pytest.raises(ValueError, match='present'):
        tpe.score_configs([cfgs[1], bad], dom, trials)
    bad = {k: v for k, v in cfgs[0].items() if k != 'zz%d' % b}
    with pytest.raises(ValueError, match='missing'):
        tpe.score_configs([bad], dom, trials)


@pytest.mark.parametrize('m', [1, 63, 64, 65, 257])
def test_sizes_around_the_wave_and_block(m):
    """A configuration's numbers do not depend on how many are scored with it."""
    _, d, _ = _fixture('cond')
    total, terms, active = _scored('cond')
    idx = np.arange(m) % 120
    got = _plan('cond').score_points(np.ascontiguousarray(d['vals'][:, idx]), want_terms=True,
                                     want_active=True)
    np.testing.assert_array_equal(_bits(got[0]), _bits(total[idx]))
    np.testing.assert_array_equal(_bits(got[1]), _bits(terms[:, idx]))
    np.testing.assert_array_equal(got[2], active[:, idx])


def test_hp_inactive_in_every_row():
    _, d, dom = _fixture('cond')
    cs = dom.space
    total, terms, active = _scored('cond')
    top = cs.labels.index('top')
    idx = np.flatnonzero(d['vals'][top] != 0)
    assert 64 < idx.size < 120
    got = _plan('cond').score_points(np.ascontiguousarray(d['vals'][:, idx]), want_terms=True,
                                     want_active=True)
    for lab in ('lr0', 'units0', 'act0', 'zz0'):
        i = cs.labels.index(lab)
        assert not got[2][i].any() and (_bits(got[1][i]) == 0).all()
    np.testing.assert_array_equal(_bits(got[0]), _bits(total[idx]))
    np.testing.assert_array_equal(_bits(got[1]), _bits(terms[:, idx]))


def test_inactive_slots_are_ignored():
    _, d, _ = _fixture('cond')
    total, terms, active = _scored('cond')
    on = d['active'] == 1
    rs = np.random.RandomState(3)
    for fill in (np.full(on.shape, np.nan), rs.uniform(-1e300, 1e300, on.shape),
                 np.full(on.shape, np.inf), rs.randint(0, 3, on.shape).astype(np.float64)):
        top = np.where(on, d['vals'], fill)
        got = _plan('cond').score_points(top, want_terms=True, want_active=True)
        np.testing.assert_array_equal(_bits(got[0]), _bits(total))
        np.testing.assert_array_equal(_bits(got[1]), _bits(terms))
        np.testing.assert_array_equal(got[2], active)


def test_device_entry_point_with_a_wider_leading_dimension():
    _, d, _ = _fixture('cond')
    plan = _plan('cond')
    eng = plan.engine
    total, terms, active = _scored('cond')
    P, M, ld = 14, 120, 200
    wide = np.full((P, ld), 7.0)
    wide[:, :M] = d['vals']
    v = E.DeviceBuffer(eng, wide.nbytes).upload(wide)
    tot = E.DeviceBuffer(eng, 8 * (M + 8)).upload(np.full(M + 8, -5.0))
    trm = E.DeviceBuffer(eng, 8 * P * ld).upload(np.full((P, ld), -5.0))
    act = E.DeviceBuffer(eng, P * ld).upload(np.full((P, ld), 9, dtype=np.uint8))
    plan.score_points_device(v.ptr, M, ld, tot.ptr, trm.ptr, act.ptr)
    tot = tot.download(np.empty(M + 8))
    trm = trm.download(np.empty((P, ld)))
    act = act.download(np.empty((P, ld), dtype=np.uint8))
    np.testing.assert_array_equal(_bits(tot[:M]), _bits(total))
    np.testing.assert_array_equal(_bits(trm[:, :M]), _bits(terms))
    np.testing.assert_array_equal(act[:, :M], active)
    # nothing past M is written
    assert (tot[M:] == -5.0).all() and (trm[:, M:] == -5.0).all() and (act[:, M:] == 9).all()
    # the host entry point with the same wider rows
    h_tot, h_trm = np.full(M, -5.0), np.full((P, ld), -5.0)
    h_act = np.full((P, ld), 9, dtype=np.uint8)
    eng.check(eng.lib.tpe_plan_score_points(plan.p, wide.ctypes.data, M, ld, h_tot.ctypes.data,
                                            h_trm.ctypes.data, h_act.ctypes.data, 0, None))
    np.testing.assert_array_equal(_bits(h_tot), _bits(total))
    np.testing.assert_array_equal(_bits(h_trm), _bits(trm))
    np.testing.assert_array_equal(h_act, act)
    # without the optional outputs
    tot2 = E.DeviceBuffer(eng, 8 * M).upload(np.zeros(M))
    plan.score_points_device(v.ptr, M, ld, tot2.ptr)
    np.testing.assert_array_equal(_bits(tot2.download(np.empty(M))), _bits(total))


def test_suggest_is_not_disturbed():
    meta, d, dom, trials = _fixture_trials('cond')
    kw = dict(n_EI_candidates=64)
    first = tpe.suggest([meta['new_id']], dom, trials, 7, **kw)[0]['misc']['vals']
    plan = dom._tpe_state.plan
    a = plan.suggest([11], 4096)
    kept = plan.results().copy()
    total = plan.score_points(d['vals'])
    np.testing.assert_array_equal(plan.results().view(np.uint8), kept.view(np.uint8))
    b = plan.suggest([11], 4096)
    np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
    assert tpe.suggest([meta['new_id']], dom, trials, 7, **kw)[0]['misc']['vals'] == first
    # and the scores are those of a plan that never suggested
    np.testing.assert_array_equal(_bits(total), _bits(_scored('cond')[0]))


def test_argument_checks():
    _, d, dom = _fixture('cond')
    plan = _plan('cond')
    e = plan.engine
    empty = plan.score_points(np.zeros((14, 0)))
    assert empty.shape == (0,)
    with pytest.raises(ValueError):
        plan.score_points(np.zeros((13, 4)))
    buf = np.zeros(64)
    lib = e.lib
    assert lib.tpe_plan_score_points(plan.p, buf.ctypes.data, -1, 4, buf.ctypes.data, None, None,
                                     0, None) == E.TPE_E_INVALID
    assert lib.tpe_plan_score_points(plan.p, buf.ctypes.data, 4, 3, buf.ctypes.data, None, None,
                                     0, None) == E.TPE_E_INVALID
    assert lib.tpe_plan_score_points(plan.p, None, 4, 4, buf.ctypes.data, None, None,
                                     0, None) == E.TPE_E_INVALID
    assert lib.tpe_plan_score_points(plan.p, buf.ctypes.data, 4, 4, None, None, None,
                                     0, None) == E.TPE_E_INVALID
    assert lib.tpe_plan_score_points(plan.p, None, 0, 0, None, None, None, 0, None) == E.TPE_OK
    raw = _new_plan(dom.space, d['losses'], d['vals'], d['active'], fit=False)
    with pytest.raises(ValueError, match='not been fitted'):
        raw.score_points(d['vals'])


def test_long_history():
    """2100 trials of a 3-d uniform space: the above mixtures have 2089
    components (past kRangeMinK = 2048, not a multiple of 8) and the fit takes
    its global-memory path."""
    dom = Domain(lambda x: 0.0, spaces.cfg4_space(hp, 3))
    cs = dom.space
    rs = np.random.RandomState(21)
    hv = rs.uniform(-5, 5, (3, 2100))
    losses = rs.rand(2100)
    ha = np.ones((3, 2100), dtype=np.uint8)
    vals = np.random.RandomState(22).uniform(-5, 5, (3, 300))
    act = np.ones((3, 300), dtype=np.uint8)
    plan = _new_plan(cs, losses, hv, ha)
    assert plan.mixture(0, 1)[0].size == 2089
    got = plan.score_points(vals, want_terms=True, want_active=True)
    lb, la = _oracle_lliks(cs, losses, hv, ha, vals, act)
    _check_against_oracle(got[0], got[1], got[2], lb, la, act, 'long history')


def _klass(x):
    return np.where(np.isnan(x), 2, np.where(np.isinf(x), np.sign(x), 0)).astype(int)


def test_non_finite_values():
    """A uniform value outside [low, high], and a choice of `upper` and of
    1.5: each term and total falls in numpy's class (finite / -inf / +inf /
    NaN) for the stated semantics."""
    _, d, dom = _fixture('many_dists')
    cs = dom.space
    vals = np.ascontiguousarray(d['vals'][:, :4]).copy()
    lab = cs.labels.index
    vals[lab('c'), 0] = 9.0         # uniform(4, 7)
    vals[lab('c'), 1] = -3.0
    vals[lab('a'), 2] = 3.0         # choice of 3: upper
    vals[lab('a'), 3] = 1.5
    act = np.ones(vals.shape, dtype=np.uint8)
    got = _plan('many_dists').score_points(vals, want_terms=True, want_active=True)
    np.testing.assert_array_equal(got[2], act)
    lb, la = _oracle_lliks(cs, d['losses'], d['vals'], d['active'],
                           np.where(np.isin(vals, (3.0, 1.5)) & (np.arange(11)[:, None] == lab('a')),
                                    0.0, vals), act)
    with np.errstate(all='ignore'):
        want = lb - la
    want[lab('a'), 2:] = np.nan     # not an option index: NaN
    np.testing.assert_array_equal(_klass(got[1]), _klass(want))
    np.testing.assert_array_equal(_klass(got[0]), _klass(want.sum(axis=0)))
    assert np.isnan(got[0][2:]).all() and np.isfinite(got[0][:2]).all()
    _check_total_is_the_sum(got[0], got[1])
    # in a conditional space the children of such a choice stay inactive
    _, dc, domc = _fixture('cond')
    top = domc.space.labels.index('top')
    v = np.ascontiguousarray(dc['vals'][:, :3]).copy()
    v[top] = [3.0, 1.5, np.nan]
    t, trm, a = _plan('cond').score_points(v, want_terms=True, want_active=True)
    np.testing.assert_array_equal(a, tpe.active_columns(domc.space, v))
    assert a.sum() == 6 and np.isnan(trm[top]).all() and np.isnan(t).all()
    assert np.isfinite(trm[domc.space.labels.index('aa')]).all()
