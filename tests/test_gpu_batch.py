"""The greedy batch with a pending-trial penalty on the GPU
(tpe_plan_group_batch_points, ``suggest_joint(batch='pending')``)
against ``batch_oracle``'s numpy restatement.

Everything the engine defines in terms of its own outputs is compared bit for
bit: round 0's scores are the call's total, a gain is the trace's entry, and
the picks are the selection rule applied to the device's own trace.  The
scores themselves are compared with the oracle replayed on the device's
picks: per active group |d| <= RTOL max(1, |value|) on each of J_below and Ja
(test_gpu_group.py's bar), summed over the groups.  On the fixtures -- every
round of which test_batch_host.py proves decided by 4x that bound -- the
picks are the oracle's."""
import functools

import numpy as np
import pytest

from hyperopt_amd import fmin, hp, tpe, rand, Trials
from hyperopt_amd import _engine as E
from hyperopt_amd.base import Domain

from golden_io import load_json
import batch_cases as C
import batch_oracle as B
import spaces

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b, msg=''):
    np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=msg)


def _new_plan(name, group_fit=True):
    dom, losses, vals, active = C.history(name)
    hps, conds, pprior = dom.space.engine_tables()
    plan = E.Plan(E.default_engine(), hps, conds, pprior, max_trials=losses.size)
    plan.set_history(np.ascontiguousarray(losses), np.ascontiguousarray(vals),
                     np.ascontiguousarray(active))
    plan.fit(gamma=C.GAMMA, prior_weight=C.PRIOR_WEIGHT)
    if group_fit:
        plan.group_fit()
    return plan


_plan = functools.lru_cache(maxsize=None)(_new_plan)


def _batch(plan, vals, k, eligible=None):
    """(total, idx, gain, trace) of a score followed by the batch."""
    vals = np.ascontiguousarray(vals)
    total = plan.group_score_points(vals)
    idx, gain, trace = plan.group_batch_points(vals, k, eligible=eligible, want_trace=True)
    return total, idx, gain, trace


def _check_identities(plan, model, vals, k, total, idx, gain, trace, eligible=None, msg=''):
    """What the engine defines in terms of its own outputs."""
    _same(trace[0], total, msg)
    if eligible is None:
        assert idx[0] == plan.topk_points(total, 1)[0], msg
    _same(gain, trace[np.arange(k), idx], msg)
    np.testing.assert_array_equal(idx, B.apply_rule(trace, B.config_keys(model, vals), eligible),
                                  err_msg=msg)
    assert len(set(idx.tolist())) == k


def _check_trace(model, vals, idx, trace, eligible=None, msg=''):
    """The device's scores against the oracle replayed on the device's picks."""
    res = B.run(model, vals, len(idx), eligible=eligible, forced=idx,
                prior_weight=C.PRIOR_WEIGHT)
    nan = np.isnan(res.scores)
    np.testing.assert_array_equal(np.isnan(trace), nan, err_msg=msg)
    err = np.abs(trace - res.scores)
    ok = nan | (err <= res.bound)
    worst = float(np.max(np.where(nan, 0.0, err / res.bound)))
    print('%s: max |d score| / bound = %.3g' % (msg, worst))
    assert ok.all(), (msg, np.argwhere(~ok)[:5])
    # the penalty is there: the later rounds differ from round 0
    if len(idx) > 1:
        assert (trace[-1] != trace[0]).sum() > 1, msg
    return res


# ---------------------------------------------------------------- the model
@pytest.mark.parametrize('name', C.NAMES)
def test_fixture_batches_match_the_oracle(name):
    plan, model = _plan(name), C.model(name)
    vals = np.ascontiguousarray(C.configs(name))
    total, idx, gain, trace = _batch(plan, vals, C.K)
    _check_identities(plan, model, vals, C.K, total, idx, gain, trace, msg=name)
    _check_trace(model, vals, idx, trace, msg=name)
    np.testing.assert_array_equal(idx, C.oracle_run(name).picks, err_msg=name)
    # without the optional outputs, and again: the call leaves the sides as they were
    idx2, gain2 = plan.group_batch_points(vals, C.K)
    np.testing.assert_array_equal(idx2, idx)
    _same(gain2, gain)
    _same(plan.group_score_points(vals), total)


@pytest.mark.parametrize('m, k', C.SHAPES)
def test_launch_shapes(m, k):
    """One block, a block boundary, more than one block, k = m; host and
    device mode; rows longer than m with sentinels behind them."""
    plan, model = _plan('cond'), C.model('cond')
    vals = np.ascontiguousarray(C.configs('cond')[:, :m])
    msg = 'cond m=%d k=%d' % (m, k)
    total, idx, gain, trace = _batch(plan, vals, k)
    _check_identities(plan, model, vals, k, total, idx, gain, trace, msg=msg)
    _check_trace(model, vals, idx, trace, msg=msg)
    np.testing.assert_array_equal(idx, C.oracle_run('cond', m, k).picks, err_msg=msg)
    # device pointers
    eng, P, ld = plan.engine, plan.n_hp, m + 9
    pad = np.full((P, ld), np.nan)
    pad[:, :m] = vals
    v = E.DeviceBuffer(eng, 8 * P * ld).upload(pad)
    tot = E.DeviceBuffer(eng, 8 * ld).upload(np.full(ld, -7.0))
    d_idx = E.DeviceBuffer(eng, 4 * (k + 1)).upload(np.full(k + 1, -7, dtype=np.int32))
    d_gain = E.DeviceBuffer(eng, 8 * (k + 1)).upload(np.full(k + 1, -7.0))
    d_trace = E.DeviceBuffer(eng, 8 * k * ld).upload(np.full((k, ld), -7.0))
    plan.group_score_points_device(v.ptr, m, ld, tot.ptr)
    plan.group_batch_points_device(v.ptr, m, ld, k, d_idx.ptr, d_gain.ptr, trace_ptr=d_trace.ptr)
    eng.synchronize()
    di = d_idx.download(np.empty(k + 1, dtype=np.int32))
    dg = d_gain.download(np.empty(k + 1))
    dt = d_trace.download(np.empty((k, ld)))
    assert di[k] == -7 and dg[k] == -7.0 and (dt[:, m:] == -7.0).all()
    np.testing.assert_array_equal(di[:k], idx)
    _same(dg[:k], gain)
    _same(dt[:, :m], trace)
    # ... and without gain and trace
    d_idx.upload(np.full(k + 1, -7, dtype=np.int32))
    plan.group_batch_points_device(v.ptr, m, ld, k, d_idx.ptr)
    eng.synchronize()
    np.testing.assert_array_equal(d_idx.download(np.empty(k + 1, dtype=np.int32))[:k], idx)


def test_repeated_columns_ties_and_a_bad_value():
    """Equal configurations tie bit for bit: the lower index wins, and once
    it is taken its copies sink below every other configuration; a NaN score
    is last among those.  k = m."""
    plan, model = _plan('cond'), C.model('cond')
    labels = C.history('cond')[0].space.labels
    base = C.configs('cond')[:, :70]
    vals = np.ascontiguousarray(np.concatenate([base, base[:, :66], base[:, [2]]], axis=1))
    vals[labels.index('aa'), 136] = np.nan
    m = vals.shape[1]
    total, idx, gain, trace = _batch(plan, vals, m)
    _same(total[70:136], total[:66])
    assert np.isnan(total[136])
    _check_identities(plan, model, vals, m, total, idx, gain, trace, msg='repeats')
    assert sorted(idx[:70].tolist()) == list(range(70))      # every distinct one first
    assert idx[70] == 136                                     # the NaN one last of them
    assert sorted(idx[71:].tolist()) == list(range(70, 136))  # then the copies
    _check_trace(model, vals, idx[:8], trace[:8], msg='repeats')
    # (-0.0 equals +0.0 in a value: a copy with the sign flipped is a copy)
    z = np.ascontiguousarray(np.concatenate([base[:, :3], base[:, :3]], axis=1))
    zz = labels.index('zz%d' % int(z[labels.index('top'), 0]))
    z[zz, 0], z[zz, 3] = 0.0, -0.0
    _, zi, _, _ = _batch(plan, z, 6)
    assert sorted(int(i) % 3 for i in zi[:3]) == [0, 1, 2]


def test_eligible_is_honoured_and_a_short_batch_is_an_error():
    plan, model = _plan('nested'), C.model('nested')
    vals = np.ascontiguousarray(C.configs('nested')[:, :100])
    el = np.ones(100, dtype=bool)
    el[::2] = False
    total, idx, gain, trace = _batch(plan, vals, 8, eligible=el)
    assert el[idx].all()
    _check_identities(plan, model, vals, 8, total, idx, gain, trace, eligible=el, msg='masked')
    _check_trace(model, vals, idx, trace, eligible=el, msg='masked')
    # exactly k eligible: fine; one fewer: short
    few = np.zeros(100, dtype=bool)
    few[[5, 17, 64]] = True
    idx3, _ = plan.group_batch_points(vals, 3, eligible=few)
    assert sorted(idx3.tolist()) == [5, 17, 64]
    with pytest.raises(ValueError, match='fewer than k'):
        plan.group_batch_points(vals, 4, eligible=few)
    with pytest.raises(ValueError, match='fewer than k'):
        plan.group_batch_points(vals, 101)
    # the plan is usable after the error
    idx3b, _ = plan.group_batch_points(vals, 3, eligible=few)
    np.testing.assert_array_equal(idx3b, idx3)


def test_argument_errors():
    vals = np.ascontiguousarray(C.configs('cond')[:, :40])
    plan = _new_plan('cond', group_fit=False)
    with pytest.raises(ValueError, match='no group fit'):
        plan.group_batch_points(vals, 2)
    plan.group_fit()
    with pytest.raises(ValueError, match='last group score'):      # (nothing scored yet)
        plan.group_batch_points(vals, 2)
    plan.group_score_points(vals)
    idx, _ = plan.group_batch_points(vals, 2)
    with pytest.raises(ValueError, match='last group score'):      # another m
        plan.group_batch_points(np.ascontiguousarray(vals[:, :39]), 2)
    for k in (0, -1, E.BATCH_MAX + 1):
        with pytest.raises(ValueError, match='1 <= k <= 1024'):
            plan.group_batch_points(vals, k)
    with pytest.raises(ValueError):
        plan.group_batch_points(vals[:3], 2)
    np.testing.assert_array_equal(plan.group_batch_points(vals, 2)[0], idx)
    # a new fit drops the model, a new group fit the scored sides
    plan.fit(gamma=C.GAMMA, prior_weight=C.PRIOR_WEIGHT)
    with pytest.raises(ValueError, match='no group fit'):
        plan.group_batch_points(vals, 2)
    plan.group_fit()
    with pytest.raises(ValueError, match='last group score'):
        plan.group_batch_points(vals, 2)
    # a draw is a score as well
    drawn, _ = plan.group_sample_points(4, 40)
    assert plan.group_batch_points(drawn, 2)[0].size == 2


# --------------------------------------------------------- the entry points
def _fixture_trials(name):
    meta = load_json('suggest_meta.json')[name]
    dom = C.history(name)[0]
    docs = rand.suggest(list(range(meta['n'])), dom, Trials(), meta['hist_seed'])
    return dom, C.done(docs, C.history(name)[1])


def _values(docs):
    return [{lab: v[0] for lab, v in d['misc']['vals'].items() if v} for d in docs]


def _configs(cs, vals, idx):
    cols = vals[:, idx]
    return tpe.columns_to_configs(cs, cols, ~np.isnan(cols))


def test_suggest_joint_pending_is_the_plan_calls():
    dom, trials = _fixture_trials('cond')
    cs = dom.space
    n, ids = 512, [120, 121, 122, 123]
    kw = dict(n_configs=n, n_startup_jobs=0, multivariate='groups')
    plan = _plan('cond')
    vals, total = plan.group_sample_points(tpe.batch_seeds(21, 1)[0], n)
    idx, _ = plan.group_batch_points(vals, 4)
    docs = tpe.suggest_joint(ids, dom, trials, 21, batch='pending', **kw)
    assert [d['tid'] for d in docs] == ids
    assert _values(docs) == _configs(cs, vals, idx)
    # the first pick is the top-k's first, the others are not its next ones
    topk = tpe.suggest_joint(ids, dom, trials, 21, **kw)
    assert _values(topk)[0] == _values(docs)[0] and _values(topk) != _values(docs)
    assert _values(topk) == _values(tpe.suggest_joint(ids, dom, trials, 21, batch='topk', **kw))
    # skip_seen changes nothing on a continuous draw
    assert _values(tpe.suggest_joint(ids, dom, trials, 21, batch='pending', skip_seen=False,
                                     **kw)) == _values(docs)
    # a predicate over the draw
    aa = cs.labels.index('aa')

    def feasible(cols):
        return cols['aa'] < 0.5

    plan.group_sample_points(tpe.batch_seeds(21, 1)[0], n)
    fidx, _ = plan.group_batch_points(vals, 4, eligible=vals[aa] < 0.5)
    fdocs = tpe.suggest_joint(ids, dom, trials, 21, batch='pending', feasible=feasible, **kw)
    assert _values(fdocs) == _configs(cs, vals, fidx)
    assert all(c['aa'] < 0.5 for c in _values(fdocs))
    for mv in (False, True):
        with pytest.raises(ValueError):
            tpe.suggest_joint(ids, dom, trials, 21, batch='pending', n_configs=n,
                              n_startup_jobs=0, multivariate=mv)


def _cat_space(hp_):
    return {'a': hp_.choice('a', [0, 1, 2]), 'b': hp_.choice('b', [0, 1, 2, 3]),
            'c': hp_.randint('c', 5)}


def test_suggest_joint_pending_skips_history_rows(monkeypatch):
    """An all-categorical space: the draw repeats itself and the history, so
    the picks of the first run hold history rows and the selection is rerun
    under a mask; the result is the selection over the configurations that
    are not history rows."""
    dom = Domain(lambda c: 0.0, _cat_space(hp))
    cs = dom.space
    hist = rand.suggest(list(range(30)), dom, Trials(), 4)
    cfgs = _values(hist)
    trials = C.done(hist, [abs(c['a'] - 1) + abs(c['b'] - 2) + 0.3 * c['c'] for c in cfgs])
    _, losses, hv, ha = tpe.build_history(dom, trials)
    hps, conds, pprior = cs.engine_tables()
    plan = E.Plan(E.default_engine(), hps, conds, pprior, max_trials=30)
    plan.set_history(losses, hv, ha)
    plan.fit(gamma=C.GAMMA, prior_weight=C.PRIOR_WEIGHT)
    plan.group_fit()
    n, ids = 256, [30, 31, 32, 33, 34]
    kw = dict(n_configs=n, n_startup_jobs=0, multivariate='groups', batch='pending')
    vals, _ = plan.group_sample_points(tpe.batch_seeds(9, 1)[0], n)
    seen = tpe.seen_in_history(vals, ~np.isnan(vals), hv, ha)
    free, _ = plan.group_batch_points(vals, 5)
    assert seen[free].any()                 # (the rerun path is taken)
    want, _ = plan.group_batch_points(vals, 5, eligible=~seen)
    docs = tpe.suggest_joint(ids, dom, trials, 9, **kw)
    assert _values(docs) == _configs(cs, vals, want)
    assert len({tuple(sorted(c.items())) for c in _values(docs)}) == 5
    assert _values(tpe.suggest_joint(ids, dom, trials, 9, skip_seen=False, **kw)) == \
        _configs(cs, vals, free)
    # the full host mask gives the same picks
    monkeypatch.setattr(tpe, 'PENDING_RERUNS', 0)
    assert _values(tpe.suggest_joint(ids, dom, trials, 9, **kw)) == _values(docs)
    # with a predicate on top
    ok = vals[cs.labels.index('c')] >= 1
    fwant, _ = plan.group_batch_points(vals, 5, eligible=~seen & ok)
    fdocs = tpe.suggest_joint(ids, dom, trials, 9, feasible=lambda cols: cols['c'] >= 1, **kw)
    assert _values(fdocs) == _configs(cs, vals, fwant)
    # fewer selectable configurations than asked for
    with pytest.raises(ValueError):
        tpe.suggest_joint(ids, dom, trials, 9, feasible=lambda cols: np.arange(n) < 3, **kw)


def test_fmin_with_a_pending_queue():
    def loss(c):
        b = c['top']
        k = b['kind']
        return float((np.log(b['lr%d' % k]) + 3) ** 2 + 0.1 * b['zz%d' % k] ** 2 + c['aa'] + k)

    t = Trials()
    algo = functools.partial(tpe.suggest_joint, n_configs=512, n_startup_jobs=10,
                             multivariate='groups', batch='pending')
    fmin(loss, spaces.cond_space(hp), algo=algo, max_evals=30, max_queue_len=4, trials=t,
         rstate=np.random.RandomState(3))
    assert len(t) == 30 and np.isfinite(min(t.losses()))
