"""Multi-objective TPE on the device: the Pareto ranking pass against the numpy
oracle (exact: integers, and doubles bit for bit), its independence of the
launch shape, M = 1 as the scalar path, the layering under the fits, the
switching of ``objectives`` on one domain, ``pareto_front`` and the argument
errors of the two calls."""
import ctypes as C
import functools

import numpy as np
import pytest

import hyperopt_amd as H
from hyperopt_amd import fmin, hp, rand, tpe, Trials, trials_from_docs
from hyperopt_amd import _engine as E
from hyperopt_amd.base import Domain
from hyperopt_amd.expr import as_apply

import domains
import pareto_oracle as PO
import spaces

pytestmark = pytest.mark.gpu

CAP = 1024
VALUES = np.array([-1.0, 0.0, 0.5, 2.0, 7.0])


@pytest.fixture(scope='module')
def plan():
    dom = Domain(lambda x: 0.0, spaces.cond_space(hp))
    hps, conds, pprior = dom.space.engine_tables()
    return E.Plan(E.default_engine(), hps, conds, pprior, max_trials=CAP)


@pytest.fixture(scope='module')
def tile(plan):
    t, max_obj, _, _ = plan.pareto_shape(1, 1)
    assert max_obj == E.MAX_OBJ == 8
    return t


def _blank_history(plan, n):
    """n rows whose values do not matter (no fit follows)."""
    plan.set_history(np.zeros(n), np.zeros((plan.n_hp, n)),
                     np.ones((plan.n_hp, n), dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def _case(n, M):
    """(Y, the oracle's counts and s), computed once per shape.  Y is drawn
    from five values per objective; rows with -0.0 against +0.0, with -inf,
    and pending rows with NaN or +inf in one objective, where n has the room."""
    rng = np.random.RandomState(1000 * M + n)
    Y = rng.choice(VALUES, size=(M, n))
    if n >= 2:
        Y[M - 1, 1] = -0.0
    if n >= 8:
        Y[0, 2] = -np.inf
        Y[M - 1, 3] = np.nan
        Y[0, 4] = np.inf
        Y[:, 5] = Y[:, 6]                       # a duplicate row
        Y[0, n - 1] = np.nan                    # pending in the last (partial) tile
        Y[M - 1, n - 2] = -np.inf
    by, of, s = PO.pareto_rank(Y, fast=n > 300)
    for a in (Y, by, of, s):
        a.setflags(write=False)
    return Y, by, of, s


def _assert_same(got, want):
    by, of, s = got
    assert by.dtype == np.int32 and of.dtype == np.int32 and s.dtype == np.float64
    np.testing.assert_array_equal(by, want[0])
    np.testing.assert_array_equal(of, want[1])
    assert s.tobytes() == want[2].tobytes()     # bit for bit


def _sizes(tile):
    return [1, 2, tile - 1, tile, tile + 1, 2 * tile + 1, 1000]


# --------------------------------------------------- counts and s against the oracle
@pytest.mark.parametrize('M', [1, 2, 3, E.MAX_OBJ])
@pytest.mark.parametrize('which', range(7))
def test_counts_and_surrogate_equal_the_oracle(plan, tile, which, M):
    n = _sizes(tile)[which]
    Y, by, of, s = _case(n, M)
    _blank_history(plan, n)
    plan.set_objectives(np.ascontiguousarray(Y))
    _assert_same(plan.pareto_get(n), (by, of, s))
    if n >= 8:
        assert np.isinf(s[[3, 4, n - 1]]).all() and np.isfinite(s[[1, 2, 5, 6, n - 2]]).all()
        assert s[5] == s[6]


def test_incremental_rows_and_leading_dimension(plan, tile):
    """Rows [obj0, n) from a wider host matrix on top of the rows already on
    the device give the counts of the whole matrix."""
    n, M = 2 * tile + 1, 3
    Y, by, of, s = _case(n, M)
    wide = np.full((M, n + 37), 123.0)
    wide[:, :n] = Y
    m = tile + 5
    _blank_history(plan, m)
    plan.set_objectives(wide, n=m)
    _assert_same(plan.pareto_get(m), PO.pareto_rank(Y[:, :m]))
    _blank_history(plan, n)
    plan.set_objectives(wide, n=n, obj0=m)
    _assert_same(plan.pareto_get(n), (by, of, s))
    plan.set_objectives(wide, n=n, obj0=n)              # nothing new: the same again
    _assert_same(plan.pareto_get(n), (by, of, s))


# ---------------------------------------------------------------- launch shape
@pytest.mark.parametrize('M', [2, E.MAX_OBJ])
@pytest.mark.parametrize('which', [6, 5, 4])
def test_every_j_split_gives_the_same_arrays(plan, tile, which, M):
    n = _sizes(tile)[which]                             # 4, 3 and 2 tiles
    Y, by, of, s = _case(n, M)
    tiles = -(-n // tile)
    _blank_history(plan, n)
    seen = set()
    try:
        for force in range(1, tiles + 1):
            _, _, splits, t = plan.pareto_shape(n, M, force)
            assert t == tiles and 1 <= splits <= force
            if splits in seen:
                continue
            seen.add(splits)
            plan.set_objectives(np.ascontiguousarray(Y))
            _assert_same(plan.pareto_get(n), (by, of, s))
    finally:
        default = plan.pareto_shape(n, M, 0)[2]
    assert 1 in seen and tiles in seen and default in seen


# ------------------------------------------------------------ M = 1 is the scalar path
def _docs(t):
    return [(d['tid'], d['state'], d['misc']['idxs'], d['misc']['vals'], d['result']['loss'],
             d['result']['status']) for d in t.trials]


def _with_objectives(fn):
    def wrapped(x):
        r = fn(x)
        r = dict(r) if isinstance(r, dict) else {'loss': float(r), 'status': 'ok'}
        r['objectives'] = [r['loss']]
        return r
    return wrapped


def _both(fn, make_space, algo, algo1, max_evals, **kw):
    runs = []
    for f, a in ((fn, algo), (_with_objectives(fn), algo1)):
        t = Trials()
        fmin(f, make_space(), algo=a, max_evals=max_evals, trials=t,
             rstate=np.random.RandomState(5), **kw)
        runs.append(t)
    return runs


def test_one_objective_fmin_with_tied_losses_is_the_scalar_fmin():
    a, b = _both(lambda x: round((x - 1.0) ** 2, 1), lambda: hp.uniform('x', -5, 5),
                 tpe.suggest, functools.partial(tpe.suggest, objectives=1), 60)
    assert len(a) == len(b) == 60
    assert len(set(a.losses())) < 60                    # ties occurred
    assert _docs(a) == _docs(b)
    assert all(d['result']['objectives'] == [d['result']['loss']] for d in b.trials)


def test_one_objective_fmin_on_a_conditional_space_is_the_scalar_fmin():
    make = lambda: domains.build('gauss_wave2', hp, H.scope, as_apply)      # noqa: E731
    a, b = _both(lambda r: r, make, tpe.suggest, functools.partial(tpe.suggest, objectives=1),
                 60)
    assert len(a) == 60 and _docs(a) == _docs(b)
    assert any(d['misc']['vals']['amp'] == [] for d in a.trials)        # (conditional)


def test_one_objective_pending_batch_is_the_scalar_one():
    def loss(c):
        b = c['top']
        k = b['kind']
        return float((np.log(b['lr%d' % k]) + 3) ** 2 + 0.1 * b['zz%d' % k] ** 2 + c['aa'] + k)

    kw = dict(n_configs=512, n_startup_jobs=10, multivariate='groups', batch='pending')
    a, b = _both(loss, lambda: spaces.cond_space(hp),
                 functools.partial(tpe.suggest_joint, **kw),
                 functools.partial(tpe.suggest_joint, objectives=1, **kw), 40, max_queue_len=4)
    assert len(a) == 40 and _docs(a) == _docs(b)


# -------------------------------------------------------------------- layering
def _history(n, seed, M):
    """(domain factory, docs with loss and M objectives, Y[M, n])."""
    dom = Domain(lambda x: 0.0, spaces.cond_space(hp))
    docs = rand.suggest(list(range(n)), dom, Trials(), seed)
    rng = np.random.RandomState(seed + 1)
    # a trade-off between the objectives (a front of many rows), rounded:
    # ties and partial ties
    Y = rng.rand(M, n)
    Y[1:] = 1.0 - Y[0] + 0.4 * Y[1:]
    Y = np.round(Y, 1)
    for i, d in enumerate(docs):
        d['state'] = H.JOB_STATE_DONE
        d['result'] = {'status': 'ok', 'loss': float(rng.rand()),
                       'objectives': [float(v) for v in Y[:, i]]}
    return docs, Y


def _copy_docs(docs, loss=None, drop_objectives=False):
    out = []
    for i, d in enumerate(docs):
        c = dict(d)
        c['misc'] = dict(d['misc'])
        c['result'] = dict(d['result'])
        if loss is not None:
            c['result']['loss'] = float(loss[i])
        if drop_objectives:
            c['result'].pop('objectives', None)
        out.append(c)
    return out


@pytest.fixture(scope='module')
def layered():
    docs, Y = _history(200, 21, 2)
    by, of, s = PO.pareto_rank(Y, fast=True)
    assert len(set(s)) < 200 and (by == 0).sum() > 1
    return docs, Y, s


def _new_plan(dom, cap=256):
    hps, conds, pprior = dom.space.engine_tables()
    return E.Plan(E.default_engine(), hps, conds, pprior, max_trials=cap)


def test_mixtures_equal_those_of_the_surrogate_as_a_loss(layered):
    docs, Y, s = layered
    dom = Domain(lambda x: 0.0, spaces.cond_space(hp))
    _, losses, vals, act = tpe.build_history(dom, trials_from_docs(_copy_docs(docs)))
    a, b = _new_plan(dom), _new_plan(dom)
    # a: all but the last row, then the last row with its loss as a deferred
    # patch -- set_objectives must land after it
    a.set_history(losses[:199], np.ascontiguousarray(vals[:, :199]),
                  np.ascontiguousarray(act[:, :199]))
    a.update_history(200, 199, vals, act, 200, 199, losses)
    a.set_objectives(np.ascontiguousarray(Y))
    assert a.pareto_get(200)[2].tobytes() == s.tobytes()
    a.fit()
    b.set_history(s, vals, act)
    b.fit()
    for i in range(a.n_hp):
        for side in (0, 1):
            for x, y in zip(a.mixture(i, side), b.mixture(i, side)):
                assert x.tobytes() == y.tobytes(), (i, side)


def test_group_scores_equal_those_of_the_surrogate_as_a_loss(layered):
    docs, Y, s = layered
    cfgs = [{lab: v[0] for lab, v in d['misc']['vals'].items() if v} for d in docs[:40]]
    dom_a = Domain(lambda x: 0.0, spaces.cond_space(hp))
    dom_b = Domain(lambda x: 0.0, spaces.cond_space(hp))
    got = tpe.score_configs(cfgs, dom_a, trials_from_docs(_copy_docs(docs)),
                            multivariate='groups', objectives=2)
    want = tpe.score_configs(cfgs, dom_b,
                             trials_from_docs(_copy_docs(docs, loss=s, drop_objectives=True)),
                             multivariate='groups')
    assert got.tobytes() == want.tobytes()
    assert np.isfinite(got).all()


# ----------------------------------------------------------------------- state
def _fresh(docs, cfgs, objectives, ids, seed=9):
    dom = Domain(lambda x: 0.0, spaces.cond_space(hp))
    tr = trials_from_docs(_copy_docs(docs))
    return _calls(dom, tr, cfgs, objectives, ids, seed)


def _calls(dom, tr, cfgs, objectives, ids, seed=9):
    sc = tpe.score_configs(cfgs, dom, tr, objectives=objectives)
    doc = tpe.suggest(ids, dom, tr, seed, objectives=objectives)[0]
    return sc.tobytes(), doc['misc']['vals']


def test_objectives_may_alternate_on_one_domain(layered):
    docs, Y, s = layered
    cfgs = [{lab: v[0] for lab, v in d['misc']['vals'].items() if v} for d in docs[:16]]
    dom = Domain(lambda x: 0.0, spaces.cond_space(hp))
    tr = trials_from_docs(_copy_docs(docs[:150]))
    f2 = _fresh(docs[:150], cfgs, 2, [150])
    f0 = _fresh(docs[:150], cfgs, None, [150])
    assert f2 != f0                                     # (the two modes do differ)
    assert _calls(dom, tr, cfgs, 2, [150]) == f2
    assert _calls(dom, tr, cfgs, None, [150]) == f0     # the scalar column is restored
    assert _calls(dom, tr, cfgs, 2, [150]) == f2
    # more trials, one of them still running: the incremental path is a fresh upload
    more = _copy_docs(docs[150:170])
    more[7]['state'] = H.JOB_STATE_RUNNING
    more[7]['result'] = {'status': 'new'}
    tr.insert_trial_docs(more)
    tr.refresh()
    all_docs = _copy_docs(docs[:150]) + more
    assert _calls(dom, tr, cfgs, 2, [170]) == _fresh(all_docs, cfgs, 2, [170])
    assert _calls(dom, tr, cfgs, None, [170]) == _fresh(all_docs, cfgs, None, [170])
    # the running trial finishes: its row changes in place
    done = tr.trials[157]
    done['state'] = H.JOB_STATE_DONE
    done['result'] = dict(docs[157]['result'])
    tr.refresh()
    all_docs[157] = _copy_docs([docs[157]])[0]
    assert _calls(dom, tr, cfgs, 2, [170]) == _fresh(all_docs, cfgs, 2, [170])


# --------------------------------------------------------------- pareto_front
def test_pareto_front_is_the_oracles_nondominated_set(layered):
    docs, Y, s = layered
    work = _copy_docs(docs)
    work[3]['result'] = {'status': 'fail'}              # no objectives: pending
    work[5]['result']['objectives'] = [float(Y[0, 5]), float('nan')]    # pending too
    Yw = Y.copy()
    Yw[:, 3] = np.nan
    Yw[1, 5] = np.nan
    dom = Domain(lambda x: 0.0, spaces.cond_space(hp))
    tr = trials_from_docs(work)
    by, of, sw = PO.pareto_rank(Yw, fast=True)
    tids, gby, gof, gs = tpe.pareto_ranks(dom, tr, 2)
    assert tids == list(range(200))
    _assert_same((gby, gof, gs), (by, of, sw))
    front = tpe.pareto_front(dom, tr, 2)
    want = [int(i) for i in np.flatnonzero((by == 0) & np.isfinite(sw))]
    assert [d['tid'] for d in front] == want
    assert 3 not in want and 5 not in want and len(want) > 1
    assert all(d is tr.trials[d['tid']] for d in front)


# ---------------------------------------------------------------------- errors
def test_set_objectives_argument_errors(plan):
    lib = plan.engine.lib
    n = 10
    _blank_history(plan, n)
    Y = np.zeros((E.MAX_OBJ + 1, n))
    ptr = Y.ctypes.data

    def call(y, n_obj, nn, ld, obj0):
        with plan.engine.lock:
            return lib.tpe_plan_set_objectives(plan.p, y, n_obj, nn, ld, obj0, 0, None)

    assert call(ptr, 2, n, n, 0) == E.TPE_OK
    assert call(ptr, 0, n, n, 0) == E.TPE_E_INVALID                 # n_obj outside [1, 8]
    assert call(ptr, E.MAX_OBJ + 1, n, n, 0) == E.TPE_E_INVALID
    assert call(ptr, -1, n, n, 0) == E.TPE_E_INVALID
    assert call(ptr, 2, n - 1, n, 0) == E.TPE_E_INVALID             # n is not the history length
    assert call(ptr, 2, n + 1, n + 1, 0) == E.TPE_E_INVALID
    assert call(ptr, 2, n, n - 1, 0) == E.TPE_E_INVALID             # ld too small
    assert call(ptr, 2, n, 5, 4) == E.TPE_E_INVALID
    assert call(ptr, 2, n, 6, 4) == E.TPE_OK
    assert call(None, 2, n, n, 0) == E.TPE_E_INVALID                # a null Y
    assert call(ptr, 2, n, n, -1) == E.TPE_E_INVALID                # obj0 outside [0, n]
    assert call(ptr, 2, n, n, n + 1) == E.TPE_E_INVALID
    assert call(ptr, 3, n, n, 4) == E.TPE_E_INVALID                 # rows below obj0 have another M
    with pytest.raises(ValueError):
        plan.set_objectives(np.zeros((E.MAX_OBJ + 1, n)))
    # pareto_get: only the n of the last ranking
    assert call(ptr, 2, n, n, 0) == E.TPE_OK
    with pytest.raises(ValueError):
        plan.pareto_get(n - 1)
    assert len(plan.pareto_get(n)[0]) == n
    with pytest.raises(ValueError):
        plan.pareto_shape(0, 2)
    with pytest.raises(ValueError):
        plan.pareto_shape(10, E.MAX_OBJ + 1)


def test_set_objectives_invalidates_the_fits(plan):
    docs, Y = _history(64, 33, 2)
    dom = Domain(lambda x: 0.0, spaces.cond_space(hp))
    _, losses, vals, act = tpe.build_history(dom, trials_from_docs(docs))
    plan.set_history(losses, vals, act)
    plan.fit()
    plan.group_fit()
    plan.set_objectives(np.ascontiguousarray(Y))
    cfg = np.ascontiguousarray(vals[:, :4])
    with pytest.raises(ValueError):
        plan.score_points(cfg)
    with pytest.raises(ValueError):
        plan.group_score_points(cfg)
    plan.fit()
    plan.group_fit()
    assert np.isfinite(plan.group_score_points(cfg)).all()
