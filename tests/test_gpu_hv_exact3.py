"""Exact hypervolume gains for three objectives on the device (DESIGN 5.18,
method code 3): picks, keys, R and the whole surrogate column against
``hv3_oracle``, byte for byte; a re-used plan; the method through ``tpe.*``."""
import functools

import numpy as np
import pytest

import hyperopt_amd as H
from hyperopt_amd import fmin, hp, rand, tpe, Trials, trials_from_docs
from hyperopt_amd import _engine as E
from hyperopt_amd.base import Domain

import hv_cases
import hv3_oracle as H3
import spaces

pytestmark = pytest.mark.gpu

BIG = 65536 + 300
HUGE = (1e200, 1e200, 1e200)          # +inf areas, zero-thickness slabs


@pytest.fixture(scope='module')
def plan():
    dom = Domain(lambda x: 0.0, spaces.cond_space(hp))
    hps, conds, pprior = dom.space.engine_tables()
    p = E.Plan(E.default_engine(), hps, conds, pprior, max_trials=BIG)
    yield p
    p.set_hv(None)


@functools.lru_cache(maxsize=None)
def _matrix(n):
    """``hv_cases.make_case`` (duplicate rows, a row outside r, -inf, pending
    rows; at n = 600 a front above 256 rows) with per-objective ties:
    objectives 0 and 2 rounded to two decimals.  n = BIG: 1000 complete rows
    scattered among pending ones, so the row list spans blocks and gathers
    from many tiles."""
    rng = np.random.RandomState(n)
    m = 1000 if n == BIG else n
    Y, r = hv_cases.make_case(9000 + m, 3, m, frac_front=0.5)
    Y[0], Y[2] = np.round(Y[0], 2), np.round(Y[2], 2)
    if n == BIG:
        Z = np.full((3, n), np.nan)
        Z[:, np.sort(rng.choice(n, m, replace=False))] = Y
        Y = Z
    Y.setflags(write=False)
    return Y, tuple(r)


@functools.lru_cache(maxsize=None)
def _want(n, n_pick, r=None):
    Y, r0 = _matrix(n)
    return H3.hv3_rank(Y, r or r0, n_pick=n_pick)


def _rank(plan, Y, r, n_pick, method=H3.EXACT3):
    n = Y.shape[1]
    plan.set_history(np.zeros(n), np.zeros((plan.n_hp, n)), np.ones((plan.n_hp, n), dtype=np.uint8))
    plan.set_hv(r, n_pick=n_pick, method=method)
    plan.set_objectives(np.ascontiguousarray(Y))


def _assert_same(plan, n, want):
    by, of, s, picks, keys, counts, R = want
    gby, gof, gs = plan.pareto_get(n)
    gp, gk, gc, gR = plan.hv_get()
    assert gR == R
    np.testing.assert_array_equal(gp, picks)
    np.testing.assert_array_equal(gc, counts)           # -1: an exact path
    assert gk.tobytes() == keys.tobytes() and gs.tobytes() == s.tobytes()
    np.testing.assert_array_equal(gby, by)


@pytest.mark.parametrize('n_pick', [1, 5, 32, 256])
@pytest.mark.parametrize('n', [1, 3, 64, 65, 257, 600])
def test_selection_and_column_equal_the_oracle(plan, n, n_pick):
    Y, r = _matrix(n)
    want = _want(n, n_pick)
    _rank(plan, Y, r, n_pick)
    _assert_same(plan, n, want)
    if n == 600:
        assert want[6] == n_pick                        # a front larger than n_pick
    if n_pick == 256 and n < 600:
        assert 0 < want[6] < n_pick                     # a smaller one: an early end
    if n >= 64 and n_pick == 32:
        _rank(plan, Y, HUGE, n_pick)
        _assert_same(plan, n, _want(n, n_pick, HUGE))
        assert np.isinf(_want(n, n_pick, HUGE)[4][1])


def test_a_row_list_of_several_blocks(plan):
    Y, r = _matrix(BIG)
    want = _want(BIG, 32)
    part, _ = H3.HO.participants(Y, want[0], np.asarray(r))
    assert part.sum() > 256 and want[6] == 32
    _rank(plan, Y, r, 32)
    _assert_same(plan, BIG, want)


def test_a_reused_plan_and_the_method_codes(plan):
    Y, r = _matrix(257)
    _rank(plan, *_matrix(600), 32)
    _rank(plan, _matrix(65)[0], _matrix(65)[1], 5, method=H3.HO.MC)
    _rank(plan, Y, r, 32)
    _assert_same(plan, 257, _want(257, 32))
    ref = np.ones(4)
    with plan.engine.lock:
        call = plan.engine.lib.tpe_plan_set_hv
        assert call(plan.p, 1, ref.ctypes.data, 3, 32, 1024, 0, 3) == E.TPE_OK
        assert call(plan.p, 1, ref.ctypes.data, 4, 32, 1024, 0, 3) == E.TPE_E_INVALID
        assert call(plan.p, 1, ref.ctypes.data, 2, 32, 1024, 0, 3) == E.TPE_E_INVALID


def test_the_public_path():
    dom = Domain(lambda x: 0.0, spaces.cond_space(hp))
    n, ref = 120, (1.5, 2.0, 2.0)
    docs = rand.suggest(list(range(n)), dom, Trials(), 22)
    rng = np.random.RandomState(23)
    Y = rng.rand(3, n)
    Y[1:] = np.round(1.0 - Y[0] + 0.4 * Y[1:], 1)
    for i, d in enumerate(docs):
        d['state'] = H.JOB_STATE_DONE
        d['result'] = {'status': 'ok', 'loss': 0.0, 'objectives': [float(v) for v in Y[:, i]]}
    tr = trials_from_docs(docs)
    want = H3.hv3_rank(Y, ref)
    R = want[6]
    auto = tpe.hv_picks(dom, tr, 3, hypervolume=ref)
    tids, gains, alive = tpe.hv_picks(dom, tr, 3, hypervolume=ref, hv_method='exact')
    assert R > 5 and tids == [int(p) for p in want[3][:R]]
    assert gains.tobytes() == want[4][:R].tobytes() and (alive == -1).all()
    s = tpe.pareto_ranks(dom, tr, 3, hypervolume=ref, hv_method='exact')[3]
    assert s.tobytes() == want[2].tobytes()
    again = tpe.hv_picks(dom, tr, 3, hypervolume=ref, hv_method='auto')
    assert (again[2] > 0).all() and again[0] == auto[0]
    assert again[1].tobytes() == auto[1].tobytes()
    assert tpe.hv_picks(dom, tr, 3, hypervolume=ref, hv_method='mc')[0] == auto[0]

    def f(c):
        x, y = c['x'], c['y']
        return {'loss': x + y, 'status': 'ok', 'objectives': [x, (1 - x) ** 2 + y, y * y + 0.1 * x]}
    t = Trials()
    fmin(f, {'x': hp.uniform('x', 0, 1), 'y': hp.uniform('y', 0, 1)},
         algo=functools.partial(tpe.suggest, objectives=3, hypervolume=True, hv_method='exact'),
         max_evals=40, trials=t, rstate=np.random.RandomState(11))
    assert len(t.trials) == 40
