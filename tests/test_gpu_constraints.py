"""Constrained TPE on the device against the numpy oracle, byte
for byte: no tolerance anywhere."""
import functools

import numpy as np
import pytest

from hyperopt_amd import fmin, hp, tpe, Trials
from hyperopt_amd import _engine as E
from hyperopt_amd.base import Domain

import constraint_oracle as CO
import hv_oracle as HO
import pareto_oracle as PO
import spaces

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def plan():
    dom = Domain(lambda x: 0.0, spaces.cond_space(hp))
    hps, conds, pprior = dom.space.engine_tables()
    return E.Plan(E.default_engine(), hps, conds, pprior, max_trials=1024)


def _blank_history(plan, n):
    plan.set_history(np.zeros(n), np.zeros((plan.n_hp, n)),
                     np.ones((plan.n_hp, n), dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def _case(n, M, C, feasible=None):
    """(Y, G, the oracle's v, counts and s), computed once per shape."""
    Y, G = CO.history(n, M, C, feasible)
    return (Y, G) + CO.constraint_rank(Y, G)


def _assert_same(plan, n, want):
    v, by, of, s = want
    gby, gof, gs = plan.pareto_get(n)
    assert plan.constraint_get(n).tobytes() == v.tobytes()
    np.testing.assert_array_equal(gby, by)
    np.testing.assert_array_equal(gof, of)
    assert gs.tobytes() == s.tobytes()


@pytest.mark.parametrize('feasible', [None, True, False])
@pytest.mark.parametrize('n', [1, 255, 256, 257, 700])
@pytest.mark.parametrize('C', [1, 3, 16])
@pytest.mark.parametrize('M', [1, 2, 3, 8])
def test_violation_counts_and_surrogate_equal_the_oracle(plan, M, C, n, feasible):
    Y, G, *want = _case(n, M, C, feasible)
    _blank_history(plan, n)
    seen = set()
    try:
        for force in range(0, 4 if n == 700 else 1):    # 700 rows: every j-split count
            splits = plan.pareto_shape(n, M, force)[2]
            if splits not in seen:
                seen.add(splits)
                plan.set_constraints(G)
                plan.set_objectives(Y)
                _assert_same(plan, n, want)
    finally:
        plan.pareto_shape(n, M, 0)
        plan.set_constraints(None)
    assert seen == {1, 2, 3} if n == 700 else len(seen) == 1


@pytest.mark.parametrize('M', [1, 3])
def test_all_feasible_is_the_plain_ranking_and_off_is_off(plan, M):
    n = 700
    Y, G, *_ = _case(n, M, 3, True)
    mixed = _case(n, M, 3)
    _blank_history(plan, n)
    plan.set_objectives(Y)
    plain = plan.pareto_get(n)
    plan.set_constraints(G)
    plan.set_objectives(Y)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(plan.pareto_get(n), plain))
    plan.set_constraints(mixed[1])                      # (the mode does change the column)
    plan.set_objectives(Y)
    assert plan.pareto_get(n)[2].tobytes() == mixed[5].tobytes() != plain[2].tobytes()
    plan.set_constraints(None)                          # n_con = 0: the plain ranking again
    plan.set_objectives(Y)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(plan.pareto_get(n), plain))
    with pytest.raises(ValueError):
        plan.constraint_get(n)                          # that ranking had no violations


def test_appended_rows_give_the_arrays_of_one_upload(plan):
    n, m, M, C = 700, 300, 2, 3
    Y, G, *want = _case(n, M, C)
    wide = np.full((C, n + 11), 9.0)
    wide[:, :n] = G
    try:
        _blank_history(plan, m)
        plan.set_constraints(wide, n=m)
        plan.set_objectives(Y, n=m)
        _assert_same(plan, m, CO.constraint_rank(Y[:, :m], G[:, :m]))
        _blank_history(plan, n)
        plan.set_constraints(wide, n=n, con0=m)
        plan.set_objectives(Y, n=n, obj0=m)
        _assert_same(plan, n, want)
    finally:
        plan.set_constraints(None)


def _run(fn, space, algo):
    t = Trials()
    fmin(fn, space, algo=algo, max_evals=40, trials=t, rstate=np.random.RandomState(5))
    return t, [(d['tid'], d['misc']['vals'], d['result']['loss']) for d in t.trials]


def test_always_feasible_fmin_with_tied_losses_is_the_scalar_fmin():
    loss = lambda x: round((x - 1.0) ** 2, 1)           # noqa: E731
    a, da = _run(loss, hp.uniform('x', -5, 5), tpe.suggest)
    b, db = _run(lambda x: {'status': 'ok', 'loss': loss(x), 'constraints': [-1.0 - abs(x)]},
                 hp.uniform('x', -5, 5), functools.partial(tpe.suggest, constraints=1))
    assert len(a) == len(b) == 40 and len(set(a.losses())) < 40 and da == db


def test_a_constraint_that_cuts_off_the_optimum_and_constraint_ranks():
    space = {'x': hp.uniform('x', -2, 2), 'y': hp.uniform('y', -2, 2)}

    def fn(c):                                          # the optimum (-2, -2) is infeasible
        return {'status': 'ok', 'loss': round(c['x'] + c['y'], 1),
                'constraints': [round(-1.0 - c['x'] - c['y'], 1)]}

    t, dt = _run(fn, space, functools.partial(tpe.suggest, constraints=1))
    assert dt != _run(fn, space, tpe.suggest)[1]        # the constraint steers the search
    dom = Domain(fn, space)
    Y = np.array([[d['result']['loss'] for d in t.trials]])
    G = np.array([[d['result']['constraints'][0] for d in t.trials]])
    v, by, of, s = CO.constraint_rank(Y, G)
    tids, gv, feas, gby, gof, gs = tpe.constraint_ranks(dom, t, 1)
    assert tids == list(range(40)) and 0 < feas.sum() < 40
    assert gv.tobytes() == v.tobytes() and (feas == (v == 0)).all()
    assert (gby == by).all() and (gof == of).all() and gs.tobytes() == s.tobytes()
    front = tpe.pareto_front(dom, t, constraints=1)
    assert [d['tid'] for d in front] == [int(i) for i in np.flatnonzero((by == 0) & (v == 0))]


def test_hypervolume_selection_runs_on_the_c_dominance_counts(plan):
    n = 257
    rng = np.random.default_rng(77)
    Y = np.round(rng.random((2, n)), 2)
    Y[1] = np.round(1.0 - Y[0] + 0.3 * Y[1], 2)          # a trade-off: a wide front
    G = rng.choice([-1.0, -1.0, 0.5, 2.0], size=(1, n))
    pb = PO.pareto_rank(Y, fast=True)[0]
    assert ((pb == 0) & (G[0] > 0)).any() and ((pb == 0) & (G[0] <= 0)).any()
    v, by, of, s = CO.constraint_rank(Y, G)
    ref = (1.5, 1.5)
    picks, keys, counts, R = HO.hv_select(Y, by, ref, method=HO.EXACT)
    want = HO.hv_surrogate(by, of, PO.complete_rows(Y), picks, R)
    assert R > 1 and (v[picks[:R]] == 0).all()          # the feasible front is ordered
    _blank_history(plan, n)
    try:
        plan.set_hv(ref, method=1)
        plan.set_constraints(G)
        plan.set_objectives(Y)
        gby, gof, gs = plan.pareto_get(n)
        gp, gk, gc, gR = plan.hv_get(32)
    finally:
        plan.set_hv(None)
        plan.set_constraints(None)
    assert (gby == by).all() and (gof == of).all() and gs.tobytes() == want.tobytes()
    assert gR == R and (gp == picks).all() and gk.tobytes() == keys.tobytes()


N = 10
BAD = {'n_con < 0': (1, -1, N, N, 0), 'n_con > 16': (1, 17, N, N, 0),
       'n short': (1, 2, N - 1, N, 0), 'n long': (1, 2, N + 1, N + 1, 0),
       'con0 < 0': (1, 2, N, N, -1), 'con0 > n': (1, 2, N, N, N + 1),
       'another n_con below con0': (1, 3, N, N, 4), 'ld short': (1, 2, N, 5, 4),
       'null G': (0, 2, N, N, 0), 'con0 above the rows held': (1, 2, 16, 16, 12)}
GROW = ['con0 above the rows held', 'objectives over more rows']     # the history grows to 16


@pytest.mark.parametrize('case', sorted(set(BAD) | set(GROW)))
def test_set_constraints_argument_errors_leave_the_column(plan, case):
    lib = plan.engine.lib
    Y, G, *_ = _case(16, 2, 3)
    G2 = np.ascontiguousarray(G[:2, :N])
    try:
        _blank_history(plan, N)
        plan.set_constraints(G2)
        plan.set_objectives(np.ascontiguousarray(Y[:, :N]))
        calls = []
        if case in BAD:
            ptr, n_con, nn, ld, con0 = BAD[case]
            calls.append(lambda: lib.tpe_plan_set_constraints(
                plan.p, G2.ctypes.data if ptr else None, n_con, nn, ld, con0, 0, None))
        if case in GROW:                                # the store still holds 10 rows after
            _blank_history(plan, 16)
            calls.append(lambda: lib.tpe_plan_set_objectives(
                plan.p, Y.ctypes.data, 2, 16, 16, 0, 0, None))
        before = plan.pareto_get(N)[2]
        with plan.engine.lock:
            assert [call() for call in calls] == [E.TPE_E_INVALID] * len(calls)
        assert plan.pareto_get(N)[2].tobytes() == before.tobytes()
    finally:
        plan.set_constraints(None)
