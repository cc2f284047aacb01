"""Host side of multi-objective TPE (no GPU): the ranking rule as the numpy
oracle states it, the launch plan of the device pass (a stand-alone sanitized
program), the ``objectives=`` argument checks, and the objective store of
``TrialHistory`` with the order in which ``push`` talks to a plan."""
import math
import os
import subprocess

import numpy as np
import pytest

import hyperopt_amd as H
from hyperopt_amd import hp, rand, tpe, Trials, trials_from_docs
from hyperopt_amd.base import Domain
from hyperopt_amd.history import TrialHistory

import pareto_oracle as PO
import spaces

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


# ------------------------------------------------------------------- the rule
def _tied_matrix(rng, M, n):
    """Y[M, n] from five values per objective: ties, duplicate rows and partial
    ties everywhere."""
    return rng.choice(np.array([-1.0, 0.0, 0.5, 2.0, 7.0]), size=(M, n))


@pytest.mark.parametrize('M', [1, 2, 3, 8])
def test_dominance_implies_a_smaller_surrogate(M):
    rng = np.random.RandomState(10 + M)
    Y = _tied_matrix(rng, M, 60)
    by, of, s = PO.pareto_rank(Y)
    pairs = 0
    for a in range(60):
        for b in range(60):
            if PO.dominates(Y[:, a], Y[:, b]):
                assert s[a] < s[b], (a, b)
                pairs += 1
    assert pairs > 0
    assert (s == np.floor(s)).all()                     # exact integers
    fb, ff, fs = PO.pareto_rank(Y, fast=True)           # the vectorised form is the same rule
    assert (fb == by).all() and (ff == of).all() and (fs == s).all()


@pytest.mark.parametrize('M', [2, 3])
def test_rank_zero_is_the_brute_force_nondominated_set(M):
    rng = np.random.RandomState(20 + M)
    Y = _tied_matrix(rng, M, 50)
    by, _, _ = PO.pareto_rank(Y)
    front = [i for i in range(50)
             if not any((Y[:, j] <= Y[:, i]).all() and (Y[:, j] < Y[:, i]).any()
                        for j in range(50))]
    assert sorted(np.flatnonzero(by == 0)) == front
    assert 0 < len(front) < 50


def test_one_objective_sorts_as_the_loss():
    rng = np.random.RandomState(3)
    loss = rng.permutation(40).astype(np.float64) * 0.37 - 5.0       # distinct
    _, _, s = PO.pareto_rank(loss[None, :])
    assert (np.argsort(s, kind='stable') == np.argsort(loss, kind='stable')).all()
    assert len(set(s)) == 40
    tied = np.round(rng.rand(40), 1)                                   # ties
    assert len(set(tied)) < 40
    _, _, s = PO.pareto_rank(tied[None, :])
    for a in range(40):
        for b in range(40):
            assert (s[a] == s[b]) == (tied[a] == tied[b])
            assert (s[a] < s[b]) == (tied[a] < tied[b])


def test_pending_rows_get_inf_and_take_no_part():
    rng = np.random.RandomState(4)
    Y = _tied_matrix(rng, 2, 30)
    Y[0, 3] = np.nan
    Y[1, 7] = np.inf
    Y[:, 11] = np.nan
    Y[0, 13] = -np.inf                                   # an ordinary value
    Y[1, 17] = -0.0                                      # equal to the +0.0 rows
    by, of, s = PO.pareto_rank(Y)
    pend = [3, 7, 11]
    assert np.isinf(s[pend]).all() and (by[pend] == 0).all() and (of[pend] == 0).all()
    assert np.isfinite(np.delete(s, pend)).all()
    keep = np.setdiff1d(np.arange(30), pend)
    kb, kf, _ = PO.pareto_rank(Y[:, keep])                # the counts of the rest alone
    assert (by[keep] == kb).all() and (of[keep] == kf).all()
    assert of[13] > 0                                    # -inf dominates
    z = np.array([[0.0, -0.0], [1.0, 1.0]])              # -0.0 == +0.0: neither dominates
    zb, zf, zs = PO.pareto_rank(z)
    assert (zb == 0).all() and (zf == 0).all() and zs[0] == zs[1]


def hand_built_front():
    """32 rows, two objectives: rows 0..7 on the line y1 = 1 - y0; 12 rows that
    only front row 3 dominates, 8 under front row 4, 4 under front row 7."""
    y0 = [i / 8.0 for i in range(8)]
    y1 = [1.0 - v for v in y0]
    for k in range(12):
        y0.append(0.375 + 0.01 * (k + 1)); y1.append(0.625 + 0.01 * (k + 1))
    for k in range(8):
        y0.append(0.5 + 0.01 * (k + 1)); y1.append(0.5 + 0.01 * (k + 1))
    for k in range(4):
        y0.append(0.9 + 0.01 * k); y1.append(0.2 + 0.01 * k)
    return np.array([y0, y1])


def test_the_good_side_of_a_front_is_not_the_best_of_one_objective():
    Y = hand_built_front()
    assert Y.shape == (2, 32)
    by, of, s = PO.pareto_rank(Y)
    assert sorted(np.flatnonzero(by == 0)) == list(range(8))
    assert (by[8:] > 0).all()
    assert of[:8].tolist() == [0, 0, 0, 12, 8, 0, 0, 4]
    n_below = int(math.ceil(0.25 * math.sqrt(32)))
    assert n_below == 2
    by_s = sorted(np.argsort(s, kind='stable')[:n_below].tolist())
    by_y0 = sorted(np.argsort(Y[0], kind='stable')[:n_below].tolist())
    assert by_s == [3, 4]                # the front rows that dominate the most trials
    assert by_y0 == [0, 1]               # the best of objective 0 alone
    assert s[3] == 32 - 12 and s[4] == 32 - 8


# ------------------------------------------------------------ the launch plan
def test_pareto_plan_host_checks(tmp_path):
    """The launch plan of the ranking pass (tpe_pareto_plan.hpp): tiles and
    j-splits cover their ranges exactly once, LDS within the limit, at n = 1,
    tile - 1, tile, tile + 1 and the largest n; host-only, address and
    undefined-behaviour sanitizers, a stand-alone program."""
    if not os.path.exists(HIPCC):
        pytest.fail('hipcc not found at %s' % HIPCC)
    exe = str(tmp_path / 'pareto_plan_check')
    src = os.path.join(ROOT, 'tests', 'host', 'pareto_plan_check.cpp')
    cc = subprocess.run(
        [HIPCC, '-x', 'hip', '--cuda-host-only', '-std=c++17', '-O1', '-g', '-Wall',
         '-Xarch_host', '-fsanitize=address,undefined',
         '-Xarch_host', '-fno-sanitize-recover=undefined', src, '-o', exe],
        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert cc.returncode == 0, cc.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       universal_newlines=True)
    assert r.returncode == 0, r.stdout


# ------------------------------------------------------- the objectives= argument
def _trials(dom, n, seed, objectives=None, extra=0):
    """n ok trials (+ ``extra`` new ones) with rand.suggest's values."""
    docs = rand.suggest(list(range(n + extra)), dom, Trials(), seed)
    rng = np.random.RandomState(seed + 1)
    for d in docs[:n]:
        d['state'] = H.JOB_STATE_DONE
        d['result'] = {'status': 'ok', 'loss': float(rng.rand())}
        if objectives:
            d['result']['objectives'] = [float(v) for v in rng.rand(objectives)]
    return trials_from_docs(docs)


@pytest.fixture
def dom():
    return Domain(lambda x: 0.0, spaces.cond_space(hp))


@pytest.mark.parametrize('bad', [0, -1, 9, 2.0, True, 'two'])
def test_objectives_must_be_a_count(dom, bad):
    tr = _trials(dom, 3, 1, objectives=2)
    for call in (lambda: tpe.suggest([3], dom, tr, 0, objectives=bad),
                 lambda: tpe.suggest_from_pool([3], dom, tr, 0, pool=[{}], objectives=bad),
                 lambda: tpe.suggest_joint([3], dom, tr, 0, objectives=bad),
                 lambda: tpe.score_configs([{}], dom, tr, objectives=bad),
                 lambda: tpe.sample_configs(4, dom, tr, 0, objectives=bad),
                 lambda: tpe.pareto_ranks(dom, tr, bad),
                 lambda: tpe.pareto_front(dom, tr, bad)):
        with pytest.raises(ValueError, match='objectives'):
            call()


def test_an_ok_trial_without_objectives_is_named(dom):
    tr = _trials(dom, 4, 2, objectives=2)
    del tr.trials[2]['result']['objectives']
    with pytest.raises(ValueError, match=r"trial 2: result\['objectives'\]"):
        tpe.suggest([4], dom, tr, 0, objectives=2)


def test_an_ok_trial_with_another_length_is_named(dom):
    tr = _trials(dom, 4, 3, objectives=3)
    with pytest.raises(ValueError, match=r'trial 0: .*sequence of 2 numbers'):
        tpe.suggest([4], dom, tr, 0, objectives=2)
    tr.trials[1]['result']['objectives'] = 0.5                      # not a sequence
    with pytest.raises(ValueError, match=r'trial 1: '):
        tpe.suggest_joint([4], dom, tr, 0, objectives=3)


def test_startup_without_objectives_in_new_trials(dom):
    """New and running trials report nothing yet: they are pending rows, and a
    startup call with objectives= is rand.suggest as without."""
    tr = _trials(dom, 3, 4, objectives=2, extra=2)
    a = tpe.suggest([5], dom, tr, 7, objectives=2)
    b = tpe.suggest([5], dom, tr, 7)
    assert a[0]['misc']['vals'] == b[0]['misc']['vals']
    h = tpe._state(dom).history(dom, tr).sync(tr, 2)
    assert h.n == 5 and np.isnan(h.Y[:, 3:5]).all() and np.isfinite(h.Y[:, :3]).all()


# -------------------------------------------------------- the objective store
def _append(tr, dom, n_new, seed, M):
    ids = tr.new_trial_ids(n_new)
    docs = rand.suggest(ids, dom, tr, seed)
    rng = np.random.RandomState(seed + 5)
    for d in docs:
        d['state'] = H.JOB_STATE_DONE
        d['result'] = {'status': 'ok', 'loss': float(rng.rand()),
                       'objectives': [float(v) for v in rng.rand(M)]}
    tr.insert_trial_docs(docs)
    tr.refresh()


def test_incremental_objective_store_equals_a_fresh_one(dom):
    tr = _trials(dom, 70, 5, objectives=3)
    h = TrialHistory(dom).sync(tr, 3)
    assert h.Y.shape[0] == 3 and h.n == 70
    _append(tr, dom, 9, 6, 3)                   # crosses the 64-row capacity
    h.sync(tr, 3)
    fresh = TrialHistory(dom).sync(tr, 3)
    assert h.n == fresh.n == 79
    assert np.array_equal(h.Y[:, :79], fresh.Y[:, :79])
    want = np.array([d['result']['objectives'] for d in tr.trials]).T
    assert np.array_equal(h.Y[:, :79], want)
    # a call without objectives in between, then another M: both re-read every row
    h.sync(tr)
    assert h.M is None
    for d in tr.trials:
        d['result']['objectives'] = d['result']['objectives'][:2]
    h.sync(tr, 2)
    assert np.array_equal(h.Y[:, :79], want[:2])


class _StubPlan(object):
    """Records what ``push`` sends (no engine)."""

    def __init__(self):
        self.calls = []

    def update_history(self, n, row0, vals, active, ld, loss0, losses, stream=None):
        self.calls.append(('update', n, row0, loss0))

    def set_objectives(self, Y, n=None, obj0=0, stream=None):
        self.calls.append(('objectives', Y.shape[0], n, obj0, Y[:, :n].copy()))


def test_push_sends_no_loss_under_objectives_and_every_loss_after(dom):
    tr = _trials(dom, 30, 8, objectives=2)
    h = TrialHistory(dom)
    plan = _StubPlan()
    h.sync(tr, 2).push(plan)
    # the rows without a loss (loss0 = n), then the whole objective matrix
    assert plan.calls[0] == ('update', 30, 0, 30)
    assert plan.calls[1][:4] == ('objectives', 2, 30, 0)
    _append(tr, dom, 2, 9, 2)
    plan.calls = []
    h.sync(tr, 2).push(plan)
    assert plan.calls[0] == ('update', 32, 30, 32)
    assert plan.calls[1][:4] == ('objectives', 2, 32, 30)          # only the new rows travel
    assert np.array_equal(plan.calls[1][4], TrialHistory(dom).sync(tr, 2).Y[:, :32])
    # back to the scalar loss: the column held a ranking, so every loss goes again
    plan.calls = []
    h.sync(tr).push(plan)
    assert plan.calls == [('update', 32, 32, 0)]
    plan.calls = []
    h.sync(tr).push(plan)
    assert plan.calls == [('update', 32, 32, 32)]                  # (steady state: nothing)
    # and objectives again: the device matrix is not trusted across the switch
    plan.calls = []
    h.sync(tr, 2).push(plan)
    assert plan.calls[0] == ('update', 32, 32, 32)
    assert plan.calls[1][:4] == ('objectives', 2, 32, 0)


def test_without_objectives_push_is_unchanged(dom):
    tr = _trials(dom, 30, 10)
    h = TrialHistory(dom)
    plan = _StubPlan()
    h.sync(tr).push(plan)
    assert plan.calls == [('update', 30, 0, 0)]
    assert h.Y is None
