"""Host side of the hypervolume subset selection inside the Pareto front (no
GPU): the rule as the numpy oracle states it against ground truth
(a brute-force greedy on the 2-d sweep hypervolume, inclusion-exclusion in
more dimensions), the surrogate's properties, the default reference point, the
``hypervolume=`` argument checks, the order in which ``push`` talks to a plan,
and the launch plan of the device pass (a stand-alone sanitized program)."""
import math
import os
import subprocess

import numpy as np
import pytest

import hyperopt_amd as H
from hyperopt_amd import hp, rand, tpe, Trials, trials_from_docs
from hyperopt_amd.base import Domain
from hyperopt_amd.history import (TrialHistory, check_hypervolume, default_reference,
                                  HV_N_PICK, HV_N_SAMPLES, HV_SEED, HV_METHOD)

import hv_cases
import hv_oracle as HO
import pareto_oracle as PO
import spaces

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


# ------------------------------------------------------- the exact rule, M = 2
def _brute_greedy(Y, part, r, n_pick):
    """Greedy subset selection by the sweep hypervolume itself: in every round
    the participant whose addition enlarges hv2d the most, ties to the lower
    row; ends when nothing adds area.  (picks, gains)."""
    rows = [int(i) for i in np.flatnonzero(part)]
    chosen, picks, gains = [], [], []
    for _ in range(n_pick):
        base = HO.hv2d(chosen, r)
        best, best_gain = -1, 0.0
        for i in rows:
            if i in picks:
                continue
            g = HO.hv2d(chosen + [tuple(Y[:, i])], r) - base
            if g > best_gain:
                best, best_gain = i, g
        if best < 0:
            break
        picks.append(best)
        gains.append(best_gain)
        chosen.append(tuple(Y[:, best]))
    return picks, gains


@pytest.mark.parametrize('n', [5, 8, 13, 40, 77, 120])
def test_exact_picks_are_the_brute_force_greedy(n):
    Y, r = hv_cases.make_case(100 + n, 2, n)
    by, of = PO.pareto_counts(Y)
    part, _ = HO.participants(Y, by, r)
    n_pick = 12
    picks, keys, counts, R = HO.hv_select(Y, by, r, n_pick=n_pick)
    want, gains = _brute_greedy(Y, part, r, n_pick)
    assert R == len(want) and R > 0
    assert picks[:R].tolist() == want
    assert (picks[R:] == -1).all() and (counts == -1).all() and (keys[R:] == 0).all()
    worst = 0.0
    for t in range(R):
        worst = max(worst, abs(keys[t] - gains[t]) / gains[t])
    print('n = %d: R = %d, largest relative gain error %.3g' % (n, R, worst))
    assert worst <= 1e-9
    if n >= 8:
        # the special rows: no pending, outside or infinite row is ever picked, and
        # of the two equal rows (0.0 / -0.0) only the lower one
        assert part[picks[:R]].all()
        dup = [i for i in range(n) if Y[0, i] == 0.0 and by[i] == 0 and part[i]]
        assert len(dup) == 2 and np.signbit(Y[0, dup]).sum() == 1
        if R < n_pick:                                  # the front was exhausted
            assert dup[0] in want and dup[1] not in want
            assert R == part.sum() - 1


def test_exact_ties_go_to_the_lower_row():
    # a symmetric front: rows 0 and 2 have the same box; row 1 is the knee
    Y = np.array([[0.0, 0.5, 1.0, 0.25], [1.0, 0.5, 0.0, 0.9]])
    r = np.array([2.0, 2.0])
    by, of = PO.pareto_counts(Y)
    picks, keys, _, R = HO.hv_select(Y, by, r, n_pick=4)
    assert picks.tolist() == [1, 0, 2, 3] and R == 4
    assert keys.tolist() == [2.25, 0.5, 0.5, (0.5 - 0.25) * (1.0 - 0.9)]


# ------------------------------------------------ Monte-Carlo against the truth
def _gain_truth(Y, r, chosen, i):
    """vol_i minus the part of row i's box the chosen rows cover: inclusion-
    exclusion over the chosen set of the boxes [max(y_i, y_p, ...), r]."""
    yi = Y[:, i]
    return float(np.prod(r - yi)) - HO.hv_inclusion_exclusion(
        [np.maximum(yi, Y[:, p]) for p in chosen], r) if chosen else float(np.prod(r - yi))


@pytest.mark.parametrize('M,n,n_pick', [(2, 60, 6), (2, 120, 10), (3, 60, 6), (5, 60, 6),
                                        (8, 60, 6)])
def test_monte_carlo_keys_stay_inside_the_hoeffding_bound(M, n, n_pick):
    S = 1024
    Y, r = hv_cases.make_case(200 + M, M, n)
    by, of = PO.pareto_counts(Y)
    part, w = HO.participants(Y, by, r)
    vol = HO.volumes(w)
    trace = []
    picks, keys, counts, R = HO.hv_select(Y, by, r, n_pick=n_pick, n_samples=S, method=HO.MC,
                                          trace=trace)
    assert R == n_pick and len(trace) == n_pick
    rows = np.flatnonzero(part)
    N = len(rows) * n_pick                              # (row, round) estimates covered
    eps = math.sqrt(math.log(2 * N / 1e-6) / (2 * S))
    worst = 0.0
    for t in range(n_pick):
        chosen = [int(p) for p in picks[:t]]
        for i in rows:
            if i in chosen:
                assert trace[t][i] == 0.0
                continue
            if M == 2:
                pts = [tuple(Y[:, p]) for p in chosen]
                truth = HO.hv2d(pts + [tuple(Y[:, i])], r) - HO.hv2d(pts, r)
            else:
                truth = _gain_truth(Y, r, chosen, i)
            worst = max(worst, abs(trace[t][i] / (S * vol[i]) - truth / vol[i]))
    print('M = %d: N = %d estimates, eps = %.4f, largest error %.4f' % (M, N, eps, worst))
    assert worst <= eps
    assert (counts[:R] > 0).all() and counts[0] == S and keys[0] == vol[picks[0]] * S


def test_the_sample_table_is_the_draw_of_its_own_stream():
    from draw_replay import uniforms
    u = HO.uniform_table(7, 128, 6)
    assert u.shape == (128, 6) and (u >= 0).all() and (u < 1).all()
    a = uniforms(7, np.arange(128, dtype=np.uint64), 0x60000000, 0)
    b = uniforms(7, np.arange(128, dtype=np.uint64), 0x60000000, 1)
    assert (u[:, 0] == a[0]).all() and (u[:, 3] == a[3]).all()
    assert (u[:, 4] == b[0]).all() and (u[:, 5] == b[1]).all()
    assert abs(u.mean() - 0.5) < 0.05


# -------------------------------------------------------------- the surrogate
@pytest.mark.parametrize('M,method', [(2, HO.AUTO), (2, HO.MC), (3, HO.AUTO), (8, HO.AUTO)])
def test_surrogate_properties(M, method):
    n = 60
    Y, r = hv_cases.make_case(300 + M, M, n)
    by, of, s, picks, keys, counts, R = HO.hv_rank(Y, r, n_pick=5, n_samples=128, method=method,
                                                   fast=False)
    assert R == 5
    ok = PO.complete_rows(Y)
    pairs = 0
    for a in range(n):
        for b in range(n):
            if ok[a] and ok[b] and PO.dominates(Y[:, a], Y[:, b]):
                assert s[a] < s[b], (a, b)
                pairs += 1
    assert pairs > 0
    assert np.isinf(s[~ok]).all() and (s[ok] == np.floor(s[ok])).all()
    assert s[picks[:R]].tolist() == list(range(R))       # dominated_by = 0, sec = t
    front = np.flatnonzero((by == 0) & ok)
    rest = np.setdiff1d(front, picks[:R])
    assert len(rest) > 0 and (s[rest] >= R).all() and (s[rest] <= n).all()
    behind = np.flatnonzero(by > 0)
    _, _, s0 = PO.pareto_rank(Y)
    assert (s[behind] == s0[behind]).all()               # only the front is reordered
    # the first rows of the split are the picks, in pick order
    assert np.argsort(s, kind='stable')[:R].tolist() == picks[:R].tolist()


def test_one_objective_is_untouched():
    rng = np.random.RandomState(5)
    Y = rng.rand(1, 40)
    by, of, s, picks, keys, counts, R = HO.hv_rank(Y, [2.0])
    assert R == 0 and (picks == -1).all()
    assert (s == PO.pareto_rank(Y)[2]).all()


@pytest.mark.parametrize('M', [2, 3])
def test_a_front_outside_the_reference_point_leaves_the_old_column(M):
    Y, r = hv_cases.outside_case(400 + M, M, 50)
    by, of, s, picks, keys, counts, R = HO.hv_rank(Y, r, n_pick=5, n_samples=64)
    assert R == 0 and (picks == -1).all() and (keys == 0).all()
    assert np.array_equal(s, PO.pareto_rank(Y)[2])       # bit for bit (inf == inf)


def test_an_infinite_volume_never_meets_a_zero_count():
    # boxes that overflow: vol = +inf; a key is vol * cnt or 0, never 0 * inf
    Y = np.array([[-1e200, 0.0, 1.0], [1.0, 0.0, -1e200]])
    r = np.array([1e200, 1e200])
    by, of = PO.pareto_counts(Y)
    trace = []
    picks, keys, counts, R = HO.hv_select(Y, by, r, n_pick=3, n_samples=64, method=HO.MC,
                                          trace=trace)
    assert all(np.isfinite(k).all() or (k[np.isinf(k)] > 0).all() for k in trace)
    assert not any(np.isnan(k).any() for k in trace)
    assert R >= 1


# ------------------------------------------------- the default reference point
def test_default_reference_point():
    Y = np.array([[0.0, 1.0, 3.0, np.nan, 100.0, -np.inf],
                  [2.0, 2.0, 2.0, 5.0, np.inf, 2.0]])
    # complete rows: 0, 1, 2, 5; objective 0 finite values 0, 1, 3; objective 1 all 2
    assert default_reference(Y) == (3.0 + 0.1 * 3.0, 3.0)
    assert default_reference(Y) == HO.default_reference(Y)
    assert default_reference(np.array([[np.nan, np.inf], [1.0, 1.0]])) is None
    assert default_reference(np.zeros((2, 0))) is None
    rng = np.random.RandomState(2)
    Z = rng.randn(3, 30)
    assert default_reference(Z) == HO.default_reference(Z)
    for m, v in enumerate(default_reference(Z)):
        assert v > Z[m].max()


def _trials(dom, n, seed, objectives=None):
    docs = rand.suggest(list(range(n)), dom, Trials(), seed)
    rng = np.random.RandomState(seed + 1)
    for d in docs:
        d['state'] = H.JOB_STATE_DONE
        d['result'] = {'status': 'ok', 'loss': float(rng.rand())}
        if objectives:
            d['result']['objectives'] = [float(v) for v in rng.rand(objectives)]
    return trials_from_docs(docs)


@pytest.fixture
def dom():
    return Domain(lambda x: 0.0, spaces.cond_space(hp))


def test_history_reference(dom):
    tr = _trials(dom, 20, 3, objectives=2)
    h = TrialHistory(dom).sync(tr, 2, True)
    assert h.hv is True and h.reference() == default_reference(h.Y[:, :20])
    h.sync(tr, 2, (1.5, 2))
    assert h.hv == (1.5, 2.0) and h.reference() == (1.5, 2.0)
    h.sync(tr, 2)
    assert h.hv is False and h.reference() is None
    for d in tr.trials:                                 # no complete row: off for the call
        d['result']['status'] = 'fail'
    tr.refresh()
    h = TrialHistory(dom).sync(tr, 2, True)
    assert h.reference() is None


# ------------------------------------------------- the hypervolume= argument
BAD = [None, 1, 0, 2.0, 'yes', (1.0,), (1.0, 2.0, 3.0), (1.0, float('nan')),
       (1.0, float('inf')), (1.0, 'a'), (True, 1.0), [[1.0, 2.0]], {}]


def _calls(dom, tr, objectives, hv):
    return (lambda: tpe.suggest([3], dom, tr, 0, objectives=objectives, hypervolume=hv),
            lambda: tpe.suggest_from_pool([3], dom, tr, 0, pool=[{}], objectives=objectives,
                                          hypervolume=hv),
            lambda: tpe.suggest_joint([3], dom, tr, 0, objectives=objectives, hypervolume=hv),
            lambda: tpe.score_configs([{}], dom, tr, objectives=objectives, hypervolume=hv),
            lambda: tpe.sample_configs(4, dom, tr, 0, objectives=objectives, hypervolume=hv),
            lambda: tpe.pareto_ranks(dom, tr, objectives, hypervolume=hv),
            lambda: tpe.pareto_front(dom, tr, objectives, hypervolume=hv),
            lambda: tpe.hv_picks(dom, tr, objectives, hypervolume=hv))


@pytest.mark.parametrize('bad', BAD, ids=[repr(b) for b in BAD])
def test_hypervolume_must_be_a_flag_or_a_reference_point(dom, bad):
    tr = _trials(dom, 3, 1, objectives=2)
    for call in _calls(dom, tr, 2, bad):
        with pytest.raises(ValueError, match='hypervolume'):
            call()


@pytest.mark.parametrize('hv', [True, (1.0, 1.0)])
def test_hypervolume_needs_objectives(dom, hv):
    tr = _trials(dom, 3, 1, objectives=2)
    for call in _calls(dom, tr, None, hv)[:5]:
        with pytest.raises(ValueError, match='hypervolume needs objectives'):
            call()
    for call in _calls(dom, tr, None, hv)[5:]:           # (these need objectives anyway)
        with pytest.raises(ValueError, match='objectives'):
            call()


def test_check_hypervolume_values():
    assert check_hypervolume(False, None) is False and check_hypervolume(False, 3) is False
    assert check_hypervolume(True, 2) is True
    assert check_hypervolume([1, 2.5], 2) == (1.0, 2.5)
    assert check_hypervolume(np.array([1.0, 2.0, -3.0]), 3) == (1.0, 2.0, -3.0)
    assert check_hypervolume((0.5,), 1) == (0.5,)


def test_startup_is_rand_suggest_with_hypervolume(dom):
    tr = _trials(dom, 3, 4, objectives=2)
    a = tpe.suggest([5], dom, tr, 7, objectives=2, hypervolume=True)
    b = tpe.suggest([5], dom, tr, 7)
    assert a[0]['misc']['vals'] == b[0]['misc']['vals']


# ------------------------------------------------------------- push and a plan
class _StubPlan(object):
    """Records what ``push`` sends (no engine)."""

    def __init__(self):
        self.calls = []

    def update_history(self, n, row0, vals, active, ld, loss0, losses, stream=None):
        self.calls.append(('update', n, row0, loss0))

    def set_hv(self, ref, n_obj=None, n_pick=32, n_samples=1024, seed=0, method=0):
        self.calls.append(('hv', None if ref is None else tuple(ref), n_obj, n_pick, n_samples,
                           seed, method))
        self._hv_on = ref is not None                   # (as Plan.set_hv keeps it)

    def set_objectives(self, Y, n=None, obj0=0, stream=None):
        self.calls.append(('objectives', Y.shape[0], n, obj0))


def test_push_reranks_when_only_hypervolume_changes(dom):
    tr = _trials(dom, 30, 8, objectives=2)
    h = TrialHistory(dom)
    plan = _StubPlan()
    h.sync(tr, 2).push(plan)                            # off: the plan never hears of the setting
    assert [c[0] for c in plan.calls] == ['update', 'objectives']
    plan.calls = []
    h.sync(tr, 2, (1.1, 1.2)).push(plan)                # on: the setting, then a full ranking
    assert plan.calls == [('update', 30, 30, 30),
                          ('hv', (1.1, 1.2), 2, HV_N_PICK, HV_N_SAMPLES, HV_SEED, HV_METHOD),
                          ('objectives', 2, 30, 0)]
    assert (HV_N_PICK, HV_N_SAMPLES, HV_SEED, HV_METHOD) == (32, 1024, 0, 0)
    plan.calls = []
    h.sync(tr, 2, (1.1, 1.2)).push(plan)                # steady state: no row travels
    assert plan.calls[1][0] == 'hv' and plan.calls[2] == ('objectives', 2, 30, 30)
    plan.calls = []
    h.sync(tr, 2, True).push(plan)                      # the default point, from Y
    assert plan.calls[1] == ('hv', default_reference(h.Y[:, :30]), 2, 32, 1024, 0, 0)
    assert plan.calls[2] == ('objectives', 2, 30, 0)
    plan.calls = []
    h.sync(tr, 2).push(plan)                            # off again: said once, re-ranked
    assert plan.calls == [('update', 30, 30, 30), ('hv', None, None, 32, 1024, 0, 0),
                          ('objectives', 2, 30, 0)]
    plan.calls = []
    h.sync(tr, 2).push(plan)
    assert plan.calls == [('update', 30, 30, 30), ('objectives', 2, 30, 30)]
    plan.calls = []
    h.sync(tr).push(plan)                               # the scalar loss: every loss again
    assert plan.calls == [('update', 30, 30, 0)]


# ------------------------------------------------------------ the launch plan
def test_hv_plan_host_checks(tmp_path):
    """The launches and buffers of the selection (tpe_hv_plan.hpp): row tiles
    and sample words cover their ranges exactly once, the sample table has one
    slot per (sample, objective), LDS within the limit; host-only, address and
    undefined-behaviour sanitizers, a stand-alone program."""
    if not os.path.exists(HIPCC):
        pytest.fail('hipcc not found at %s' % HIPCC)
    exe = str(tmp_path / 'hv_plan_check')
    src = os.path.join(ROOT, 'tests', 'host', 'hv_plan_check.cpp')
    cc = subprocess.run(
        [HIPCC, '-x', 'hip', '--cuda-host-only', '-std=c++17', '-O1', '-g', '-Wall',
         '-Xarch_host', '-fsanitize=address,undefined',
         '-Xarch_host', '-fno-sanitize-recover=undefined', src, '-o', exe],
        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert cc.returncode == 0, cc.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       universal_newlines=True)
    assert r.returncode == 0, r.stdout
