"""Host side of the exact three-objective hypervolume gains (no GPU; DESIGN
5.18): ``hv3_oracle`` against the truth (inclusion-exclusion, and a slab sweep
of its own over the 2-d sweep area), its picks against the brute-force greedy,
the ``hv_method=`` argument checks and the plan's method code 3."""
import os
import subprocess

import numpy as np
import pytest

from hyperopt_amd import hp, tpe
from hyperopt_amd.base import Domain
from hyperopt_amd.history import TrialHistory, check_hv_method, HV_N_PICK, HV_N_SAMPLES, HV_SEED

import hv_cases
import hv_oracle as HO
import hv3_oracle as H3
import pareto_oracle as PO
import spaces
from test_hv_host import _StubPlan, _trials, HIPCC, ROOT


def _truth(Y, r, chosen, i, sweep):
    """Row i's box minus what the chosen rows dominate of it."""
    yi = Y[:, i]
    C = [np.maximum(yi, Y[:, p]) for p in chosen]
    if not sweep:
        return float(np.prod(r - yi)) - (HO.hv_inclusion_exclusion(C, r) if C else 0.0)
    cuts = sorted({float(yi[2]), float(r[2])} | {float(c[2]) for c in C})
    box, total = (r[0] - yi[0]) * (r[1] - yi[1]), 0.0
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        total += (hi - lo) * (box - HO.hv2d([(c[0], c[1]) for c in C if c[2] <= lo], r))
    return total


@pytest.mark.parametrize('n,n_pick,sweep', [(13, 6, False), (40, 9, False), (77, 9, True),
                                            (120, 40, True)])
def test_keys_are_the_true_gains_and_picks_the_brute_force_greedy(n, n_pick, sweep):
    Y, r = hv_cases.make_case(500 + n, 3, n)           # (two equal rows, rows outside r, pending)
    Y[0, 5], Y[2, 6] = Y[0, 4], Y[2, 4]                 # equal coordinates in X and in Z
    by, of = PO.pareto_counts(Y)
    part, _ = HO.participants(Y, by, r)
    trace = []
    picks, keys, counts, R = H3.hv3_select(Y, by, r, n_pick=n_pick, trace=trace)
    assert R >= 3 and (counts == -1).all() and (picks[R:] == -1).all()
    worst, zeros = 0.0, 0
    for t in range(len(trace)):
        chosen = [int(p) for p in picks[:t]]
        truth = np.zeros(n)
        for i in np.flatnonzero(part):
            if i not in chosen:
                truth[i] = _truth(Y, r, chosen, i, sweep)
                if any((Y[:, p] == Y[:, i]).all() for p in chosen):
                    assert trace[t][i] == 0.0           # a pick equals the row: exactly 0
                    zeros += 1
                else:
                    worst = max(worst, abs(trace[t][i] - truth[i]) / truth[i])
        best = int(np.argmax(np.where(truth > 1e-12, truth, 0.0)))
        assert (picks[t] == best) if t < R else truth.max() <= 1e-12
    print('n = %d: R = %d, largest relative gain error %.3g' % (n, R, worst))
    assert worst <= 1e-9 and zeros > 0


def _method_calls(dom, tr, M, hv, method):
    kw = dict(objectives=M, hypervolume=hv, hv_method=method)
    return (lambda: tpe.suggest([3], dom, tr, 0, **kw),
            lambda: tpe.suggest_from_pool([3], dom, tr, 0, pool=[{}], **kw),
            lambda: tpe.suggest_joint([3], dom, tr, 0, **kw),
            lambda: tpe.score_configs([{}], dom, tr, **kw),
            lambda: tpe.sample_configs(4, dom, tr, 0, **kw),
            lambda: tpe.pareto_ranks(dom, tr, **kw),
            lambda: tpe.pareto_front(dom, tr, **kw),
            lambda: tpe.hv_picks(dom, tr, **kw))


@pytest.mark.parametrize('hv,M,method,msg', [
    (True, 4, 'exact', 'objectives=2 or objectives=3'), (True, 1, 'exact', 'objectives=2 or'),
    (True, 3, 'fast', 'hv_method must be'), (True, 3, 3, 'hv_method must be'),
    (True, 3, None, 'hv_method must be'), (False, 3, 'mc', 'needs hypervolume'),
    (False, 3, 'exact', 'needs hypervolume')])
def test_hv_method_is_checked_before_any_engine_call(hv, M, method, msg):
    dom = Domain(lambda x: 0.0, spaces.cond_space(hp))
    tr = _trials(dom, 3, 1, objectives=M)
    for call in _method_calls(dom, tr, M, hv, method):
        with pytest.raises(ValueError, match=msg):
            call()
    assert check_hv_method('exact', True, 3) == 'exact'
    assert check_hv_method('auto', False, None) == 'auto'


@pytest.mark.parametrize('M,method,code', [(3, 'auto', 0), (2, 'auto', 0), (3, 'mc', 2),
                                           (2, 'exact', 1), (3, 'exact', 3)])
def test_push_sends_the_method(M, method, code):
    dom = Domain(lambda x: 0.0, spaces.cond_space(hp))
    tr = _trials(dom, 20, 3, objectives=M)
    ref = tuple(1.5 for _ in range(M))
    h, plan = TrialHistory(dom), _StubPlan()
    h.sync(tr, M, ref, hv_method=method).push(plan)
    assert plan.calls[1] == ('hv', ref, M, HV_N_PICK, HV_N_SAMPLES, HV_SEED, code)
    plan.calls = []
    h.sync(tr, M, ref).push(plan)                       # 'auto' after it: a full ranking again
    assert plan.calls[1][-1] == 0 and plan.calls[2] == ('objectives', M, 20, 20 if code == 0 else 0)


def test_hv_plan_method_3(tmp_path):
    exe = str(tmp_path / 'hv3_plan_check')
    src = os.path.join(ROOT, 'tests', 'host', 'hv3_plan_check.cpp')
    subprocess.check_call([HIPCC, '-x', 'hip', '--cuda-host-only', '-std=c++17', '-O1', '-g',
                           '-Wall', '-Xarch_host', '-fsanitize=address,undefined',
                           '-Xarch_host', '-fno-sanitize-recover=undefined', src, '-o', exe])
    subprocess.check_call([exe])
