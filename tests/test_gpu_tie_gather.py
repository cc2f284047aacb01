"""The direct pass behind the Chebyshev tables on gathered blocks
(k_tie_gather / k_score_wave_tie): the table pass leaves every
wave tile's best table score, the gather lists each slot's wave tiles within
the tie window, and the direct pass scores those alone, 8 per block.

Shape of test_gpu_table.py: 3 hps, N = 6000 trials, 2^18 + 8192 + 37
candidates (265 tiles of 8 wave tiles per slot, the last sort block partial),
6 suggestions.  The conditional space puts two bounded uniforms under the two
branches of a choice, beside an unconditional one that keeps the plan in the
16-wide moment class (mom_width takes the largest expected mixture), with 11
suggestions so that the level of the two conditional hps takes the sorted
draw.  Environment switches are read once per process: their runs are child
interpreters.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from hyperopt_amd import hp, _engine as E
from hyperopt_amd.base import Domain

import test_gpu_table as T

pytestmark = pytest.mark.gpu

N, NC = T.N, T.NC
SEEDS6, SEEDS11 = T.SEEDS6, T.SEEDS11
WAVE_TILES = 8 * ((NC + 1023) // 1024)    # per slot: 8 per 1024-candidate tile
WIDE = {'TPE_TABLE_TIE_LOG2': '2000'}     # 2^2000 overflows: the threshold is -inf or NaN


def _cond_space():
    return {'u': hp.uniform('u', -5, 5),
            'c': hp.choice('c', [{'a': hp.uniform('a', -5, 5)}, {'b': hp.uniform('b', 0, 3)}])}


def _cond_plan():
    dom = Domain(lambda x: 0.0, _cond_space())
    # A categorical's score depends on the category alone, so with this many
    # candidates one history gives one branch whatever the seed -- unless the
    # two categories tie exactly, when the first candidate's wins (numpy's
    # argmax) and the seed decides: both sides of the loss split hold each
    # branch equally often, and lf >= N below keeps every weight at 1, so the
    # two posterior probabilities are sums of the same integers.
    rs = np.random.RandomState(21)
    loss = np.random.RandomState(22).rand(N)
    c = np.empty(N, dtype=np.int64)
    c[np.argsort(loss, kind='stable')] = np.arange(N) % 2
    cols = {'u': rs.uniform(-5, 5, N), 'c': c.astype(float),
            'a': np.where(c == 0, rs.uniform(-5, 5, N), 0.0),
            'b': np.where(c == 1, rs.uniform(0, 3, N), 0.0)}
    on = {'u': np.ones(N, bool), 'c': np.ones(N, bool), 'a': c == 0, 'b': c == 1}
    vals = np.stack([cols[l] for l in dom.space.labels])
    act = np.stack([on[l] for l in dom.space.labels]).astype(np.uint8)
    hps, conds, pprior = dom.space.engine_tables()
    plan = E.Plan(E.default_engine(), hps, conds, pprior, max_trials=N)
    plan.set_history(loss, vals, act)
    plan.fit(lf=N)
    return dom, plan


def case_common(gap=False):
    """The 6-suggestion call twice on one plan and once on a fresh one, and
    the hot-wave counts of the first."""
    dom, plan, _ = T._plan(gap)
    first = plan.suggest(SEEDS6, NC)
    counts = plan.tie_counts(len(SEEDS6))
    again = plan.suggest(SEEDS6, NC)
    fresh = T._plan(gap)[1].suggest(SEEDS6, NC)
    return dict(hex=T._hex(first), again=T._hex(again), fresh=T._hex(fresh),
                counts=counts.tolist(), labels=list(dom.space.labels))


def case_cond():
    dom, plan = _cond_plan()
    res = plan.suggest(SEEDS11, NC)
    counts = plan.tie_counts(len(SEEDS11))
    return dict(hex=T._hex(res), counts=counts.tolist(), labels=list(dom.space.labels),
                active=res['active'].tolist(), branch=res['value'].tolist())


def _child(case, env):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, json; sys.path.insert(0, 'tests'); import test_gpu_tie_gather as G; "
            "print('JSON' + json.dumps(G.%s))" % case)
    r = subprocess.run([sys.executable, '-c', code], cwd=root, env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.split('JSON')[-1])


@pytest.fixture(scope='module')
def default_run():
    return case_common()


@pytest.fixture(scope='module')
def wide_run():
    return _child('case_common()', WIDE)


@pytest.fixture(scope='module')
def off_run():
    return _child('case_common()', {'TPE_TABLE': '0'})


def _counts(run, label):
    return np.asarray(run['counts'])[:, run['labels'].index(label)]


def test_wide_window(wide_run, off_run):
    """Every wave hot: the full-capacity list, several gathered blocks per
    persistent block -- the records of the TPE_TABLE=0 run byte for byte, and
    every wave tile of each slot in its list."""
    assert wide_run['hex'] == off_run['hex']
    for lab in ('u', 'lu', 'n'):      # (n takes no table: every tile as well)
        c = _counts(wide_run, lab)
        print(lab, c.tolist())
        assert (c == WAVE_TILES).all(), (lab, c.tolist())
    assert (np.asarray(off_run['counts']) == -1).all()     # no such launch without tables


def test_conditional_space():
    """A choice between two branches, each holding a bounded uniform: an hp
    inactive in a suggestion has skipped that suggestion's table pass, so its
    wave scores are stale -- its list is empty, the active hp's is not, and
    the records are those of the TPE_TABLE=0 run byte for byte."""
    on = case_cond()
    off = _child('case_cond()', {'TPE_TABLE': '0'})
    lab = off['labels']
    act = np.asarray(off['active'])
    ia, ib, ic = lab.index('a'), lab.index('b'), lab.index('c')
    branch = np.asarray(off['branch'])[:, ic]
    print('branches', branch.tolist())
    assert set(branch.tolist()) == {0.0, 1.0}, branch       # both branches occur
    np.testing.assert_array_equal(act[:, ia] == 1, branch == 0.0)
    np.testing.assert_array_equal(act[:, ib] == 1, branch == 1.0)
    assert on['hex'] == off['hex']
    cnt = np.asarray(on['counts'])
    print('counts a', cnt[:, ia].tolist(), 'b', cnt[:, ib].tolist(), 'u', cnt[:, lab.index('u')].tolist())
    for i in (ia, ib):
        assert (cnt[act[:, i] == 0, i] == 0).all(), cnt[:, i]
        assert (cnt[act[:, i] == 1, i] > 0).all(), cnt[:, i]
        # (the tables are in play: a certified slot's list is a part of its tiles)
        assert (cnt[act[:, i] == 1, i] < WAVE_TILES).all(), cnt[:, i]


def test_sparse_by_default(default_run):
    """Default switches: a certified slot's list holds some of its wave tiles
    and not all of them; the uncertified u of the gap history and the normal,
    which has no table, hold all."""
    for lab in ('u', 'lu'):
        c = _counts(default_run, lab)
        print(lab, c.tolist())
        assert ((c > 0) & (c < WAVE_TILES)).all(), (lab, c.tolist())
    assert (_counts(default_run, 'n') == WAVE_TILES).all()
    gap = case_common(gap=True)
    print('gap u', _counts(gap, 'u').tolist(), 'lu', _counts(gap, 'lu').tolist())
    assert (_counts(gap, 'u') == WAVE_TILES).all()
    c = _counts(gap, 'lu')
    assert ((c > 0) & (c < WAVE_TILES)).all(), c.tolist()


def test_repeatable(default_run, wide_run):
    """The same call twice on one plan and once on a fresh plan: the same
    bytes, in the default and in the wide-window setting."""
    for run in (default_run, wide_run):
        assert run['again'] == run['hex']
        assert run['fresh'] == run['hex']
