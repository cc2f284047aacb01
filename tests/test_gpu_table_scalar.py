"""The Chebyshev tables read through scalar loads: the
scalar-panel tab_eval in the operator form (mode 4) and the per-wave map
kernel k_table_map of a suggest's table pass, against the per-lane forms the
same library keeps behind TPE_TABLE_SCALAR=0.

Suggests: test_gpu_table.py's shape (3 hps, N = 6000, 2^18 + 8192 + 37
candidates: the last wave tile holds 37, one row partial and one empty) and
test_gpu_tie_gather.py's conditional plan.  Both forms evaluate one
recurrence on the same coefficients, so everything is compared bit for bit.

Operator form: candidate sets that stress the panel loop -- (a) 300 values
spread evenly over the whole range and shuffled (a 64-candidate row of the
bucketed order then spans about ten panels of the above table; 300 is no
multiple of 64) plus one NaN, which mode 4 accepts on the per-lane form too
(it lands on panel 0, gives NaN lpdfs and wins the argmax); (b) 128 copies of
one value; (c) every panel boundary of both tables with the doubles just
under and just over it, low and the last double under high, padded to 257
with posterior draws.  The lpdf bound against the oracle is test_gpu_table's
derived 2^-27 max(1, |lpdf|).

The switch is read once per process: the TPE_TABLE_SCALAR=0 run is a child
interpreter.
"""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from hyperopt_amd import _engine as E

import test_gpu_table as T
import test_gpu_tie_gather as G

pytestmark = pytest.mark.gpu

NC = T.NC
SEEDS6, SEEDS11 = T.SEEDS6, T.SEEDS11
NWT = (NC + 127) // 128          # wave tiles holding a candidate
LABELS = ('u', 'lu')
CASES = ('a', 'b', 'c')


def _u64hex(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).tobytes().hex()


def _suggest(dom, plan, seeds, wmax_labels=()):
    res = plan.suggest(seeds, NC)
    counts = plan.tie_counts(len(seeds))
    out = dict(hex=T._hex(res), counts=counts.tolist(), labels=list(dom.space.labels))
    if wmax_labels:
        wm = plan.tab_wmax(len(seeds))
        assert wm.shape[:2] == (len(seeds), len(dom.space.labels)) and wm.shape[2] >= NWT, wm.shape
        for lab in wmax_labels:
            out['wmax_' + lab] = _u64hex(wm[:, dom.space.by_label[lab].index, :NWT])
    return out


def _candidates(dom, plan, lab, case):
    i = dom.space.by_label[lab].index
    t = dom.space.engine_tables()[0][i]
    lg = t.family == E.LGMM
    dom_of = (lambda v: np.exp(v)) if lg else (lambda v: np.asarray(v, dtype=np.float64))
    lo = float(dom_of(t.low))
    hi_prev = float(np.nextafter(dom_of(t.high), -np.inf))
    rs = np.random.RandomState(5)
    if case == 'a':
        x = np.clip(dom_of(np.linspace(t.low, t.high, 300)), lo, hi_prev)
        rs.shuffle(x)
        return np.concatenate([x[:150], [np.nan], x[150:]])
    if case == 'b':
        return np.full(128, float(dom_of(0.5 * (t.low + t.high))))
    edge = np.concatenate([T._panel_points(plan, t, i, 0), T._panel_points(plan, t, i, 1)])
    edge = np.concatenate([np.nextafter(edge, -np.inf), edge, np.nextafter(edge, np.inf)])
    ends = np.array([lo, hi_prev])
    assert edge.size + ends.size < 257
    w, mu, sg = plan.mixture(i, 0)
    draws = plan.engine.sample(t.family, w, mu, sg, t.low, t.high, None, seed=98, stream=i,
                               n=257 - edge.size - ends.size)
    return np.concatenate([draws, ends, edge])


def _operator(dom, plan):
    """Mode 4 on every (label, case), with and without the lpdf outputs."""
    plan.fit()
    out = {}
    for lab in LABELS:
        i = dom.space.by_label[lab].index
        for case in CASES:
            x = _candidates(dom, plan, lab, case)
            lb, la, bi, bs = plan.score_candidates(i, x, sorted_mode=4)
            _, _, bi0, bs0 = plan.score_candidates(i, x, sorted_mode=4, want_llik=False)
            out['%s_%s' % (lab, case)] = dict(lb=_u64hex(lb), la=_u64hex(la), bi=int(bi),
                                              bs=_u64hex([bs]), bi0=int(bi0), bs0=_u64hex([bs0]))
    return out


def case_all():
    dom, plan, _ = T._plan()
    out = dict(plain=_suggest(dom, plan, SEEDS6, LABELS), op=_operator(dom, plan))
    dom, plan, _ = T._plan(True)
    out['gap'] = _suggest(dom, plan, SEEDS6, ('lu',))
    dom, plan = G._cond_plan()
    out['cond'] = _suggest(dom, plan, SEEDS11)
    return out


def _child(case, env):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, json; sys.path.insert(0, 'tests'); import test_gpu_table_scalar as S; "
            "print('JSON' + json.dumps(S.%s))" % case)
    r = subprocess.run([sys.executable, '-c', code], cwd=root, env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.split('JSON')[-1])


@pytest.fixture(scope='module')
def on_run():
    assert os.environ.get('TPE_TABLE_SCALAR', '1') != '0', 'the default form is under test'
    return case_all()


@pytest.fixture(scope='module')
def off_run():
    return _child('case_all()', {'TPE_TABLE_SCALAR': '0'})


def _wave_scores(run, lab):
    return np.frombuffer(bytes.fromhex(run['wmax_' + lab]), dtype=np.uint64)


@pytest.mark.parametrize('kind', ['plain', 'gap', 'cond'])
def test_suggest_both_forms(on_run, off_run, kind):
    """k_table_map against k_score_table<., true>: the records byte for byte,
    the direct pass's wave-tile counts equal, and every wave tile's table
    score bit for bit on the certified slots (plain: u and lu; gap: u's above
    table is not certified, so u falls back and lu keeps its tables; cond:
    inactive slots on a compact grid)."""
    on, off = on_run[kind], off_run[kind]
    assert on['labels'] == off['labels']
    assert on['hex'] == off['hex']
    assert on['counts'] == off['counts']
    cnt = np.asarray(on['counts'])
    for lab in LABELS if kind == 'plain' else ('lu',) if kind == 'gap' else ():
        a, b = _wave_scores(on, lab), _wave_scores(off, lab)
        assert a.size == len(SEEDS6) * NWT
        print(kind, lab, 'wave tiles differing:', int((a != b).sum()), 'of', a.size)
        np.testing.assert_array_equal(a, b)
        c = cnt[:, on['labels'].index(lab)]
        assert ((c > 0) & (c < G.WAVE_TILES)).all(), c     # the tables are in play
    if kind == 'gap':
        assert (cnt[:, on['labels'].index('u')] == G.WAVE_TILES).all()
    if kind == 'cond':
        assert (cnt == 0).any() and (cnt > 0).any()


@pytest.fixture(scope='module')
def oracle_plan():
    dom, plan, hist = T._plan()
    from test_gpu_shifted import _oracle_obs
    plan.fit()
    return dom, plan, _oracle_obs(dom, *hist)


@pytest.mark.parametrize('case', CASES)
@pytest.mark.parametrize('lab', LABELS)
def test_operator_scalar_panels(on_run, off_run, oracle_plan, lab, case):
    """Mode 4 through the scalar-panel tab_eval: lb and la bit for bit those
    of the per-lane form, the same argmax index and score with and without
    the lpdf outputs, and both lpdfs within 2^-27 of the oracle.  Case (a)
    carries a NaN candidate: NaN lpdfs, and it wins the argmax."""
    from test_gpu_shifted import _oracle_score
    on, off = on_run['op']['%s_%s' % (lab, case)], off_run['op']['%s_%s' % (lab, case)]
    for k in ('lb', 'la', 'bi', 'bs', 'bi0', 'bs0'):
        assert on[k] == off[k], (lab, case, k)
    dom, plan, obs = oracle_plan
    x = _candidates(dom, plan, lab, case)
    lb = np.frombuffer(bytes.fromhex(on['lb']), dtype=np.float64)
    la = np.frombuffer(bytes.fromhex(on['la']), dtype=np.float64)
    bs = np.frombuffer(bytes.fromhex(on['bs']), dtype=np.float64)[0]
    assert lb.size == x.size and la.size == x.size
    ok = ~np.isnan(x)
    ref = _oracle_score(dom, obs, lab, x[ok])
    T._assert_lpdf(lb[ok], ref['llik_b'], '%s (%s) below' % (lab, case))
    T._assert_lpdf(la[ok], ref['llik_a'], '%s (%s) above' % (lab, case))
    if not ok.all():
        nan = int(np.flatnonzero(~ok)[0])
        assert np.isnan(lb[~ok]).all() and np.isnan(la[~ok]).all()
        assert on['bi'] == nan and on['bi0'] == nan and math.isnan(bs), (on['bi'], on['bi0'], bs)
    else:
        sc = lb - la
        assert on['bi'] == int(np.argmax(sc)) and bs == sc[on['bi']], (on['bi'], bs)
