"""The prefilter of a suggest's table pass (k_table_bound / k_table_pilot /
tab_prefilter): wave tiles that the certified bound of the table
score rules out leave -inf in tab_wmax instead of being scored, and nothing
downstream changes.

Suggests: test_gpu_table.py's shape (3 hps, N = 6000, 2^18 + 8192 + 37
candidates, SEEDS6), its gap history (u's above table is not certified: no
lattice, every wave tile scored) and test_gpu_tie_gather.py's conditional
plan (inactive slots on a compact grid).  The default run is compared with a
child interpreter under TPE_TABLE_PREFILTER=0 (the switch is read once per
process): records byte for byte, the direct pass's wave-tile counts, every
wave tile's table score bit for bit where the default run kept it, and where
it left -inf the unfiltered score lies under k_tie_gather's threshold
tab_max - 2^-16 max(1, |tab_max|) of the unfiltered run's own scores.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_table as T
import test_gpu_tie_gather as G
import test_gpu_table_scalar as S

pytestmark = pytest.mark.gpu

NC, NWT = T.NC, S.NWT
SEEDS6, SEEDS11 = T.SEEDS6, T.SEEDS11
WMAX = dict(plain=('u', 'lu'), gap=('u', 'lu'), cond=('u', 'a', 'b'))
NEG_INF = np.array([-np.inf]).view(np.uint64)[0]


def case_plain(repeat=False):
    dom, plan, _ = T._plan()
    out = dict(plain=S._suggest(dom, plan, SEEDS6, WMAX['plain']))
    if repeat:
        out['again'] = S._suggest(dom, plan, SEEDS6, WMAX['plain'])
        dom, plan, _ = T._plan()
        out['fresh'] = S._suggest(dom, plan, SEEDS6, WMAX['plain'])
    return out


def case_records():
    """The records alone (TPE_TABLE=0 keeps no wave scores)."""
    dom, plan, _ = T._plan()
    return dict(hex=T._hex(plan.suggest(SEEDS6, NC)))


def case_all(repeat=False):
    out = case_plain(repeat)
    dom, plan, _ = T._plan(True)
    out['gap'] = S._suggest(dom, plan, SEEDS6, WMAX['gap'])
    dom, plan = G._cond_plan()
    out['cond'] = S._suggest(dom, plan, SEEDS11, WMAX['cond'])
    return out


def _child(case, env):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, json; sys.path.insert(0, 'tests'); import test_gpu_table_prefilter as P; "
            "print('JSON' + json.dumps(P.%s))" % case)
    r = subprocess.run([sys.executable, '-c', code], cwd=root, env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.split('JSON')[-1])


@pytest.fixture(scope='module')
def on_run():
    assert os.environ.get('TPE_TABLE_PREFILTER', '1') != '0', 'the default is under test'
    return case_all(repeat=True)


@pytest.fixture(scope='module')
def off_run():
    return _child('case_all()', {'TPE_TABLE_PREFILTER': '0'})


def _bits(run, lab, n_sug):
    return np.frombuffer(bytes.fromhex(run['wmax_' + lab]), dtype=np.uint64).reshape(n_sug, NWT)


@pytest.mark.parametrize('kind', ['plain', 'gap', 'cond'])
def test_prefilter_changes_nothing_downstream(on_run, off_run, kind):
    on, off = on_run[kind], off_run[kind]
    n_sug = len(SEEDS11 if kind == 'cond' else SEEDS6)
    assert on['labels'] == off['labels']
    assert on['hex'] == off['hex']
    assert on['counts'] == off['counts']
    cnt = np.asarray(on['counts'])
    for lab in WMAX[kind]:
        a, b = _bits(on, lab, n_sug), _bits(off, lab, n_sug)
        c = cnt[:, on['labels'].index(lab)]
        if kind == 'gap' and lab == 'u':       # no certified pair: no lattice, nothing pruned
            assert not (a == NEG_INF).any()
            assert (c == G.WAVE_TILES).all(), c
            continue
        assert not (b == NEG_INF).any()        # a real score is never -inf
        fracs = []
        for s in range(n_sug):
            if c[s] == 0:                      # (cond: inactive, its wave scores are stale)
                continue
            pruned = a[s] == NEG_INF
            np.testing.assert_array_equal(a[s][~pruned], b[s][~pruned])
            w = b[s].view(np.float64)
            tab_max = np.nan if np.isnan(w).any() else w.max()
            thr = tab_max - 2.0 ** -16 * max(1.0, abs(tab_max))
            assert (w[pruned] < thr).all(), (kind, lab, s, float(w[pruned].max()), thr)
            assert pruned.any() and not pruned.all(), (kind, lab, s, int(pruned.sum()))
            assert (c[s] > 0) and (c[s] <= int((~pruned).sum()) + (G.WAVE_TILES - NWT))
            fracs.append(pruned.mean())
        assert fracs, (kind, lab)
        print('%s %s: pruned fraction of the wave tiles min %.4f median %.4f max %.4f'
              % (kind, lab, min(fracs), float(np.median(fracs)), max(fracs)))


def test_wide_window_prunes_nothing():
    """TPE_TABLE_TIE_LOG2=2000: the threshold is -inf or NaN, no compare
    prunes -- no -inf entry, and the records are those of TPE_TABLE=0."""
    wide = _child('case_plain()', dict(G.WIDE))['plain']
    off = _child('case_records()', {'TPE_TABLE': '0'})
    for lab in WMAX['plain']:
        assert not (_bits(wide, lab, len(SEEDS6)) == NEG_INF).any(), lab
    assert wide['hex'] == off['hex']


def test_repeatable(on_run):
    """The same plan suggested twice and a fresh plan: the same tab_wmax bytes
    (pruned entries included: the hot intervals depend on the scores and the
    lattice alone), the same records and counts."""
    first = on_run['plain']
    for other in (on_run['again'], on_run['fresh']):
        for k in ('hex', 'counts') + tuple('wmax_' + l for l in WMAX['plain']):
            assert other[k] == first[k], k
