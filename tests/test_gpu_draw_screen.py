"""The screened pruning draw (k_draw_zone, k_draw_sorted_screen):
behind the pilot the draw inverts the CDF only of the candidates whose
(component, u1) can land near a hot interval, and composes the kept wave tiles
from those alone -- byte for byte the tiles k_draw_sorted_prune writes.

Space A: four bounded uniforms (the <32, true> launch, screened).  Space B:
test_gpu_table.py's u, n, lu (the <., false> launch: the screen is not used).
Every run is NC = 2^18 + 8192 + 77 candidates for 4 suggestions on a 6000-trial
history: 34 sort blocks -- the pilot's, 32 whole ones and a 77-candidate one
with a single partial wave tile.  (The pruning draw runs only behind the
Chebyshev tables: suggestions of more than 2^18 candidates, a history in the
16-wide moment class -- 4000 trials up -- and 2^22 candidates per launch.  This
is the smallest shape of this kind that reaches it; a 400-trial history or
2 * 8192 + 77 candidates would take k_draw and test nothing.)

The engine screens launches of 2^26 candidate-slots up (below, k_draw_zone
costs more than the screen saves), so every run here is a child interpreter
with TPE_DRAW_SCREEN_MIN=0: the default one is compared with children that add
TPE_DRAW_SCREEN=0, TPE_DRAW_PRUNE=0 and TPE_DRAW_SCREEN_TILES=0 (the switches
are read once per process), and a TPE_GRAPH=1 child with an eager one.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from hyperopt_amd import hp, _engine as E
from hyperopt_amd.base import Domain

import test_gpu_table as T

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import table_error as TE  # noqa: E402

pytestmark = pytest.mark.gpu

N = 6000
NC = (1 << 18) + 8192 + 77
NWT = (NC + 127) // 128
SORT = 8192
SEEDS = [4001 + 29 * s for s in range(4)]
LABELS_A = ('a', 'b', 'c', 'd')
FITS = ('default', 'few-below', 'wide-below')
NEG_INF = np.array([-np.inf]).view(np.uint64)[0]


def _space_a():
    return {'a': hp.uniform('a', -5, 5), 'b': hp.uniform('b', 0, 1),
            'c': hp.uniform('c', -300, -100), 'd': hp.uniform('d', 2, 2.5)}


def _plan_a(fit='default'):
    """The good trials cluster: a's at its low edge, b's in the middle, c's at
    its high edge, d's nowhere (the loss ignores it)."""
    dom = Domain(lambda x: 0.0, _space_a())
    rs = np.random.RandomState(21)
    cols = {'a': rs.uniform(-5, 5, N), 'b': rs.uniform(0, 1, N), 'c': rs.uniform(-300, -100, N),
            'd': rs.uniform(2, 2.5, N)}
    loss = ((cols['a'] + 5) / 10) ** 2 + (cols['b'] - 0.55) ** 2 + ((cols['c'] + 100) / 200) ** 2 \
        + 0.02 * rs.rand(N)
    vals = np.stack([cols[l] for l in dom.space.labels])
    hps, conds, pprior = dom.space.engine_tables()
    plan = E.Plan(E.default_engine(), hps, conds, pprior, max_trials=N)
    plan.set_history(loss, vals, np.ones_like(vals, dtype=np.uint8))
    plan.fit(**TE.fit_params(fit))
    return dom, plan


def _u64hex(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).tobytes().hex()


def case_all(path):
    """Space A under every fit set (dumps and tab_wmax of the default one) and
    space B; per run the records and the screen's counters."""
    out, arrays = {}, {}
    for fit in FITS:
        dom, plan = _plan_a(fit)
        plan.draw_screen_stats()
        res = plan.suggest(SEEDS, NC)
        r = dict(hex=T._hex(res), stats=list(plan.draw_screen_stats()),
                 K=[int(plan.mixture(dom.space.by_label[l].index, 0)[0].size) for l in LABELS_A])
        if fit == 'default':
            wm = plan.tab_wmax(len(SEEDS))
            for lab in LABELS_A:
                i = dom.space.by_label[lab].index
                r['wmax_' + lab] = _u64hex(wm[:, i, :NWT])
                for s in (0, 3):
                    v, p = plan.cand_dump(s, i)
                    assert v.shape == (NC,) and p.shape == (NC,)
                    arrays['%s_%d_v' % (lab, s)] = v.view(np.uint64)
                    arrays['%s_%d_p' % (lab, s)] = p
        out['A/' + fit] = r
    dom, plan, _ = T._plan()
    plan.draw_screen_stats()
    res = plan.suggest(SEEDS, NC)
    out['B'] = dict(hex=T._hex(res), stats=list(plan.draw_screen_stats()))
    np.savez(path, **arrays)
    return out


def case_graph(path=None):
    """fit_suggest four times with changing seeds (TPE_GRAPH=1: the later calls
    replay the captured step with patched seeds)."""
    dom, plan = _plan_a()
    return dict(hex=[T._hex(plan.fit_suggest([s + 1000 * i for s in SEEDS], NC)) for i in range(4)],
                stats=list(plan.draw_screen_stats()))


@pytest.fixture(scope='module')
def tmpdir_mod():
    with tempfile.TemporaryDirectory() as d:
        yield d


def _child(case, path, env):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, json; sys.path.insert(0, 'tests'); import test_gpu_draw_screen as P; "
            "print('JSON' + json.dumps(P.%s(%r)))" % (case, path))
    r = subprocess.run([sys.executable, '-c', code], cwd=root,
                       env=dict(os.environ, TPE_DRAW_SCREEN_MIN='0', **env),
                       capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.split('JSON')[-1]), (dict(np.load(path)) if case == 'case_all' else None)


@pytest.fixture(scope='module')
def on_run(tmpdir_mod):
    for k in ('TPE_DRAW_SCREEN', 'TPE_DRAW_PRUNE', 'TPE_TABLE_PREFILTER'):
        assert os.environ.get(k, '1') != '0', 'the default is under test'
    assert 'TPE_DRAW_SCREEN_TILES' not in os.environ, 'the default is under test'
    return _child('case_all', os.path.join(tmpdir_mod, 'on.npz'), {})


@pytest.fixture(scope='module')
def screen_off(tmpdir_mod):
    return _child('case_all', os.path.join(tmpdir_mod, 'soff.npz'), {'TPE_DRAW_SCREEN': '0'})


@pytest.fixture(scope='module')
def tiles0(tmpdir_mod):
    return _child('case_all', os.path.join(tmpdir_mod, 't0.npz'), {'TPE_DRAW_SCREEN_TILES': '0'})


def _tiles(a):
    pad = NWT * 128 - a.size
    return np.concatenate([a, np.repeat(a[-1:], pad)]).reshape(NWT, 128)


def test_records_equal_without_the_screen(on_run, screen_off, tiles0, tmpdir_mod):
    """Space A, every fit set, and space B: the records of the default run are
    those of TPE_DRAW_SCREEN=0, TPE_DRAW_PRUNE=0 and TPE_DRAW_SCREEN_TILES=0."""
    prune_off, _ = _child('case_all', os.path.join(tmpdir_mod, 'poff.npz'), {'TPE_DRAW_PRUNE': '0'})
    on = on_run[0]
    for name, other in (('screen=0', screen_off[0]), ('prune=0', prune_off), ('tiles=0', tiles0[0])):
        for k in on:
            assert on[k]['hex'] == other[k]['hex'], (name, k)
    for k in on:
        assert screen_off[0][k]['stats'] == [0, 0, 0], k
        assert prune_off[k]['stats'] == [0, 0, 0], k


def test_tiles_and_marks_equal(on_run, screen_off, tiles0):
    """Plan.cand_dump on every kept wave tile and the tab_wmax marks against the
    TPE_DRAW_SCREEN=0 child -- for the default widening and for none."""
    off, off_d = screen_off
    for name, (run, dump) in (('default', on_run), ('tiles=0', tiles0)):
        dropped = 0
        for lab in LABELS_A:
            assert run['A/default']['wmax_' + lab] == off['A/default']['wmax_' + lab], (name, lab)
            bits = np.frombuffer(bytes.fromhex(run['A/default']['wmax_' + lab]),
                                 dtype=np.uint64).reshape(len(SEEDS), NWT)
            for s in (0, 3):
                kept = bits[s] != NEG_INF
                dropped += int((~kept).sum())
                kept[:SORT // 128] = True                # the pilot's sort block is written whole
                for q in ('v', 'p'):
                    key = '%s_%d_%s' % (lab, s, q)
                    np.testing.assert_array_equal(_tiles(dump[key])[kept], _tiles(off_d[key])[kept],
                                                  err_msg=name + ' ' + key)
        assert dropped > 0, name                         # (the draw does prune here)


def test_screen_counters(on_run, tiles0):
    """Blocks are screened, fewer candidates than all are inverted; space B
    and the wide-below set (K = 79: the large table's launch) never reach the
    screen; without the widening some blocks fall back."""
    on = on_run[0]
    assert on['A/default']['K'] == [21] * 4 and on['A/few-below']['K'] == [3] * 4
    assert on['A/wide-below']['K'] == [79] * 4
    for fit in ('default', 'few-below'):
        scr, fb, exact = on['A/' + fit]['stats']
        print('%s: %d sort blocks screened, %d fell back, %.4f of the screened blocks\' candidates '
              'inverted' % (fit, scr, fb, exact / max(1, scr * SORT)))
        # (at most 16 of the screened blocks are 77-candidate ones)
        least = max(0, scr - 16) * SORT + min(scr, 16) * 77
        assert scr > 0 and exact < least, (fit, scr, fb, exact)
    assert on['A/wide-below']['stats'] == [0, 0, 0]
    assert on['B']['stats'] == [0, 0, 0]
    scr, fb, exact = tiles0[0]['A/default']['stats']
    print('tiles=0: %d sort blocks screened, %d fell back' % (scr, fb))
    assert fb > 0
    # this process, without TPE_DRAW_SCREEN_MIN: a launch under 2^26
    # candidate-slots is not screened, and gives the same records
    assert 'TPE_DRAW_SCREEN_MIN' not in os.environ, 'the default is under test'
    dom, plan = _plan_a()
    plan.draw_screen_stats()
    res = plan.suggest(SEEDS, NC)
    assert plan.draw_screen_stats() == (0, 0, 0)
    assert T._hex(res) == on['A/default']['hex']


def test_graph_replay_matches_eager(tmpdir_mod):
    """TPE_GRAPH=1 (child): replays with changed seeds equal the eager calls,
    and the replayed step runs the screened draw."""
    eager, _ = _child('case_graph', None, {})
    graph, _ = _child('case_graph', None, {'TPE_GRAPH': '1'})
    assert graph['hex'] == eager['hex']
    assert graph['stats'][0] > 0 and list(graph['stats']) == list(eager['stats'])
