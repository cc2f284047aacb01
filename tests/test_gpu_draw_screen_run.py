"""The integer screened draw by runs (k_draw_sorted_screen_run): a
block draws TPE_DRAW_SCREEN_RUN consecutive sort blocks of its slot, with
Philox in the row form, the slot's draw table from k_draw_zone and the uniforms
compared in their word form -- everything it writes is byte for byte what
TPE_DRAW_SCREEN_RUN=0 (k_draw_sorted_screen_int, a block per sort block) and
TPE_DRAW_SCREEN=0 (no screen, the unchanged philox()) write.

test_gpu_draw_screen.py's shape and cases: NC = 2^18 + 8192 + 77 candidates, 4
suggestions, a 6000-trial history: 33 sort blocks behind the pilot's, the last
a 77-candidate one.  Runs of 3 divide 33, runs of 16 leave a run of one (the
short block alone) -- and the default run length may be any.  Every run is a
child interpreter with TPE_DRAW_SCREEN_MIN=0, one after the other (the
switches are read once per process).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_draw_screen import (FITS, LABELS_A, NC, NEG_INF, NWT, SEEDS, SORT, _child, _plan_a,
                                  _tiles, _u64hex, case_all, case_graph)  # noqa: F401
import test_gpu_table as T

pytestmark = pytest.mark.gpu

RUNS = ('run=0', 'run=1', 'run=3', 'run=16')
# cand_begin of a shard whose low counter word wraps on a row boundary inside
# sort block 4, and one whose rows straddle the wrap (the general Philox path)
WRAPS = ((1 << 32) - 5 * SORT, (1 << 32) - 5 * SORT - 17)


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    for k in ('TPE_DRAW_SCREEN', 'TPE_DRAW_SCREEN_INT', 'TPE_DRAW_PRUNE', 'TPE_TABLE_PREFILTER'):
        assert os.environ.get(k, '1') != '0', 'the default is under test'
    for k in ('TPE_DRAW_SCREEN_TILES', 'TPE_DRAW_SCREEN_GUIDE_BITS', 'TPE_DRAW_SCREEN_RUN'):
        assert k not in os.environ, 'the default is under test'
    d = str(tmp_path_factory.mktemp('drawrun'))
    envs = [('default', {})] + [(r, {'TPE_DRAW_SCREEN_RUN': r[4:]}) for r in RUNS] + \
        [('screen=0', {'TPE_DRAW_SCREEN': '0'})]
    return {name: _child('case_all', os.path.join(d, '%d.npz' % i), env)
            for i, (name, env) in enumerate(envs)}


def _same_tiles_and_marks(a, b, what):
    """tab_wmax rows equal; cand_dump values and positions equal on every kept
    wave tile (a dropped tile's entries are unspecified).  The dropped tiles."""
    (ra, da), (rb, db) = a, b
    dropped = 0
    for lab in LABELS_A:
        assert ra['A/default']['wmax_' + lab] == rb['A/default']['wmax_' + lab], (what, lab)
        bits = np.frombuffer(bytes.fromhex(ra['A/default']['wmax_' + lab]),
                             dtype=np.uint64).reshape(len(SEEDS), NWT)
        for s in (0, 3):
            kept = bits[s] != NEG_INF
            dropped += int((~kept).sum())
            kept[:SORT // 128] = True                    # the pilot's sort block is written whole
            for q in ('v', 'p'):
                key = '%s_%d_%s' % (lab, s, q)
                np.testing.assert_array_equal(_tiles(da[key])[kept], _tiles(db[key])[kept],
                                              err_msg=what + ' ' + key)
    return dropped


def test_records_equal(runs):
    """Space A under every fit set and space B: every child's records."""
    on = runs['default'][0]
    assert set(on) == {'A/' + f for f in FITS} | {'B'}
    for name in RUNS + ('screen=0',):
        for k in on:
            assert on[k]['hex'] == runs[name][0][k]['hex'], (name, k)


def test_tiles_and_marks_equal(runs):
    dropped = 0
    for name in RUNS + ('screen=0',):
        dropped += _same_tiles_and_marks(runs['default'], runs[name], name)
    assert dropped > 0                                   # (the draw does prune here)


def test_counters_equal_per_sort_block_kernel(runs):
    """Sort blocks screened, fallen back and elements inverted: the totals of
    a block per sort block, whatever the run length."""
    base = runs['run=0'][0]
    assert base['A/default']['stats'][0] > 0 and base['A/few-below']['stats'][0] > 0
    for name in ('default',) + RUNS[1:]:
        for k in base:
            print('%s %s: %s' % (name, k, runs[name][0][k]['stats']))
            assert runs[name][0][k]['stats'] == base[k]['stats'], (name, k)
    for k in base:
        assert runs['screen=0'][0][k]['stats'] == [0, 0, 0], k


def test_fallback_inside_a_run(tmp_path):
    """TPE_DRAW_SCREEN_TILES=0: some sort blocks fall back to the full body and
    others do not, so runs of 3 hold both kinds.  (The first counter is the
    sort blocks the screen completed -- the fallen-back ones are not in it --
    so "both kinds" is both counters positive.)"""
    env = {'TPE_DRAW_SCREEN_TILES': '0'}
    one = _child('case_all', str(tmp_path / 'r0.npz'), dict(env, TPE_DRAW_SCREEN_RUN='0'))
    run = _child('case_all', str(tmp_path / 'r3.npz'), dict(env, TPE_DRAW_SCREEN_RUN='3'))
    scr, fb, exact = one[0]['A/default']['stats']
    print('tiles=0, run=0: %d screened, %d fell back' % (scr, fb))
    assert fb > 0 and scr > 0
    for k in one[0]:
        assert run[0][k]['hex'] == one[0][k]['hex'], k
        assert run[0][k]['stats'] == one[0][k]['stats'], k
    _same_tiles_and_marks(run, one, 'tiles=0 run=3')


def test_graph_replay_matches_eager():
    """TPE_GRAPH=1 (child): the replays' patched seeds reach the run kernel's
    node, its fifth parameter kept -- four calls equal the eager child's."""
    env = {'TPE_DRAW_SCREEN_RUN': '3'}
    eager, _ = _child('case_graph', None, env)
    graph, _ = _child('case_graph', None, dict(env, TPE_GRAPH='1'))
    assert graph['hex'] == eager['hex']
    assert graph['stats'][0] > 0 and list(graph['stats']) == list(eager['stats'])


def case_wrap(path):
    """Space A as a shard [CB, CB + NC) of a suggestion of CB + NC candidates,
    for both WRAPS: records, marks and the dumps of suggestions 0 and 3."""
    out, arrays = {}, {}
    dom, plan = _plan_a()
    for w, cb in enumerate(WRAPS):
        plan.draw_screen_stats()
        res = plan.suggest(SEEDS, NC, cand_begin=cb, n_total=cb + NC)
        r = dict(hex=T._hex(res), stats=list(plan.draw_screen_stats()))
        wm = plan.tab_wmax(len(SEEDS))
        for lab in LABELS_A:
            i = dom.space.by_label[lab].index
            r['wmax_' + lab] = _u64hex(wm[:, i, :NWT])
            for s in (0, 3):
                v, p = plan.cand_dump(s, i)
                arrays['%d_%s_%d_v' % (w, lab, s)] = v.view(np.uint64)
                arrays['%d_%s_%d_p' % (w, lab, s)] = p
        out[str(w)] = r
    np.savez(path, **arrays)
    return out


def _child_wrap(path, env):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, json; sys.path.insert(0, 'tests'); import test_gpu_draw_screen_run as P; "
            "print('JSON' + json.dumps(P.case_wrap(%r)))" % (path,))
    r = subprocess.run([sys.executable, '-c', code], cwd=root,
                       env=dict(os.environ, TPE_DRAW_SCREEN_MIN='0', **env),
                       capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.split('JSON')[-1]), dict(np.load(path))


def test_counters_across_two_to_the_32(tmp_path):
    """The low counter word wraps inside the launch -- on a row boundary, and
    inside a row (that row takes the general Philox path): records, marks and
    kept tiles are those of TPE_DRAW_SCREEN=0, which draws with philox()."""
    on, on_d = _child_wrap(str(tmp_path / 'on.npz'), {})
    off, off_d = _child_wrap(str(tmp_path / 'off.npz'), {'TPE_DRAW_SCREEN': '0'})
    for w in ('0', '1'):
        assert on[w]['stats'][0] > 0 and off[w]['stats'] == [0, 0, 0], w
        assert on[w]['hex'] == off[w]['hex'], w
        for lab in LABELS_A:
            assert on[w]['wmax_' + lab] == off[w]['wmax_' + lab], (w, lab)
            bits = np.frombuffer(bytes.fromhex(on[w]['wmax_' + lab]),
                                 dtype=np.uint64).reshape(len(SEEDS), NWT)
            for s in (0, 3):
                kept = bits[s] != NEG_INF
                kept[:SORT // 128] = True
                for q in ('v', 'p'):
                    key = '%s_%s_%d_%s' % (w, lab, s, q)
                    np.testing.assert_array_equal(_tiles(on_d[key])[kept], _tiles(off_d[key])[kept],
                                                  err_msg=key)
