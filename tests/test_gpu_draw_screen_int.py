"""The screened draw on integer uniforms (k_draw_sorted_screen_int; DESIGN
5.6): phase 1 takes the component from a guide table on the top bits of U0 and
the class from U1 against integer thresholds -- the float screen's function of
the same Philox words, so everything it writes is byte for byte what
TPE_DRAW_SCREEN_INT=0 (the float screen) and TPE_DRAW_SCREEN=0 (no screen)
write.

test_gpu_draw_screen.py's shape and cases: NC = 2^18 + 8192 + 77 candidates, 4
suggestions, a 6000-trial history, space A under its three fit sets and space
B; every run a child interpreter with TPE_DRAW_SCREEN_MIN=0, one after the
other.  TPE_DRAW_SCREEN_GUIDE_BITS=0 leaves one bucket for every pick
boundary, so no slot of space A (K = 21, 3, 79) has a valid guide: none is
screened, each runs the unscreened body.
"""
import os

import numpy as np
import pytest

from test_gpu_draw_screen import (FITS, LABELS_A, NEG_INF, NWT, SEEDS, SORT, _child, _tiles,
                                  case_all, case_graph)  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    for k in ('TPE_DRAW_SCREEN', 'TPE_DRAW_SCREEN_INT', 'TPE_DRAW_PRUNE', 'TPE_TABLE_PREFILTER'):
        assert os.environ.get(k, '1') != '0', 'the default is under test'
    for k in ('TPE_DRAW_SCREEN_TILES', 'TPE_DRAW_SCREEN_GUIDE_BITS'):
        assert k not in os.environ, 'the default is under test'
    d = str(tmp_path_factory.mktemp('drawint'))
    envs = (('default', {}), ('int=0', {'TPE_DRAW_SCREEN_INT': '0'}),
            ('screen=0', {'TPE_DRAW_SCREEN': '0'}), ('guide=0', {'TPE_DRAW_SCREEN_GUIDE_BITS': '0'}))
    return {name: _child('case_all', os.path.join(d, '%d.npz' % i), env)
            for i, (name, env) in enumerate(envs)}


def test_records_equal(runs):
    """Space A under every fit set and space B: all children give the same
    records."""
    on = runs['default'][0]
    assert set(on) == {'A/' + f for f in FITS} | {'B'}
    for name in ('int=0', 'screen=0', 'guide=0'):
        other = runs[name][0]
        for k in on:
            assert on[k]['hex'] == other[k]['hex'], (name, k)


def test_tiles_and_marks_equal(runs):
    """The tab_wmax rows, and Plan.cand_dump's values and positions on every
    kept wave tile (a dropped tile's entries are unspecified), of all children."""
    on, on_d = runs['default']
    dropped = 0
    for name in ('int=0', 'screen=0', 'guide=0'):
        other, other_d = runs[name]
        for lab in LABELS_A:
            assert on['A/default']['wmax_' + lab] == other['A/default']['wmax_' + lab], (name, lab)
            bits = np.frombuffer(bytes.fromhex(on['A/default']['wmax_' + lab]),
                                 dtype=np.uint64).reshape(len(SEEDS), NWT)
            for s in (0, 3):
                kept = bits[s] != NEG_INF
                dropped += int((~kept).sum())
                kept[:SORT // 128] = True                # the pilot's sort block is written whole
                for q in ('v', 'p'):
                    key = '%s_%d_%s' % (lab, s, q)
                    np.testing.assert_array_equal(_tiles(on_d[key])[kept], _tiles(other_d[key])[kept],
                                                  err_msg=name + ' ' + key)
    assert dropped > 0                                   # (the draw does prune here)


def test_counters(runs):
    """The classification is the float screen's: the same blocks screened and
    fallen back, the same elements inverted.  Without a guide nothing of space
    A is screened."""
    on, off = runs['default'][0], runs['int=0'][0]
    for k in on:
        print('%s: %s' % (k, on[k]['stats']))
        assert on[k]['stats'] == off[k]['stats'], k
    assert on['A/default']['stats'][0] > 0 and on['A/few-below']['stats'][0] > 0
    assert on['A/default']['K'] == [21] * 4 and on['A/few-below']['K'] == [3] * 4
    for fit in FITS:
        assert runs['guide=0'][0]['A/' + fit]['stats'] == [0, 0, 0], fit
        assert runs['screen=0'][0]['A/' + fit]['stats'] == [0, 0, 0], fit


def test_graph_replay_matches_eager():
    """TPE_GRAPH=1 (child): the replays' patched seeds reach the integer
    kernel's node -- four calls equal the eager child's."""
    eager, _ = _child('case_graph', None, {})
    graph, _ = _child('case_graph', None, {'TPE_GRAPH': '1'})
    assert graph['hex'] == eager['hex']
    assert graph['stats'][0] > 0 and list(graph['stats']) == list(eager['stats'])
