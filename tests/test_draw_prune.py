"""The pruning sorted draw on its numpy emulation (tools/table_error.py
draw_prune): behind the pilot's sort block a wave tile is
kept iff its positions meet a non-empty bucket that holds an element inside a
hot interval.  On the tool's named histories and on config 4's hps 0 / 42 /
76, over 2^18 emulated draws each: no wave tile whose best score reaches
k_tie_gather's threshold T(tab_max) is dropped; the kept share is printed
beside the exact filter's passing share.  The ties history and u of the gap
history have no certified pair: the draw writes every tile.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, ROOT)
import table_error as TE  # noqa: E402

import test_table_bound as B  # noqa: E402

DRAWS = 1 << 18
CFG4_HPS = (0, 42, 76)


def _check(name, pair):
    tb, ta, (w, mu, sg), (low, high, pm) = pair
    y = TE.draw_below(w, mu, sg, low, high, pm, DRAWS, np.random.RandomState(23))
    r = TE.draw_prune(tb, ta, y)
    print('%s: wave tiles kept %d of %d (%.2f %%), exact filter passing %.2f %%, elements ranked '
          '%.2f %%, hot wave tiles dropped %d'
          % (name, int(r['kept'].sum()), r['kept'].size, 100.0 * r['kept'].mean(),
             100.0 * (~r['pruned']).mean(), 100.0 * r['live'], r['dropped_hot']))
    assert r['dropped_hot'] == 0
    hot = ~(r['wmax'] < r['thr'])
    assert r['kept'][hot].all()
    assert r['kept'][:TE.SORT_BLOCK // TE.WAVE].all()      # the pilot's block is whole
    # every element inside a hot interval sits in a kept tile
    y_lo, y_hi = tb['y_lo'], tb['y_lo'] + tb['width'] * tb['P']
    yb, _ = TE.bucketed_waves(y, y_lo, y_hi)
    yc = np.clip(yb, y_lo, y_hi)
    inside = np.zeros(yb.size, dtype=bool)
    for lo, hi in r['intervals']:
        inside |= (yc >= lo) & (yc <= hi)
    assert r['kept'][np.flatnonzero(inside) // TE.WAVE].all()
    assert not r['kept'].all()                             # something is dropped
    assert 0.0 < r['live'] < 1.0


@pytest.mark.parametrize('name', B.CERTIFIED)
def test_no_hot_wave_tile_is_dropped(name):
    h = B.HIST[name]
    _check(name, TE.certified_pair(h[0], h[1], h[2], *h[3]))


@pytest.mark.parametrize('name', ['gap-u', 'ties'])
def test_uncertified_slots_take_no_pruning(name):
    h = B.HIST[name]
    assert TE.certified_pair(h[0], h[1], h[2], *h[3]) is None


def test_config4_hps():
    import bench
    dom, losses, vals, act = bench.build_workload('cfg4')
    hps = list(dom.space.hps)
    for i in CFG4_HPS:
        h = hps[i]
        pair = TE.certified_pair(losses, {h.label: vals[h.index]}, h.label, 'uniform', (-5.0, 5.0))
        assert pair is not None, h.label
        _check('cfg4 hp %d' % i, pair)


def test_everything_interval_keeps_every_tile():
    """The wide tie window of the tie tests: one interval, everything."""
    h = B.HIST['shape-u']
    tb, ta, (w, mu, sg), (low, high, pm) = TE.certified_pair(h[0], h[1], h[2], *h[3])
    y = TE.draw_below(w, mu, sg, low, high, pm, 1 << 16, np.random.RandomState(23))
    r = TE.draw_prune(tb, ta, y, tie=np.inf)
    assert r['kept'].all() and r['live'] == 1.0
