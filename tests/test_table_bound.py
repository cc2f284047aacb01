"""The prefilter of the table pass on its numpy emulation (tools/table_error.py,
DESIGN 5.10): the bound lattice U[c] of the table score, the hot intervals a
pilot score leaves, and the pruning of value-bucketed wave tiles.

Histories: the shape of test_gpu_table.py (N = 6000, hps u and lu); one whose
good trials cluster at the lower bound, so the EI maximum sits at `low`
(config 4's hp 0 behaves like this), its mirror at `high`, the band (99 % of
the trials a quarter unit wide: the certificate closest to its bar) and the
comb (a local maximum of the score per tooth); the gap history (--gap
u:-3:0), where u has no certified pair -- it takes no lattice and is skipped
-- and lu does; and the ties history (half-unit values), which has none either.

Per hp: every cell's bound holds at both end points, the midpoint and 16
random points (cells straddling a panel edge of either table and the two edge
cells with arguments clamped from outside the range included); and over 2^18
emulated draws no wave tile whose best score reaches k_tie_gather's threshold
T(tab_max) is pruned, while at least one wave tile is.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import table_error as TE  # noqa: E402

DRAWS = 1 << 18


def _histories():
    out = {}
    losses, cols, specs = TE.test_shape(6000)
    for lab in ('u', 'lu'):
        out['shape-' + lab] = (losses, cols, lab, specs[lab])
    losses, cols, specs = TE.low_edge_shape(6000)
    out['low-edge'] = (losses, cols, 'e', specs['e'])
    for name in ('high-edge', 'band', 'comb', 'ties'):
        losses, cols, specs = TE.NAMED[name](6000)
        out[name] = (losses, cols, 'e', specs['e'])
    losses, cols, specs = TE.test_shape(6000, ('u', -3.0, 0.0))
    for lab in ('u', 'lu'):
        out['gap-' + lab] = (losses, cols, lab, specs[lab])
    return out


HIST = _histories()
CERTIFIED = ('shape-u', 'shape-lu', 'low-edge', 'gap-lu', 'high-edge', 'band', 'comb')


@pytest.fixture(scope='module')
def pairs():
    return {k: TE.certified_pair(h[0], h[1], h[2], *h[3]) for k, h in HIST.items()}


def test_gap_slot_has_no_pair(pairs):
    """u of the gap history loses panels of its above table, the ties
    history one: no lattice."""
    assert pairs['gap-u'] is None
    assert pairs['ties'] is None
    for k in CERTIFIED:
        assert pairs[k] is not None, k


@pytest.mark.parametrize('name', CERTIFIED)
def test_lattice_bounds_the_score(pairs, name):
    tb, ta, _, _ = pairs[name]
    U = TE.bound_lattice(tb, ta)
    C = U.size
    y_lo = tb['y_lo']
    y_hi = y_lo + tb['width'] * tb['P']
    cw = (y_hi - y_lo) / C
    assert np.isfinite(U).all(), int((~np.isfinite(U)).sum())
    rs = np.random.RandomState(17)
    c = np.arange(C, dtype=np.float64)
    lo, hi = y_lo + cw * c, y_lo + cw * (c + 1.0)
    pts = np.concatenate([lo[:, None], hi[:, None], 0.5 * (lo + hi)[:, None],
                          lo[:, None] + cw * rs.rand(C, 16)], axis=1)
    s = TE.score(tb, ta, pts.reshape(-1)).reshape(pts.shape)
    worst = float((s - U[:, None]).max())
    print(name, 'max(score - U) over cells:', worst, 'median U - max score:',
          float(np.median(U - s.max(1))))
    assert (s <= U[:, None]).all(), worst
    # cells that hold a panel edge of either table are among those checked
    for tab in (tb, ta):
        edges = tab['y_lo'] + tab['width'] * np.arange(1, tab['P'])
        cells = np.unique(np.clip(np.floor((edges - y_lo) / cw), 0, C - 1).astype(int))
        assert cells.size >= min(tab['P'] - 1, 1)
        for e in edges:   # the edge itself and the doubles beside it, each in its own cell
            y = np.array([np.nextafter(e, -np.inf), e, np.nextafter(e, np.inf)])
            k = np.clip(np.floor((y - y_lo) / cw), 0, C - 1).astype(int)
            assert (TE.score(tb, ta, y) <= U[k]).all(), (name, e)
    # arguments outside the range are clamped onto the edge cells' end points
    out = np.array([y_lo - 1.0, y_lo - 1e-9, y_hi + 1e-9, y_hi + 1.0])
    so = TE.score(tb, ta, out)
    assert (so[:2] <= U[0]).all() and (so[2:] <= U[-1]).all(), so


@pytest.mark.parametrize('name', CERTIFIED)
def test_no_hot_wave_tile_is_pruned(pairs, name):
    tb, ta, (w, mu, sg), (low, high, pm) = pairs[name]
    y = TE.draw_below(w, mu, sg, low, high, pm, DRAWS, np.random.RandomState(23))
    r = TE.prefilter(tb, ta, y)
    hot = ~(r['wmax'] < r['thr'])
    print(name, 'cells hot', int(r['hot'].sum()), 'intervals', len(r['intervals']),
          'wave tiles pruned', int(r['pruned'].sum()), 'of', r['pruned'].size, 'hot', int(hot.sum()))
    assert len(r['intervals']) <= TE.HOT_IV
    assert r['L0'] <= r['tab_max']
    assert not (r['pruned'] & hot).any(), int((r['pruned'] & hot).sum())
    assert r['pruned'].any()
    # a pruned wave tile's score is below the bound of every cell it touches
    assert (r['wmax'][r['pruned']] < r['L0'] - TE.TIE * max(1.0, abs(r['L0']))).all()


def test_all_hot_settings(pairs):
    """A non-finite pilot score, or the wide window of the tie tests, keeps
    every wave tile."""
    tb, ta, (w, mu, sg), (low, high, pm) = pairs['shape-u']
    U = TE.bound_lattice(tb, ta)
    y_lo, y_hi = tb['y_lo'], tb['y_lo'] + tb['width'] * tb['P']
    for L0 in (np.nan, np.inf, -np.inf):
        iv, hot = TE.hot_intervals(U, L0, y_lo, y_hi)
        assert iv == [(-np.inf, np.inf)] and hot.all()
    iv, hot = TE.hot_intervals(U, 1.0, y_lo, y_hi, tie=np.inf)
    assert iv == [(-np.inf, np.inf)] and hot.all()


def test_comb_lattice_takes_the_merge(pairs):
    """The comb's real lattice under a tie window of 1.0: more than HOT_IV
    runs are merged into exactly HOT_IV intervals, every hot cell stays
    covered, some wave tile is pruned and no hot one."""
    tb, ta, (w, mu, sg), (low, high, pm) = pairs['comb']
    y = TE.draw_below(w, mu, sg, low, high, pm, DRAWS, np.random.RandomState(23))
    r = TE.prefilter(tb, ta, y, tie=1.0)
    y_lo, y_hi = tb['y_lo'], tb['y_lo'] + tb['width'] * tb['P']
    cw = (y_hi - y_lo) / TE.CELLS
    raw = TE.hot_runs(r['hot'])
    print('comb, tie 1.0: cells hot', int(r['hot'].sum()), 'raw runs', raw, 'intervals',
          len(r['intervals']), 'wave tiles pruned', int(r['pruned'].sum()), 'of', r['pruned'].size)
    assert raw > TE.HOT_IV, raw
    assert len(r['intervals']) == TE.HOT_IV
    c = np.flatnonzero(r['hot']).astype(np.float64)
    mid = y_lo + cw * (c + 0.5)
    lo, hi = y_lo + cw * c, y_lo + cw * (c + 1.0)
    cov = np.zeros(c.size, dtype=bool)
    for a, b in r['intervals']:
        cov |= (a <= lo) & (hi <= b) & (a < mid) & (mid < b)
    assert cov.all(), c[~cov]
    hot = ~(r['wmax'] < r['thr'])
    assert r['pruned'].any() and not (r['pruned'] & hot).any()
    # and the default window leaves one run
    iv, hot_cells = TE.hot_intervals(r['U'], r['L0'], y_lo, y_hi)
    assert TE.hot_runs(hot_cells) == 1 and len(iv) == 1


def test_interval_merge_keeps_a_superset():
    """More than HOT_IV runs: the nearest are merged, every hot cell stays
    covered."""
    U = np.full(TE.CELLS, -1.0)
    hot_cells = [5, 100, 103, 400, 900, 1500, 1510, 2000, 2600, 3000, 3500, 4095]
    U[hot_cells] = 1.0
    iv, hot = TE.hot_intervals(U, 0.5, 0.0, 4096.0)
    assert len(iv) == TE.HOT_IV and np.flatnonzero(hot).tolist() == hot_cells
    for c in hot_cells:
        assert any(lo <= c and c + 1 <= hi for lo, hi in iv), c
    assert iv[-1][1] == np.inf
