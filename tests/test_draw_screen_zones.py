"""The zones of the screened draw (k_draw_zone) under the tail rank
and the half-tile widening, on the CPU through tools/table_error.py's
restatement (draw_zones, draw_screen): whatever the two rules leave, a sort
block that does not fall back has the full computation's layout; the defaults
keep config 4's fallbacks rare and invert fewer candidates than the whole-tile
rule with the end tiles' extremes as tail edges.
"""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import table_error as TE  # noqa: E402

CSRC = os.path.join(ROOT, 'hyperopt_amd', 'csrc')
TAIL, HALVES = 24, 4           # the engine's defaults (test_defaults_are_the_engines)
LAYOUT_DRAWS = 21 * 8192       # the pilot's sort block and 20 behind it
SHARE_DRAWS = 1 << 20          # ... and 127 behind it


def test_defaults_are_the_engines():
    text = open(os.path.join(CSRC, 'tpe_switches.hpp')).read()
    assert int(re.search(r'constexpr int64_t kDrawScreenTail = (\d+);', text).group(1)) == TAIL
    assert int(re.search(r'constexpr int64_t kDrawScreenHalves = (\d+);', text).group(1)) == HALVES


@pytest.fixture(scope='module')
def pairs():
    """(name, tb, ta, below mixture, low, high, centre) of config 4's hps 0, 40
    and 90 and of the named histories."""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    sys.path.insert(0, ROOT)
    import bench
    dom, losses, vals, act = bench.build_workload('cfg4')
    jobs = [('cfg4/%d' % i, losses, {h.label: vals[h.index] for h in dom.space.hps},
             dom.space.hps[i].label, ('uniform', (-5.0, 5.0))) for i in (0, 40, 90)]
    for name in ('low-edge', 'high-edge', 'band', 'comb'):
        l, cols, specs = TE.NAMED[name](6000)
        lab = next(iter(specs))
        jobs.append((name, l, cols, lab, specs[lab]))
    out = []
    for name, l, cols, lab, (dist, args) in jobs:
        cp = TE.certified_pair(l, cols, lab, dist, args)
        assert cp is not None, name
        tb, ta, mix, (low, high, center) = cp
        out.append((name, tb, ta, mix, low, high, center))
    return out


@pytest.fixture(scope='module')
def layout_draws(pairs):
    return [TE.draw_picks(*p[3], p[4], p[5], LAYOUT_DRAWS, np.random.RandomState(700 + j))
            for j, p in enumerate(pairs)]


@pytest.mark.parametrize('halves', [0, 3, 4])
@pytest.mark.parametrize('tail', [1, 24, 128])
def test_layout_under_every_rule(pairs, layout_draws, tail, halves):
    """No mismatch on any block that does not fall back: key range, kept mask,
    live buckets with their counts and bases, bucket bytes."""
    for (name, tb, ta, mix, low, high, center), (k, u1, x) in zip(pairs, layout_draws):
        r = TE.draw_screen(tb, ta, mix, low, high, center, k, u1, x, tail=tail, halves=halves)
        print('%-9s tail %3d halves %d: blocks %d fallback %d inverted %.4f'
              % (name, tail, halves, r['blocks'], r['fallback'], r['exact']))
        assert r['blocks'] == LAYOUT_DRAWS // 8192 - 1, name
        assert r['mismatch'] == [], (name, r['mismatch'][:3])


def test_tail_128_whole_tiles_is_the_rule_before():
    """draw_zones' defaults (and tail = 128 spelled out) are the zones of the
    tiles' extremes and the whole-tile widening."""
    rs = np.random.RandomState(3)
    pilot = rs.normal(0.0, 1.0, 8192)
    iv = [(-0.31, -0.29), (1.2, 1.25)]
    a = TE.draw_zones(pilot, iv, -4.0, 4.0, 0.0, 2)
    b = TE.draw_zones(pilot, iv, -4.0, 4.0, 0.0, 2, tail=128, halves=None)
    key = TE._block_bytes(pilot, pilot.min(), pilot.max())
    t = pilot[np.argsort(key, kind='stable')].reshape(-1, 128)
    for (la, ha), (lb, hb) in ((a, b),):
        np.testing.assert_array_equal(la, lb)
        np.testing.assert_array_equal(ha, hb)
    assert a[1][0] == t[0].max() and a[0][-1] == t[-1].min()
    # tail r: the r-th smallest of tile 0, the r-th largest of tile 63
    c = TE.draw_zones(pilot, iv, -4.0, 4.0, 0.0, 2, tail=24)
    assert c[1][0] == np.sort(t[0])[23] and c[0][-1] == np.sort(t[-1])[128 - 24]
    # the half-tile rule at 0: the interval itself, reaching no further than
    # the half tiles that hold its ends
    d = TE.draw_zones(pilot, iv, -4.0, 4.0, 0.0, 2, halves=0)
    h = pilot[np.argsort(key, kind='stable')].reshape(-1, 64)
    lo_half = h[np.flatnonzero(h.max(axis=1) >= iv[0][0])[0]]
    a0 = iv[0][0] - 8.0 * np.finfo(np.float64).eps * abs(iv[0][0])
    assert min(lo_half.min(), a0) in d[0]


@pytest.fixture(scope='module')
def shares(pairs):
    """Config 4's three hps at 2^20 draws: the defaults and (128, whole tiles x 2)."""
    out = {}
    for j, (name, tb, ta, mix, low, high, center) in enumerate(pairs):
        if not name.startswith('cfg4'):
            continue
        k, u1, x = TE.draw_picks(*mix, low, high, SHARE_DRAWS, np.random.RandomState(900 + j))
        new = TE.draw_screen(tb, ta, mix, low, high, center, k, u1, x, tail=TAIL, halves=HALVES)
        old = TE.draw_screen(tb, ta, mix, low, high, center, k, u1, x, 2)
        print('%-8s defaults: blocks %d fallback %d inverted %.4f; tail 128, tiles 2: fallback %d '
              'inverted %.4f' % (name, new['blocks'], new['fallback'], new['exact'],
                                 old['fallback'], old['exact']))
        out[name] = (new, old)
    assert len(out) == 3
    return out


def test_default_fallback_share(shares):
    """At most 2 % of the blocks of any of config 4's hps 0, 40, 90 fall back
    under the defaults (a condition on these inputs, not a measurement)."""
    for name, (new, _) in shares.items():
        assert new['blocks'] == SHARE_DRAWS // 8192 - 1 and new['mismatch'] == [], name
        assert new['fallback'] <= 0.02 * new['blocks'], (name, new['fallback'], new['blocks'])


def test_defaults_invert_fewer(shares):
    for name, (new, old) in shares.items():
        assert old['mismatch'] == [], name
        assert new['exact'] < old['exact'], (name, new['exact'], old['exact'])
