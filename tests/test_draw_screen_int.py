"""The integer screen (k_draw_sorted_screen_int) on the CPU,
through tools/table_error.py's restatement: the pick boundaries B against the
float predicate they bisect, the guide pick against pick_cdf and the ladder,
the guide's validity rule, the integer edge thresholds against the float ones,
and whole sort blocks (draw_screen) with the integer pick against the float
pick.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import table_error as TE  # noqa: E402

ONE53 = 1 << 53


def _tables():
    """name -> inclusive CDF of the pick weights (K = 1, 2, 26, 32)."""
    rs = np.random.RandomState(11)
    w = {}
    w['one'] = np.array([0.7])
    w['two'] = np.array([0.3, 0.9])
    w['equal26'] = np.ones(26)
    w['equal32'] = np.ones(32) / 32.0
    w['random26'] = rs.uniform(0.2, 1.0, 26)
    w['random32'] = rs.gamma(2.0, 1.0, 32) + 0.05
    t = np.ones(26)
    t[9] = 26.0 * 2.0 ** -13           # under 2^-12 of the total: two boundaries in one G = 9 bucket
    w['tiny26'] = t
    z = np.ones(32)
    z[[12, 13]] = 0.0                  # two adjacent zero-mass components: tied boundaries
    w['zeros32'] = z
    z = rs.uniform(0.5, 1.0, 26)
    z[[0, 1]] = 0.0                    # ... at the front (B = 0 twice)
    z[[24, 25]] = 0.0                  # ... and at the back (B = 2^53)
    w['zeros26'] = z
    return {k: np.cumsum(v) for k, v in w.items()}


TABLES = _tables()


@pytest.fixture(scope='module')
def boundaries():
    return {name: TE.pick_thresholds(cdf) for name, cdf in TABLES.items()}


def test_tables_are_the_named_shapes(boundaries):
    assert sorted({c.size for c in TABLES.values()}) == [1, 2, 26, 32]
    B = boundaries['zeros32']
    assert B[11] == B[12] == B[13] and B[10] < B[11] < B[14]
    B = boundaries['zeros26']
    assert B[0] == B[1] == 0 and B[23] == B[24] == ONE53
    B = boundaries['tiny26']
    assert 0 < B[9] - B[8] < 1 << (53 - 12) and (B[8] >> (53 - 9)) == (B[9] >> (53 - 9))


@pytest.mark.parametrize('name', sorted(TABLES))
def test_pick_boundaries_bisect_the_float_predicate(boundaries, name):
    """B is nondecreasing, 2^53 from K - 1 up, and for every B[j] strictly
    between 0 and 2^53 the draw's own test is false at B[j] - 1 and true at B[j]."""
    cdf, B = TABLES[name], boundaries[name]
    K = cdf.size
    assert B.shape == (K,) and B.dtype == np.uint64 and B[K - 1] == ONE53
    assert (np.diff(B.astype(np.int64)) >= 0).all()
    seen = 0
    for j in range(K - 1):
        b = int(B[j])
        if 0 < b < ONE53:
            seen += 1
            assert not TE.pick_predicate(cdf, j, np.uint64(b - 1)), (name, j)
            assert TE.pick_predicate(cdf, j, np.uint64(b)), (name, j)
        elif b == 0:
            assert TE.pick_predicate(cdf, j, np.uint64(0)), (name, j)
        else:
            assert not TE.pick_predicate(cdf, j, np.uint64(ONE53 - 1)), (name, j)
    assert seen > 0 or K <= 1


def _probe(B, gbits, rs):
    """Every boundary and its neighbours, every bucket's first and last U0, the
    ends of the range, and 1e5 random U0."""
    sh = 53 - gbits
    first = np.arange(1 << gbits, dtype=np.int64) << sh
    b = B.astype(np.int64)
    u = np.concatenate([b, b - 1, b + 1, first, first + (1 << sh) - 1, [0, ONE53 - 1],
                        rs.randint(0, ONE53, 100000)])
    return np.unique(u[(u >= 0) & (u < ONE53)]).astype(np.uint64)


@pytest.mark.parametrize('gbits', [0, 4, 9, 12])
def test_guide_pick_is_the_float_pick(boundaries, gbits):
    """Where the guide is valid its pick equals pick_cdf's and the ladder's."""
    rs = np.random.RandomState(100 + gbits)
    valid = []
    for name, cdf in sorted(TABLES.items()):
        if gbits == 0 and cdf.size > 2:
            continue
        g = TE.guide_table(cdf, gbits)
        assert (g['B'] == boundaries[name]).all()
        if not g['valid']:
            continue
        valid.append(name)
        U0 = _probe(g['B'], gbits, rs)
        k = TE.guide_pick(g, U0)
        np.testing.assert_array_equal(k, TE.pick_cdf_emul(cdf, U0), err_msg=name)
        np.testing.assert_array_equal(k, TE.pick_ladder_emul(cdf, U0), err_msg=name)
        assert k.min() == 0 or name.startswith('zeros')
        assert k.max() <= cdf.size - 1
    print('G = %d: valid %s' % (gbits, valid))
    assert 'one' in valid and 'two' in valid
    if gbits >= 9:
        assert {'equal26', 'equal32', 'zeros32', 'zeros26'} <= set(valid)


@pytest.mark.parametrize('gbits', [0, 4, 9, 12])
def test_guide_validity(boundaries, gbits):
    """Not valid exactly when some bucket holds two distinct boundaries
    strictly inside it (ties are fine), or the table is not a CDF."""
    for name, cdf in sorted(TABLES.items()):
        g = TE.guide_table(cdf, gbits)
        B = [int(b) for b in boundaries[name][:-1]]
        sh = 53 - gbits
        two = False
        for b in range(1 << gbits):
            inner = {v for v in B if (b << sh) < v < ((b + 1) << sh)}
            two |= len(inner) > 1
        assert g['valid'] == (not two), (name, gbits)
        if gbits == 0:
            assert g['valid'] == (len({v for v in B if 0 < v < ONE53}) <= 1), name
    if gbits == 9:
        assert not TE.guide_table(TABLES['tiny26'], 9)['valid']
        assert TE.guide_table(TABLES['zeros32'], 9)['valid']
    if gbits == 12:
        assert not TE.guide_table(TABLES['tiny26'], 12)['valid']
    for bad in (np.array([0.2, np.nan, 0.9]), np.array([0.5, 0.4, 0.9]), np.array([0.0, 0.0]),
                np.array([0.2, np.inf])):
        assert not TE.guide_table(bad, gbits)['valid']


@pytest.fixture(scope='module')
def below_mixture():
    losses, cols, specs = TE.test_shape()
    fit, (low, high, _) = TE.mixtures(losses, cols, 'u', *specs['u'], **TE.fit_params('default'))
    return fit[0] + (low, high)


def test_integer_edge_thresholds(below_mixture):
    """U1 >= thrI iff u1 >= thr, on every threshold and one step on each side."""
    w, mu, sg, low, high = below_mixture
    span = high - low
    zlo = np.array([-np.inf, low + 0.30 * span, low + 0.70 * span, high - 0.02 * span])
    zhi = np.array([low + 0.02 * span, low + 0.31 * span, low + 0.7004 * span, np.inf])
    _, base, mass, mode = TE.draw_table(w, mu, sg, low, high)
    thr = TE.zone_thresholds(zlo, zhi, base, mass, mode, mu, sg)
    thr_i = TE.zone_thresholds(zlo, zhi, base, mass, mode, mu, sg, integer=True)
    assert thr_i.dtype == np.uint64 and thr_i.shape == thr.shape
    assert (thr_i.astype(np.float64) * 2.0 ** -53 == thr).all()
    assert ((thr == 1.0) == (thr_i == ONE53)).all()
    assert (thr_i < ONE53).any()
    t = thr_i.astype(np.int64)
    for d in (-1, 0, 1):
        U1 = np.clip(t + d, 0, ONE53 - 1)
        u1 = U1.astype(np.float64) * 2.0 ** -53
        for e in range(thr.shape[1]):
            np.testing.assert_array_equal(U1[:, [e]].astype(np.uint64) >= thr_i, u1[:, [e]] >= thr)


DRAWS = 21 * 8192          # (tests/test_draw_screen.py's)


def test_screened_blocks_with_the_integer_pick():
    """draw_screen with the guide pick and the integer thresholds: the blocks,
    fall-backs and inverted shares of the float pick, no mismatch, on the
    shapes tests/test_draw_screen.py uses."""
    sys.path.insert(0, ROOT)
    import bench
    dom, losses, vals, act = bench.build_workload('cfg4')
    jobs = [('cfg4/%d' % i, losses, {h.label: vals[h.index] for h in dom.space.hps},
             dom.space.hps[i].label, ('uniform', (-5.0, 5.0))) for i in (0, 40, 90)]
    for name in ('low-edge', 'high-edge', 'band', 'comb'):
        l, cols, specs = TE.NAMED[name](6000)
        lab = next(iter(specs))
        jobs.append((name, l, cols, lab, specs[lab]))
    screened = 0
    for j, (name, l, cols, lab, (dist, args)) in enumerate(jobs):
        tb, ta, mix, (low, high, center) = TE.certified_pair(l, cols, lab, dist, args)
        k, u1, x, U0, U1 = TE.draw_picks(*mix, low, high, DRAWS, np.random.RandomState(700 + j),
                                         integers=True)
        assert (U1.astype(np.float64) * 2.0 ** -53 == u1).all()
        for tiles in (2, 0):
            f = TE.draw_screen(tb, ta, mix, low, high, center, k, u1, x, tiles)
            i = TE.draw_screen(tb, ta, mix, low, high, center, k, u1, x, tiles, integers=(U0, U1))
            print('%-9s tiles %d: blocks %d fallback %d inverted %.4f' % (name, tiles, i['blocks'],
                                                                          i['fallback'], i['exact']))
            assert i['valid'] and i['pick_mismatch'] == 0, name
            assert i['mismatch'] == [] and f['mismatch'] == [], name
            assert (i['blocks'], i['fallback'], i['exact']) == (f['blocks'], f['fallback'], f['exact'])
            screened += i['blocks'] - i['fallback']
        g0 = TE.draw_screen(tb, ta, mix, low, high, center, k, u1, x, 2, integers=(U0, U1), gbits=0)
        assert len(mix[0]) > 2 and not g0['valid'] and g0['blocks'] == 0, name
    assert screened > 0
