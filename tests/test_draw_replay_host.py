"""The host replay of the draws (tests/draw_replay.py) on the CPU: Philox
against the Random123 known answers, u53's layout, the conditions the cases of
tests/test_gpu_draw_replay.py must meet for a per-draw comparison to be
decidable, and the replay against tools/table_error.py's emulation of the
table inversion -- what tests/test_draw_screen.py already rests on.
"""
import numpy as np
import pytest

import draw_replay as R
from draw_replay import TE

# (counter; key) -> output, Random123's kat_vectors for philox4x32 10
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_philox_known_answers():
    for c, k, want in KAT:
        got = tuple(int(v) for v in R.philox4x32_10(*c, *k))
        assert got == want, (c, k, [hex(v) for v in got])
    # vectorised over the counters: the three vectors in one call
    c = np.array([v[0] for v in KAT], dtype=np.uint64).T
    k = np.array([v[1] for v in KAT], dtype=np.uint64).T
    got = np.array(R.philox4x32_10(*c, *k)).T
    assert (got == np.array([v[2] for v in KAT], dtype=np.uint64)).all()


def test_u53_layout():
    top = 2 ** 32 - 1
    assert R.u53(0, 0) == 0.0
    assert R.u53(top, top) == 1.0 - 2.0 ** -53
    # a's top 27 bits are the high part, b's top 26 the low part
    assert R.u53(1 << 31, 0) == 0.5
    assert R.u53(1 << 5, 0) == 2.0 ** -27
    assert R.u53(0, 1 << 6) == 2.0 ** -53
    assert R.u53(0, 1 << 31) == 2.0 ** -28
    # the dropped low bits (5 of a, 6 of b) do not matter
    rs = np.random.RandomState(0)
    a = rs.randint(0, 2 ** 32, 1000, dtype=np.uint64)
    b = rs.randint(0, 2 ** 32, 1000, dtype=np.uint64)
    assert (R.u53(a, b) == R.u53(a | np.uint64(31), b | np.uint64(63))).all()
    assert (R.u53(a, b) != R.u53(b, a)).mean() > 0.99


def test_uniforms_counter_layout():
    """gi's high word is counter word 1, the stream word 2, the iteration
    2 it / 2 it + 1 in word 3; the key is the seed's two halves."""
    seed, gi, stream, it = 0xa4093822299f31d0, (0x85a308d3 << 32) | 0x243f6a88, 0x13198a2e, 3
    u = R.uniforms(seed, np.array([gi], dtype=np.uint64), stream, it)
    a = R.philox4x32_10(0x243f6a88, 0x85a308d3, 0x13198a2e, 6, 0x299f31d0, 0xa4093822)
    b = R.philox4x32_10(0x243f6a88, 0x85a308d3, 0x13198a2e, 7, 0x299f31d0, 0xa4093822)
    want = (R.u53(a[0], a[1]), R.u53(a[2], a[3]), R.u53(b[0], b[1]), R.u53(b[2], b[3]))
    assert [float(v[0]) for v in u] == [float(v) for v in want]


def test_box_muller_reference():
    """The extended-precision normal against mpmath at 40 digits."""
    import mpmath
    rs = np.random.RandomState(1)
    u1 = np.floor(rs.random_sample(300) * 2.0 ** 53) * 2.0 ** -53
    u2 = np.floor(rs.random_sample(300) * 2.0 ** 53) * 2.0 ** -53
    u2[:8] = [0.0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875]
    u2[8:12] = [0.25 - 2.0 ** -53, 0.25 + 2.0 ** -53, 0.75 - 2.0 ** -53, 0.75 + 2.0 ** -53]
    z, r = R.box_muller(u1, u2)
    with mpmath.workdps(40):
        for a, b, zz, rr in zip(u1, u2, z, r):
            ref = mpmath.sqrt(-2 * mpmath.log1p(-mpmath.mpf(float(a)))) * mpmath.cospi(2 * mpmath.mpf(float(b)))
            hi = float(zz)                      # (z is wider than float64: two parts)
            got = mpmath.mpf(hi) + mpmath.mpf(float(zz - hi))
            assert abs(got - ref) <= 2.0 ** -60 * float(rr), (a, b)


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_gpu_case_is_decidable(name):
    """No ambiguous pick; few draws beside a rounding boundary; few deep ones."""
    c, r = R.CASES[name], R.case_replay(name)
    n = c['n']
    print('%-18s ambiguous_pick %d ambiguous_round %.2e deep %.2e spent %.4f tries max %d'
          % (name, r['ambiguous_pick'].sum(), r['ambiguous_round'].mean(), r['deep'].mean(),
             r['spent'].mean(), r['tries'].max()))
    assert c['seed'] >> 32 != 0 and R.STREAM != 0
    assert R.OFFSET < 2 ** 32 < R.OFFSET + n and R.SPLIT % 2 == 1
    assert r['ambiguous_pick'].sum() == 0
    assert r['ambiguous_round'].mean() <= 1e-3
    assert r['deep'].mean() <= 1e-3
    fam, w, mu, sigma, low, high, q = R.mixture(name)
    if fam != R.CAT and w.size > 1:
        assert sigma.max() / sigma.min() >= 16.0 or c['shape'] == 'std-normal'
    assert (w[r['k']] > 0.0).all()                # a zero-weight component is never picked


def test_modes_and_paths_are_hit():
    seen = set()
    for name in R.MODE_CASES:
        seen |= set(np.unique(R.case_replay(name)['mode']).tolist())
    assert seen == {0, 1, 2}
    # a few deep draws in both outer placements: the deep rule is exercised
    assert all(R.case_replay(name)['deep'].sum() >= 8 for name in ('gmm-above', 'gmm-below'))
    # the upper branch of mode 0 (q = 1 - Phi) and its lower one
    r = R.case_replay('gmm-in')
    m0 = r['mode'] == 0
    fam, w, mu, sigma, low, high, q = R.mixture('gmm-in')
    assert (m0 & (r['x'] > mu[r['k']])).any() and (m0 & (r['x'] < mu[r['k']])).any()
    # zero mass: the far components exist and are never picked
    fam, w, mu, sigma, low, high, q = R.mixture('gmm-zero-mass')
    mass = TE.draw_table(w, mu, sigma, low, high)[2]
    assert (mass == 0.0).sum() == 8 and (mass[R.case_replay('gmm-zero-mass')['k']] > 0.0).all()
    fam, w = R.mixture('gmm-zero-weight')[:2]
    assert (w == 0.0).sum() == 8
    for name in ('cat-4', 'cat-300', 'cat-2048', 'cat-2049'):
        p = R.mixture(name)[1]
        assert (p == 0.0).any() and (p[R.case_replay(name)['k']] > 0.0).all()
    # the rejection sampler: one try unbounded, several at half the mass, and
    # ~ (1 - 2e-4)^64 = 98.7 % of the draws out of budget between 3.5 and 4 sigma
    assert (R.case_replay('reject-unbounded')['tries'] == 1).all()
    half = R.case_replay('reject-half')
    assert 1.5 < half['tries'].mean() < 3.0 and half['tries'].max() >= 5 and not half['spent'].any()
    spent = R.case_replay('reject-spent')
    assert 0.98 <= spent['spent'].mean() <= 0.995
    assert (~spent['spent']).sum() >= 16          # and some accepted ones


@pytest.mark.parametrize('name', ['gmm-in', 'gmm-above', 'gmm-below', 'gmm-k1', 'gmm-k2048',
                                  'gmm-zero-weight', 'gmm-zero-mass'])
def test_replay_matches_table_emulation(name):
    """x* against draw_invert_emul at the replayed (k, u1): within
    kScreenMargin / 16 sigma for the draws that are not deep."""
    fam, w, mu, sigma, low, high, q = R.mixture(name)
    r = R.case_replay(name)
    k = r['k']
    _, base, mass, mode = TE.draw_table(w, mu, sigma, low, high)
    emul = TE.draw_invert_emul(base[k], mass[k], mode[k], mu[k], sigma[k], low, high, r['u1'])
    d = np.abs(emul - r['x']) / sigma[k]
    nd = ~r['deep']
    print('%-16s max |emul - x*| / sigma %.3e (not deep), %.3e (deep, %d draws)'
          % (name, d[nd].max(), d[~nd].max() if (~nd).any() else 0.0, (~nd).sum()))
    assert d[nd].max() <= R.screen_margin() / 16.0
    assert ((r['x'] >= low) & (r['x'] < high)).all()
    assert (emul[~nd] >= low).all() and (emul[~nd] < high).all()
