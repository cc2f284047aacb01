"""The device math helpers on given arguments (tpe_math_probe): fast_log and
fast_log2 (tpe_device.hpp) against mpmath at 50 digits, erfcinv_fast
(tpe_draw.hpp) against scipy and against tools/table_error.py's emulation of
it -- the hardware's share of the draw screen's margin, measured instead of
assumed -- and the library erfc against mpmath at the relative error
tpe_screen.hip's zone_crossed takes for it (rho).

The bars: 3 ulp of the correctly rounded logarithm, kScreenMargin
sigma for sqrt2 |erfcinv_fast - erfcinv| over the tail probabilities the screen
covers, kScreenMargin less the emulation's own worst error for sqrt2
|erfcinv_fast - emulation|, 4e-7 relative past the fp64 hand-off (the figure of
erfcinv_fast's comment), 1e-13 relative for erfc.
"""
import numpy as np
import pytest

from hyperopt_amd import _engine as E

import draw_replay as R
from draw_replay import TE

pytestmark = pytest.mark.gpu

FAST_LOG, FAST_LOG2, ERFCINV_FAST, ERFC = 0, 1, 2, 3
ULP_BAR = 3.0
RHO = 1e-13
SQRT2 = 1.4142135623730951
SQRT_HALF = 0.70710678118654752440


def probe(which, x):
    return E.default_engine().math_probe(which, x)


def _beside(v, n=4):
    """The n doubles on each side of v."""
    out, lo, hi = [], v, v
    for _ in range(n):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return out


def log_arguments():
    rs = np.random.RandomState(20)
    parts = [
        # log-uniform over every finite positive double, subnormals included
        np.ldexp(rs.uniform(1.0, 2.0, 20000), rs.randint(-1074, 1023, 20000)),
        rs.randint(1, 2 ** 52, 10000, dtype=np.int64).view(np.float64),      # subnormals
        rs.uniform(0.5, 2.0, 20000),
        np.array([1.0 + s * 2.0 ** -j for j in range(1, 53) for s in (1.0, -1.0)]),
        np.ldexp(1.0, np.arange(-1074, 1024)),
        # the mantissa fold at sqrt(1/2) 2^k
        np.array([v for k in (-1070, -1023, -1022, -500, -52, -1, 0, 1, 2, 53, 500, 1023)
                  for v in _beside(float(np.ldexp(SQRT_HALF, k)))]),
    ]
    x = np.concatenate(parts)
    assert ((x > 0.0) & np.isfinite(x)).all() and x.size <= 55000
    return x


@pytest.fixture(scope='module')
def log_reference():
    """(x, log x, log2 x) with the logarithms as mpmath numbers at 50 digits."""
    import mpmath
    x = log_arguments()
    with mpmath.workdps(50):
        ln2 = mpmath.log(2)
        ln = [mpmath.log(mpmath.mpf(float(v))) for v in x]
        l2 = [v / ln2 for v in ln]
    return x, ln, l2


def _ulp_errors(got, ref):
    """|got - ref| in ulps of the correctly rounded ref."""
    import mpmath
    out = np.empty(got.size)
    with mpmath.workdps(50):
        for i, (g, r) in enumerate(zip(got, ref)):
            out[i] = float(abs(mpmath.mpf(float(g)) - r) / float(np.spacing(abs(float(r))))) \
                if np.isfinite(g) else np.inf
    return out


@pytest.mark.parametrize('which', [FAST_LOG, FAST_LOG2])
def test_fast_log_within_three_ulp(log_reference, which):
    x, ln, l2 = log_reference
    name = 'fast_log2' if which == FAST_LOG2 else 'fast_log'
    got = probe(which, x)
    err = _ulp_errors(got, l2 if which == FAST_LOG2 else ln)
    sub = x < 2.0 ** -1022
    near = (x >= 0.5) & (x <= 2.0)
    lines = ['%-9s max error %.3f ulp at x = %r (%d arguments)' % (name, err.max(),
                                                                  float(x[np.argmax(err)]), x.size),
             '%-9s   subnormal arguments %.3f ulp, [0.5, 2] %.3f ulp, the rest %.3f ulp'
             % (name, err[sub].max(), err[near].max(), err[~sub & ~near].max())]
    print('\n'.join(lines))
    R.record_profile(name, lines)
    assert err.max() <= ULP_BAR, float(x[np.argmax(err)])


def test_fast_log_exact_results():
    k = np.arange(-1074, 1024)
    got = probe(FAST_LOG2, np.ldexp(1.0, k))
    assert (got == k).all(), k[got != k][:5]
    assert probe(FAST_LOG, [1.0])[0] == 0.0 and probe(FAST_LOG2, [1.0])[0] == 0.0
    # zero, infinite and NaN arguments take the library's results: numpy's bits
    _assert_numpy_bits(np.array([0.0, -0.0, np.inf, np.nan]))


def _assert_numpy_bits(x):
    with np.errstate(all='ignore'):
        for which, fn in ((FAST_LOG, np.log), (FAST_LOG2, np.log2)):
            got, want = probe(which, x).view(np.uint64), fn(x).view(np.uint64)
            print(which, [hex(v) for v in got], [hex(v) for v in want])
            assert (got == want).all(), ([hex(v) for v in got], [hex(v) for v in want])


def test_fast_log_negative_arguments_give_numpy_bits():
    """Negative arguments: the bits np.log / np.log2 give on the reference's
    platform, 0xfff8000000000000 -- the default NaN of an invalid x86
    operation, sign set.  (The library log alone returns the quiet NaN with
    the sign clear; fast_log / fast_log2 return numpy's.)"""
    _assert_numpy_bits(np.array([-1.0, -2.0 ** -1074, -np.inf]))


def test_probe_arguments():
    eng = E.default_engine()
    with pytest.raises(ValueError):
        eng.math_probe(4, [1.0])
    with pytest.raises(ValueError):
        eng.math_probe(-1, [1.0])
    assert eng.math_probe(FAST_LOG, np.zeros(0)).size == 0
    x = np.linspace(1.0, 2.0, 257).reshape(1, 257)          # one thread past a block
    assert eng.math_probe(ERFC, x).shape == (1, 257)


@pytest.fixture(scope='module')
def erfcinv_grid():
    """DESIGN 8's grid (sorted), its device values, scipy's and the emulation's."""
    from scipy.special import erfcinv
    y = TE.erfcinv_grid()
    if y.size % 64 == 0:
        y = y[:-1]
    return y, probe(ERFCINV_FAST, y), erfcinv(y), TE.erfcinv_fast_emul(y), -np.log(y * (2.0 - y))


def test_erfcinv_fast_bounds(erfcinv_grid):
    y, dev, ref, emul, w = erfcinv_grid
    margin = R.screen_margin()
    worst = max(e for _, e, _ in TE.invert_error()[:2])
    assert y.size >= 700000 and (y <= 1.0).all() and y.max() == 1.0
    assert np.isfinite(dev).all() and (dev >= 0.0).all()
    et, ee = SQRT2 * np.abs(dev - ref), SQRT2 * np.abs(dev - emul)
    central, screened = w < 5.0, (w >= 5.0) & (w <= TE.SCREEN_W_MAX)
    drift = (w > TE.SCREEN_W_MAX) & (w <= 35.5)
    band = (w > 35.5) & (w <= 36.5)
    far = w > 36.5
    assert central.any() and screened.any() and drift.any() and band.any() and far.any()
    rel = np.abs(dev[far] - ref[far]) / ref[far]
    lines = ['erfcinv_fast, sqrt2 |device - x| in sigma, x = erfcinv (scipy) / the numpy emulation:']
    for lab, sel in (('w < 5 (central)', central),
                     ('5 <= w <= %.2f (screened tail)' % TE.SCREEN_W_MAX, screened),
                     ('%.2f < w <= 35.5 (tail, never cold)' % TE.SCREEN_W_MAX, drift)):
        lines.append('  %-36s %.3e / %.3e' % (lab, et[sel].max(), ee[sel].max()))
    lines.append('  w > 36.5 (fp64 hand-off)              %.3e relative' % rel.max())
    lines.append('  emulation against erfcinv, w <= %.2f: %.3e; kScreenMargin %.3e'
                 % (TE.SCREEN_W_MAX, worst, margin))
    print('\n'.join(lines))
    R.record_profile('erfcinv_fast', lines)
    cov = central | screened
    assert et[cov].max() <= margin
    assert ee[cov].max() <= margin - worst
    assert ee[drift].max() <= margin - worst
    assert rel.max() <= 4e-7
    assert (dev[band] > 0.0).all()
    assert probe(ERFCINV_FAST, [1.0])[0] == 0.0


def test_erfcinv_fast_is_independent_of_the_wave(erfcinv_grid):
    """Sorted, the grid's waves are all central or all in the tail; permuted,
    nearly every wave mixes both (the tail polynomial is evaluated when some
    lane of the wave needs it): the same bits per value."""
    y, dev = erfcinv_grid[:2]
    assert y.size % 64 != 0 and (np.diff(y) > 0.0).all()
    perm = np.random.RandomState(21).permutation(y.size)
    tail = y[perm] * (2.0 - y[perm]) < np.exp(-5.0)
    waves = tail[:tail.size // 64 * 64].reshape(-1, 64)
    mixed = waves.any(axis=1) & ~waves.all(axis=1)
    assert mixed.mean() > 0.9
    got = probe(ERFCINV_FAST, y[perm])
    assert (got.view(np.uint64) == dev[perm].view(np.uint64)).all()


def test_erfc_relative_error():
    """Every argument the zone kernel can form with tail >= kScreenQMin:
    erfc(3.8) / 2 < 2^-24 < erfc(-6) / 2."""
    import mpmath
    rs = np.random.RandomState(22)
    x = np.concatenate([rs.uniform(-6.0, 3.8, 39990), [-6.0, 3.8, 0.0, -0.0, 2.0 ** -1074],
                        _beside(0.0, 1), [0.5, 1.0, -1.0]])
    assert x.size <= 40000
    got = probe(ERFC, x)
    with mpmath.workdps(50):
        rel = np.array([float(abs(mpmath.mpf(float(g)) / mpmath.erfc(mpmath.mpf(float(v))) - 1))
                        for g, v in zip(got, x)])
    lines = ['erfc      max relative error %.3e at x = %r over [-6, 3.8] (%d arguments); rho %.1e'
             % (rel.max(), float(x[np.argmax(rel)]), x.size, RHO)]
    print(lines[0])
    R.record_profile('erfc', lines)
    assert rel.max() <= RHO
