"""Every draw of tpe_sample against the host replay (tests/draw_replay.py).

Nothing here is statistical and nothing compares the device with itself: for
each of the shared cases the replay gives, per draw, the component, the exact
value x* and how far a correct device may be from it, and every one of the
2^16 draws (4096 on the rejection sampler) is held to that:

  bounded table draw, tail probability >= 2^-24
      |x - x*| <= kScreenMargin sigma_k + 4 spacing(|x*|) -- the property the
      draw screen's zone thresholds rely on (tpe_screen.hip zone_crossed);
  bounded table draw, deeper tail
      low <= x < high and finite only (erfcinv_fast's tail polynomial drifts
      there);
  Box-Muller draw (unbounded table draw, accepted rejection draw)
      |x - x*| <= 8 2^-52 (|mu_k| + sigma_k sqrt(-2 log(1 - u1))): 1 - u1 and
      2 u2 are exact, the library log, sqrt and cospi and the three arithmetic
      roundings stay under 5 ulp of the larger term, 8 is the margin
      test_gpu_anneal.py takes for the same functions;
  spent-budget draw (64 rejections)
      |x - x*| <= 8 2^-53 sigma / phi(z*) + 4 spacing(|x*|): the branch forms
      a + u3 (b - a) from values next to 1, a few 2^-53 absolute in
      probability, which the density turns into value;
  LGMM     the same on log x, plus 4 2^-52 relative for exp;
  quantized    x == rint(x* / q) q, either neighbour where x* / q is within the
      draw's tolerance of a half-integer;
  categorical  the replayed index exactly.

No pick is ambiguous in any case (tests/test_draw_replay_host.py), so a wrong
pick shows as a value far outside its bar; a failure names the component whose
value is nearest.  The seed has a nonzero high word, the stream is nonzero and
the offset 2^32 - 1000 takes the counter's high word through a change.
"""
import functools

import numpy as np
import pytest

from hyperopt_amd import _engine as E

import draw_replay as R

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
_MAXIMA = {}


def _sample(name, offset, n):
    fam, w, mu, sigma, low, high, q = R.mixture(name)
    return E.default_engine().sample(fam, w, mu, sigma, low=low, high=high, q=q,
                                     seed=R.CASES[name]['seed'], stream=R.STREAM, offset=offset, n=n)


@functools.lru_cache(maxsize=None)
def device_draws(name):
    x = _sample(name, R.OFFSET, R.CASES[name]['n'])
    x.setflags(write=False)
    return x


def _explain(name, r, x, i):
    """A failing draw: index, components, values, and the component whose
    value under the same uniforms is nearest to the device's."""
    fam = R.mixture(name)[0]
    msg = '%s draw %d: device %r, replay x* %r (value %r) of component %d, tol %.3e, u1 %r' % (
        name, i, x[i], r['x'][i], r['value'][i], r['k'][i], r['tol'][i], r['u1'][i])
    allx = R.all_component_values(name, r, i)
    if allx is not None:
        xd = np.log(x[i]) if fam == R.LGMM else x[i]
        j = int(np.nanargmin(np.abs(allx - xd)))
        msg += '; nearest component %d (x* %r)' % (j, allx[j])
    return msg


def _assert_all(ok, name, r, x):
    if not ok.all():
        bad = np.flatnonzero(~ok)
        raise AssertionError('%d of %d draws off: %s' % (bad.size, ok.size,
                                                          _explain(name, r, x, int(bad[0]))))


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_draws_equal_replay(name):
    fam, w, mu, sigma, low, high, q = R.mixture(name)
    r, x = R.case_replay(name), device_draws(name)
    deep = r['deep']
    worst = float('nan')
    _assert_all(np.isfinite(x), name, r, x)
    if fam == R.CAT:
        _assert_all(x == r['k'], name, r, x)
        assert (w[x.astype(np.int64)] > 0.0).all()      # a zero-probability category never appears
    elif q is not None:
        vs = np.exp(r['x']) if fam == R.LGMM else r['x']
        lo_n, hi_n = np.floor(vs / q) * q, np.ceil(vs / q) * q
        ok = (x == r['value']) | (r['ambiguous_round'] & ((x == lo_n) | (x == hi_n)))
        _assert_all(ok | deep, name, r, x)
        _assert_all(x == np.rint(x / q) * q, name, r, x)
        if low is not None:
            # (a value rounds to the lattice after the bounds are applied)
            lv, hv = (np.exp(low), np.exp(high)) if fam == R.LGMM else (low, high)
            _assert_all((x >= np.rint(lv / q) * q) & (x <= np.rint(hv / q) * q), name, r, x)
    else:
        xd = np.log(x) if fam == R.LGMM else x
        d = np.abs(xd - r['x'])
        tol = r['tol']
        if fam == R.LGMM:
            # exp's 4 2^-52 relative, and this test's own log (an ulp of |x*|)
            tol = tol + 4.0 * EPS + np.spacing(np.abs(r['x']))
        _assert_all((d <= tol) | deep, name, r, x)
        worst = float((d / r['sigma'])[~deep].max())
        if low is not None and fam == R.GMM:
            _assert_all((x >= low) & (x < high), name, r, x)
        elif low is not None:
            # log x in [low, high) up to exp's error (4 2^-52) and numpy's (an ulp)
            _assert_all((x >= np.exp(low) * (1.0 - 5.0 * EPS)) &
                        (x <= np.exp(high) * (1.0 + 5.0 * EPS)), name, r, x)
    if name == 'reject-spent':
        # acceptance is 2e-4 a try: ~98.7 % of the draws spend the 64 tries
        assert r['spent'].mean() >= 0.98
    line = '%-18s max |x - x*| / sigma %s  deep %.2e  spent %.4f' % (
        name, 'exact    ' if worst != worst else '%.3e' % worst, deep.mean(), r['spent'].mean())
    print(line)
    _MAXIMA[name] = line
    if len(_MAXIMA) == len(R.CASES):
        R.record_profile('draws against the host replay', [_MAXIMA[k] for k in sorted(_MAXIMA)])


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_split_call_gives_the_same_bits(name):
    """The call split at an odd offset concatenates to the whole call's bits."""
    n = R.CASES[name]['n']
    a = _sample(name, R.OFFSET, R.SPLIT if n > R.SPLIT else 1001)
    b = _sample(name, R.OFFSET + a.size, n - a.size)
    got = np.concatenate([a, b]).view(np.uint64)
    assert (got == device_draws(name).view(np.uint64)).all()
