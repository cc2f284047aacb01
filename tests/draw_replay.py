"""Host replay of the engine's draws (tpe_draw.hpp; tpe_sample): Philox4x32-10
and u53 in numpy, then draw_table_value / draw_one step by step with the
device's approximations (erfcinv_fast, the library erfc / erfinv / log /
cospi) replaced by exact functions (scipy in float64, extended precision for
the Box-Muller normal).  The result of `replay` is what a draw must be, with
the distance a correct device may be off (`tol`), so a GPU test needs no
statistics: every single draw is checked (tests/test_gpu_draw_replay.py), and
tests/test_draw_replay_host.py ties the replay to known answers and to
tools/table_error.py's emulation on the CPU.

numpy, scipy and mpmath only; nothing here touches the engine.
"""
import math
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import table_error as TE  # noqa: E402

GMM, LGMM, CAT = 0, 1, 2
TAB_CAP = 2048            # kTabCap: larger mixtures take the rejection sampler
REJECT_TRIES = 64         # draw_one's budget
DEEP_Q = 2.0 ** -24       # below it erfcinv_fast's tail polynomial drifts
PICK_RTOL = 1e-12         # scan orders differ: 2048 additions stay under it
EPS = 2.0 ** -52

_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def screen_margin():
    """kScreenMargin of the engine (tests/test_draw_screen.py's regex)."""
    src = open(os.path.join(ROOT, 'hyperopt_amd', 'csrc', 'tpe_internal.hpp')).read()
    m = re.search(r'constexpr double %s = ([^;]+);' % 'kScreenMargin', src)
    return float.fromhex(m.group(1)) if m.group(1).startswith('0x') else float(m.group(1))


PROFILE = os.path.join(ROOT, 'profiles', 'device_math.txt')


def record_profile(section, lines):
    """With TPE_RECORD_PROFILES=1, put the measured maxima of a GPU test into
    its section of profiles/device_math.txt (other sections stay); a normal
    test run writes nothing."""
    if os.environ.get('TPE_RECORD_PROFILES', '') != '1':
        return
    sections, cur = {}, None
    if os.path.exists(PROFILE):
        for ln in open(PROFILE).read().splitlines():
            if ln.startswith('[') and ln.endswith(']'):
                cur = ln[1:-1]
                sections[cur] = []
            elif cur is not None and ln:
                sections[cur].append(ln)
    sections[section] = list(lines)
    os.makedirs(os.path.dirname(PROFILE), exist_ok=True)
    with open(PROFILE, 'w') as f:
        f.write('# Measured on an MI355X by tests/test_gpu_device_math.py and\n'
                '# tests/test_gpu_draw_replay.py (TPE_RECORD_PROFILES=1 pytest -m gpu ...).\n')
        for name in sorted(sections):
            f.write('\n[%s]\n%s\n' % (name, '\n'.join(sections[name])))


# ---------------------------------------------------------------------------
# Philox4x32-10 and the uniforms of a draw
# ---------------------------------------------------------------------------
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32 with 10 rounds (Salmon et al., SC'11) as philox() of
    tpe_draw.hpp computes it: four uint32 words per counter, vectorised over
    the counters (every argument broadcasts)."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(
        *(np.asarray(v, dtype=np.uint64) & _M32 for v in (c0, c1, c2, c3, k0, k1)))
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2            # 32 x 32 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _M32, (p0 >> _S32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + w0) & _M32, (k1 + w1) & _M32
    return c0, c1, c2, c3


def u53(a, b):
    """The uniform in [0, 1) of two Philox words: the top 27 bits of a, then
    the top 26 of b, over 2^53 (exact in float64)."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    hi, lo = (a >> np.uint64(5)).astype(np.float64), (b >> np.uint64(6)).astype(np.float64)
    return (hi * 67108864.0 + lo) * (1.0 / 9007199254740992.0)


def uniforms(seed, gi, stream, it=0):
    """(u0, u1, u2, u3) of draw4(seed, gi, stream, it): blocks with counter
    word 3 = 2 it and 2 it + 1, counter = (gi low, gi high, stream), key =
    (seed low, seed high).  (draw_block0 is the first block of it = 0.)"""
    gi = np.asarray(gi, dtype=np.uint64)
    seed = int(seed) & (2 ** 64 - 1)
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    glo, ghi = gi & _M32, gi >> _S32
    st = int(stream) & 0xFFFFFFFF
    a = philox4x32_10(glo, ghi, st, 2 * int(it), k0, k1)
    b = philox4x32_10(glo, ghi, st, 2 * int(it) + 1, k0, k1)
    return u53(a[0], a[1]), u53(a[2], a[3]), u53(b[0], b[1]), u53(b[2], b[3])


# ---------------------------------------------------------------------------
# exact pieces
# ---------------------------------------------------------------------------
_LD = np.longdouble
_WIDE = np.finfo(_LD).nmant >= 63     # x87 extended: 11 bits past float64


def box_muller(u1, u2):
    """(z, r): z = sqrt(-2 log(1 - u1)) cos(2 pi u2) and its radius r, z to
    well under a float64 ulp (extended precision behind an exact octant
    reduction of u2; mpmath where long double is no wider than double)."""
    u1, u2 = np.asarray(u1, dtype=np.float64), np.asarray(u2, dtype=np.float64)
    r = np.sqrt(-2.0 * np.log1p(-u1))
    if not _WIDE:
        import mpmath
        with mpmath.workprec(120):
            z = [mpmath.sqrt(-2 * mpmath.log1p(-mpmath.mpf(float(a)))) *
                 mpmath.cospi(2 * mpmath.mpf(float(b))) for a, b in zip(u1.ravel(), u2.ravel())]
            return np.array([z_ for z_ in z], dtype=object).reshape(u1.shape), r
    # cos(pi t), t = 2 u2 in [0, 2): every step of the reduction is exact
    t = 2.0 * u2
    t = np.where(t > 1.0, 2.0 - t, t)            # cos(pi (2 - t)) = cos(pi t)
    neg = t > 0.5
    t = np.where(neg, 1.0 - t, t)                # cos(pi (1 - t)) = -cos(pi t)
    pi = _LD('3.14159265358979323846264338327950288')
    tl = t.astype(_LD)
    c = np.where(t <= 0.25, np.cos(pi * tl), np.sin(pi * (_LD(0.5) - tl)))
    c = np.where(neg, -c, c)
    rl = np.sqrt(_LD(-2.0) * np.log1p(-u1.astype(_LD)))
    return rl * c, r


def _affine(mu, sigma, z):
    """mu + sigma z rounded once to float64 (z from box_muller)."""
    if z.dtype == object:
        import mpmath
        return np.array([float(mpmath.mpf(float(m)) + mpmath.mpf(float(s)) * zz)
                         for m, s, zz in zip(mu.ravel(), sigma.ravel(), z.ravel())]).reshape(z.shape)
    return (mu.astype(_LD) + sigma.astype(_LD) * z).astype(np.float64)


def truncated_quantile(base, mass, mode, mu, sigma, low, high, u):
    """draw_table_value's bounded branch with exact functions: the tail
    probability q the inversion sees by build_table's three-way rule, then
    x = mu +- sqrt2 sigma erfcinv(2 q), clipped to [low, nextafter(high, -inf)].
    Returns (x, q, side)."""
    from scipy.special import erfcinv
    um = u * mass
    pu, pp = base - um, base + um
    lower = (mode != 1) & ((mode == 2) | (pp < 0.5))
    q = np.where(mode == 1, pu, np.where(lower, pp, 1.0 - pp))
    side = np.where(lower, -1.0, 1.0)
    with np.errstate(all='ignore'):
        e = np.where(q > 0.0, erfcinv(np.where(q > 0.0, 2.0 * q, 1.0)), np.inf)
        x = mu + side * (1.4142135623730951 * sigma) * e
    x = np.where(x >= low, x, low)
    x = np.where(x < high, x, np.nextafter(high, -np.inf))
    return x, q, side


def _pick(cdf, t):
    """(k, ambiguous): the first k with cdf[k] > t, capped at K - 1, and
    whether t lies within PICK_RTOL cdf[-1] of a boundary beside k."""
    K = cdf.size
    k = np.minimum(np.searchsorted(cdf, t, side='right'), K - 1)
    d = np.full(t.shape, np.inf)
    up = k < K - 1
    d[up] = np.abs(cdf[k[up]] - t[up])
    dn = k > 0
    d[dn] = np.minimum(d[dn], np.abs(cdf[k[dn] - 1] - t[dn]))
    return k, d <= PICK_RTOL * cdf[-1]


# ---------------------------------------------------------------------------
# the replay
# ---------------------------------------------------------------------------
def replay(family, w, mu, sigma, low, high, q, seed, stream, offset, n):
    """Draws offset .. offset + n - 1 of tpe_sample(family, w, mu, sigma, low,
    high, q, seed, stream): a dict of arrays [n]
      k        the picked component (the last pick of the rejection sampler)
      x        the exact value x* in the mixture's domain (log x for LGMM,
               before quantization); the index for a categorical
      value    what tpe_sample returns for x* (exp, rint(x / q) q applied)
      sigma    sigma of component k
      q        the tail probability the table inversion sees (NaN elsewhere)
      u1       the uniform behind the value (u3 for a spent-budget draw)
      tol      how far a correct device value may lie from x*, in x's domain
               (the bars of tests/test_gpu_draw_replay.py; 0 for categoricals,
               inf for deep draws, which are only bounded)
      tries    rejection iterations used (1 on the table path)
      ambiguous_pick   u0 cdf_last within 1e-12 cdf_last of a pick boundary, or
                       a rejection test within tol of a bound
      ambiguous_round  x* / q within the draw's tolerance of a half-integer
      deep     bounded table draw with q < 2^-24
      spent    the rejection budget ran out (truncated inverse CDF at u3)
      table    drawn by the table sampler (K <= 2048)
    low / high: None for an unbounded mixture (log-space for LGMM); q: None
    for an unquantized one."""
    w = np.asarray(w, dtype=np.float64)
    K = w.size
    gi = (np.uint64(offset) + np.arange(n, dtype=np.uint64))
    bounded = family != CAT and low is not None
    table = K <= TAB_CAP
    out = dict(k=np.zeros(n, dtype=np.int64), x=np.zeros(n), value=np.zeros(n), sigma=np.ones(n),
               q=np.full(n, np.nan), u1=np.zeros(n), tol=np.zeros(n),
               tries=np.ones(n, dtype=np.int64), ambiguous_pick=np.zeros(n, dtype=bool),
               ambiguous_round=np.zeros(n, dtype=bool), deep=np.zeros(n, dtype=bool),
               spent=np.zeros(n, dtype=bool), table=np.full(n, table))
    if family == CAT:
        u0 = uniforms(seed, gi, stream, 0)[0]
        cdf = np.cumsum(w)
        # (table: u0 cdf[K-1] of the block scan; rejection path: u0 wsum, the
        # pairwise sum -- both within PICK_RTOL of this one)
        k, amb = _pick(cdf, u0 * cdf[-1])
        out.update(k=k, x=k.astype(np.float64), value=k.astype(np.float64), ambiguous_pick=amb)
        return out
    mu, sigma = np.asarray(mu, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    if table:
        u0, u1, u2, _ = uniforms(seed, gi, stream, 0)
        if bounded:
            pw, base, mass, mode = TE.draw_table(w, mu, sigma, low, high)
            k, amb = _pick(np.cumsum(pw), u0 * np.sum(pw))
            x, tq, _ = truncated_quantile(base[k], mass[k], mode[k], mu[k], sigma[k], low, high, u1)
            deep = tq < DEEP_Q
            tol = screen_margin() * sigma[k] + 4.0 * np.spacing(np.abs(x))
            out.update(q=tq, deep=deep, tol=np.where(deep, np.inf, tol), mode=mode[k])
        else:
            k, amb = _pick(np.cumsum(w), u0 * np.sum(w))
            z, r = box_muller(u1, u2)
            x = _affine(mu[k], sigma[k], z)
            out.update(tol=8.0 * EPS * (np.abs(mu[k]) + sigma[k] * r))
        out.update(k=k, x=x, sigma=sigma[k], u1=u1, ambiguous_pick=amb)
    else:
        cdf = np.cumsum(w)                   # pick(): the running sum, in order
        wsum = np.sum(w)
        todo = np.arange(n)
        for it in range(REJECT_TRIES):
            u0, u1, u2, u3 = uniforms(seed, gi[todo], stream, it)
            k, amb = _pick(cdf, u0 * wsum)
            z, r = box_muller(u1, u2)
            v = _affine(mu[k], sigma[k], z)
            tol = 8.0 * EPS * (np.abs(mu[k]) + sigma[k] * r)
            if bounded:
                ok = (low <= v) & (v < high)
                amb = amb | (np.abs(v - low) <= tol) | (np.abs(v - high) <= tol)
            else:
                ok = np.ones(v.shape, dtype=bool)
            out['ambiguous_pick'][todo] |= amb
            out['k'][todo], out['sigma'][todo], out['tries'][todo] = k, sigma[k], it + 1
            acc = todo[ok]
            out['x'][acc], out['u1'][acc], out['tol'][acc] = v[ok], u1[ok], tol[ok]
            last = (k[~ok], u3[~ok])
            todo = todo[~ok]
            if todo.size == 0:
                break
        if todo.size:
            # budget spent: the truncated inverse CDF of the last component at
            # u3.  The device forms a + u3 (b - a) from 0.5 (1 + erf) values:
            # a few 2^-53 absolute in probability, i.e. that over the density
            # in value -- the exact quantile comes from the tail that keeps
            # its precision (the table's rule)
            k, u3 = last
            _, base, mass, mode = TE.draw_table(np.ones(k.size), mu[k], sigma[k], low, high)
            x, _, _ = truncated_quantile(base, mass, mode, mu[k], sigma[k], low, high, u3)
            zs = (x - mu[k]) / sigma[k]
            phi = np.exp(-0.5 * zs * zs) / math.sqrt(2.0 * math.pi)
            out['spent'][todo] = True
            out['x'][todo], out['u1'][todo] = x, u3
            out['tol'][todo] = 8.0 * 2.0 ** -53 * sigma[k] / phi + 4.0 * np.spacing(np.abs(x))
    x = out['x']
    v = np.exp(x) if family == LGMM else x.copy()
    if q is not None:
        # the tolerance in the value's domain, then in lattice steps
        tv = out['tol'] * np.abs(v) + 4.0 * EPS * np.abs(v) if family == LGMM else out['tol']
        s = v / q
        half = np.abs((s - np.floor(s)) - 0.5)         # distance to the rounding boundary
        out['ambiguous_round'] = ~(half > tv / q + 4.0 * EPS * np.abs(s))
        v = np.rint(s) * q
    out['value'] = v
    return out


def all_component_values(case, rep, i):
    """x* of draw i under every component of the case's mixture instead of the
    picked one (the same uniforms): for a failure report -- the component of
    the nearest value tells a wrong pick from a wrong inversion."""
    family, w, mu, sigma, low, high, q = mixture(case)
    if family == CAT or not rep['table'][i]:
        return None
    u1 = np.full(w.size, rep['u1'][i])
    if low is not None:
        _, base, mass, mode = TE.draw_table(w, mu, sigma, low, high)
        return truncated_quantile(base, mass, mode, mu, sigma, low, high, u1)[0]
    z = (rep['x'][i] - mu[rep['k'][i]]) / sigma[rep['k'][i]]
    return mu + sigma * z


# ---------------------------------------------------------------------------
# the cases the CPU and the GPU test share
# ---------------------------------------------------------------------------
N_DRAWS = 1 << 16
N_REJECT = 4096
STREAM = 7
OFFSET = 2 ** 32 - 1000       # the counter's high word changes inside the call
SPLIT = 12345                 # the odd offset a second call is split at
SIGMA_LO, SIGMA_HI = 0.15, 2.4


def _seed(j):
    """A Philox key with a nonzero high word, one per case."""
    return (0x9E3779B97F4A7C15 + 0x0123456789ABCDEF * j) & (2 ** 64 - 1)


def _components(K, rs, mu_lo=-3.0, mu_hi=3.0):
    w = rs.uniform(0.2, 1.0, K)
    mu = rs.uniform(mu_lo, mu_hi, K)
    sigma = np.exp(rs.uniform(math.log(SIGMA_LO), math.log(SIGMA_HI), K))
    if K > 1:
        sigma[0], sigma[-1] = SIGMA_LO, SIGMA_HI      # the span is a factor of 16 at least
    return w / w.sum(), mu, sigma


def _cat(K, rs):
    p = rs.uniform(0.1, 1.0, K)
    p[rs.permutation(K)[:max(1, K // 5)]] = 0.0
    p[0] = 0.0
    return p / p.sum()


def _build(name):
    """(family, w, mu, sigma, low, high, q) of a case, from a fixed RandomState."""
    kind = CASES[name]
    rs = np.random.RandomState(kind['rs'])
    fam = kind['family']
    if fam == CAT:
        return CAT, _cat(kind['K'], rs), None, None, None, None, None
    K = kind['K']
    w, mu, sigma = _components(K, rs)
    shape = kind.get('shape')
    if shape == 'zero-weight':
        w[::4] = 0.0
        w /= w.sum()
    elif shape == 'zero-mass':
        mu[1::4] = np.where(np.arange(mu[1::4].size) % 2 == 0, 60.0, -60.0)
        sigma[1::4] = SIGMA_LO
    elif shape == 'one':
        w, mu, sigma = np.array([1.0]), np.array([0.3]), np.array([1.0])
    elif shape == 'std-normal':
        mu[:], sigma[:] = 0.0, 1.0
    return fam, w, mu, sigma, kind.get('low'), kind.get('high'), kind.get('q')


_MIX = {}


def mixture(name):
    if name not in _MIX:
        _MIX[name] = _build(name)
    return _MIX[name]


def _case(family, K, rs, seed, low=None, high=None, q=None, shape=None, n=N_DRAWS):
    return dict(family=family, K=K, rs=rs, seed=_seed(seed), low=low, high=high, q=q, shape=shape, n=n)


# (the outer placements lie far enough out for a few draws in 1e4 to be deep)
IN, ABOVE, BELOW = (-2.0, 2.5), (10.0, 12.0), (-12.0, -10.0)
CASES = {
    # GMM, bounded: the table sampler's three modes
    'gmm-in': _case(GMM, 32, 1, 1, *IN),
    'gmm-above': _case(GMM, 32, 1, 2, *ABOVE),
    'gmm-below': _case(GMM, 32, 1, 3, *BELOW),
    'gmm-k1': _case(GMM, 1, 2, 4, -1.0, 2.0, shape='one'),
    'gmm-k2048': _case(GMM, 2048, 3, 5, *IN),
    'gmm-zero-weight': _case(GMM, 32, 4, 6, *IN, shape='zero-weight'),
    'gmm-zero-mass': _case(GMM, 32, 5, 7, *IN, shape='zero-mass'),
    # Box-Muller
    'gmm-unbounded': _case(GMM, 32, 6, 8),
    'lgmm-bounded': _case(LGMM, 32, 7, 9, *IN),
    'lgmm-unbounded': _case(LGMM, 32, 8, 10),
    'qgmm-bounded': _case(GMM, 32, 9, 11, *IN, q=0.5),
    'qgmm-unbounded': _case(GMM, 32, 10, 12, q=0.5),
    'qlgmm-bounded': _case(LGMM, 32, 11, 13, *IN, q=0.5),
    'qlgmm-unbounded': _case(LGMM, 32, 12, 14, q=0.5),
    'cat-4': _case(CAT, 4, 13, 15),
    'cat-300': _case(CAT, 300, 14, 16),
    'cat-2048': _case(CAT, 2048, 15, 17),
    'cat-2049': _case(CAT, 2049, 16, 18),
    # K = 2049: the rejection sampler
    'reject-unbounded': _case(GMM, 2049, 17, 19, n=N_REJECT),
    'reject-half': _case(GMM, 2049, 18, 20, 0.0, 9.0, n=N_REJECT),
    'reject-spent': _case(GMM, 2049, 19, 21, 3.5, 4.0, shape='std-normal', n=N_REJECT),
}
MODE_CASES = ('gmm-in', 'gmm-above', 'gmm-below')

_REPLAY = {}


def case_replay(name):
    """The replay of a case, computed once and shared (read-only)."""
    if name not in _REPLAY:
        c = CASES[name]
        fam, w, mu, sigma, low, high, q = mixture(name)
        r = replay(fam, w, mu, sigma, low, high, q, c['seed'], STREAM, OFFSET, c['n'])
        for v in r.values():
            v.setflags(write=False)
        _REPLAY[name] = r
    return _REPLAY[name]
