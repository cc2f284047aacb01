"""The screened pruning draw's screen (tpe_screen.hip) on the
CPU, through tools/table_error.py's restatement of it: erfcinv_fast's measured
error against the margin the engine uses, and the soundness of the u1
thresholds -- a draw the screen calls cold lies, as draw_bounded_invert
computes it, strictly inside the gap the screen says, outside every zone; and
whole sort blocks (draw_screen) against the computation on all elements.
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


def _constant(path, name):
    m = re.search(r'constexpr double %s = ([^;]+);' % name, open(os.path.join(CSRC, path)).read())
    return float.fromhex(m.group(1)) if m.group(1).startswith('0x') else float(m.group(1))


def test_margin_covers_measured_error():
    """16 times the largest |x drawn - x true| / sigma over the tail
    probabilities the screen covers fits in the margin; beyond them the tail
    polynomial drifts, which is why they are never cold; and the engine's
    constants are the tool's."""
    rows = TE.invert_error()
    for lab, e, y in rows:
        print('%-44s %.3e at y = %.6e' % (lab, e, y))
    worst = max(e for _, e, _ in rows[:2])
    assert 16.0 * worst <= TE.SCREEN_MARGIN <= 32.0 * worst, worst
    assert rows[2][1] > TE.SCREEN_MARGIN          # (the reason for SCREEN_Q_MIN)
    assert rows[3][1] == 0.0
    assert _constant('tpe_internal.hpp', 'kScreenMargin') == TE.SCREEN_MARGIN
    assert _constant('tpe_screen.hip', 'kScreenQMin') == TE.SCREEN_Q_MIN


DRAWS = 21 * 8192          # the pilot's sort block and 20 behind it


@pytest.fixture(scope='module')
def screen_cases():
    """(name, tb, ta, below mixture, low, high, centre, k, u1, x): config 4's
    history (three hyperparameters) and the named shapes (`ties` has no
    certified above table: k_draw_zone leaves it unscreened, nothing to emulate)."""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    sys.path.insert(0, ROOT)
    import bench
    dom, losses, vals, act = bench.build_workload('cfg4')
    jobs = [('cfg4/%d' % i, losses, {h.label: vals[h.index] for h in dom.space.hps},
             dom.space.hps[i].label, ('uniform', (-5.0, 5.0))) for i in (0, 40, 90)]
    for name in ('low-edge', 'high-edge', 'band', 'ties', 'comb'):
        l, cols, specs = TE.NAMED[name](6000)
        lab = next(iter(specs))
        jobs.append((name, l, cols, lab, specs[lab]))
    out = []
    for j, (name, l, cols, lab, (dist, args)) in enumerate(jobs):
        cp = TE.certified_pair(l, cols, lab, dist, args)
        if cp is None:     # no two certified tables: the slot is not screened (nz = 0)
            assert name == 'ties', name
            continue
        tb, ta, mix, (low, high, center) = cp
        k, u1, x = TE.draw_picks(*mix, low, high, DRAWS, np.random.RandomState(500 + j))
        out.append((name, tb, ta, mix, low, high, center, k, u1, x))
    return out


@pytest.mark.parametrize('tiles', [2, 0])
def test_screened_blocks_equal_full_computation(screen_cases, tiles):
    """Every block that does not fall back has the full computation's key
    range, kept mask, live buckets with their counts and bases, and bucket
    bytes.  Without widening some blocks must fall back; with the default
    widening fewer than 5 % of config 4's blocks may."""
    blocks = fallback = cfg4_blocks = cfg4_fallback = 0
    for name, tb, ta, mix, low, high, center, k, u1, x in screen_cases:
        r = TE.draw_screen(tb, ta, mix, low, high, center, k, u1, x, tiles)
        print('%-9s tiles %d: blocks %d fallback %d inverted %.4f' % (name, tiles, r['blocks'],
                                                                      r['fallback'], r['exact']))
        assert r['mismatch'] == [], (name, r['mismatch'][:3])
        assert r['blocks'] == DRAWS // 8192 - 1, name
        blocks += r['blocks']
        fallback += r['fallback']
        if name.startswith('cfg4'):
            cfg4_blocks += r['blocks']
            cfg4_fallback += r['fallback']
    if tiles == 0:
        assert fallback > 0
    else:
        assert cfg4_fallback < 0.05 * cfg4_blocks, (cfg4_fallback, cfg4_blocks)


@pytest.fixture(scope='module')
def below_mixtures():
    losses, cols, specs = TE.test_shape()
    out = {}
    for name in ('default', 'few-below', 'wide-below'):
        fit, (low, high, _) = TE.mixtures(losses, cols, 'u', *specs['u'], **TE.fit_params(name))
        out[name] = fit[0] + (low, high)
    return out


def _zones(low, high, mu):
    """Two tails, a plain interval, and one narrower than any margin around a
    component's mean; ascending and disjoint."""
    w = high - low
    mid = float(np.clip(np.median(mu), low + 0.1 * w, high - 0.1 * w))
    z = [(-np.inf, low + 0.02 * w), (low + 0.30 * w, low + 0.31 * w), (mid - 1e-9 * w, mid + 1e-9 * w),
         (low + 0.70 * w, low + 0.7004 * w), (high - 0.02 * w, np.inf)]
    z.sort()
    out = [z[0]]
    for a, b in z[1:]:
        if a <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], b))
        else:
            out.append((a, b))
    return np.array([a for a, _ in out]), np.array([b for _, b in out])


@pytest.mark.parametrize('name', ['default', 'few-below', 'wide-below'])
def test_cold_draws_lie_in_their_gap(below_mixtures, name):
    """Every mode of the table (the bounds moved so that all components lie
    below, inside and above them), a dense u1 grid plus the 8 doubles and the
    8 steps of 2^-53 on both sides of every threshold."""
    w, mu, sg, low, high = below_mixtures[name]
    span = high - low
    modes, cold_total = set(), 0
    for lo_b, hi_b in ((low, high), (mu.max() + 0.05 * span, mu.max() + 1.5 * span),
                       (mu.min() - 1.5 * span, mu.min() - 0.05 * span)):
        _, base, mass, mode = TE.draw_table(w, mu, sg, lo_b, hi_b)
        modes |= set(int(m) for m in mode[mass > 0.0])
        zlo, zhi = _zones(lo_b, hi_b, mu)
        thr = TE.zone_thresholds(zlo, zhi, base, mass, mode, mu, sg)
        assert thr.shape == (mu.size, 2 * (zlo.size - 1))
        assert (np.diff(thr, axis=1) >= 0.0).all() and (thr >= 0.0).all() and (thr <= 1.0).all()
        grid = np.floor(np.linspace(0.0, 1.0, 40001)[:-1] * 2.0 ** 53) * 2.0 ** -53
        for k in range(mu.size):
            near = [thr[k] + j * 2.0 ** -53 for j in range(-8, 9)]
            up, dn = thr[k].copy(), thr[k].copy()
            for _ in range(8):
                up, dn = np.nextafter(up, 2.0), np.nextafter(dn, -1.0)
                near += [up.copy(), dn.copy()]
            u = np.unique(np.concatenate([grid] + near))
            u = u[(u >= 0.0) & (u < 1.0)]
            gap = TE.screen_gap(thr[k], u)
            x = TE.draw_invert_emul(base[k], mass[k], mode[k], mu[k], sg[k], lo_b, hi_b, u)
            cold = gap >= 0
            cold_total += int(cold.sum())
            g = gap[cold]
            assert (x[cold] > zhi[g]).all() and (x[cold] < zlo[g + 1]).all(), (name, k, lo_b, hi_b)
            if not (mass[k] > 0.0):
                assert not cold.any()
    assert modes == {0, 1, 2}, modes
    assert cold_total > 0
