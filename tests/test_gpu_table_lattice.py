"""The device's bound lattice and hot intervals (k_table_bound / k_table_pilot,
DESIGN 5.10) read back through Plan.tab_bound and Plan.tab_hot and held
against a reference: the lattice against the oracle's fp64 score of the
device's own mixtures, the intervals against tools/table_error.py's
hot_intervals on the device's own lattice.

Histories: test_gpu_table.py's plan (u, lu: the log-space transform; n takes
no table) and one uniform(-5, 5) hp 'e' per named history of
tools/table_error.py (a plan each, with two copies of the hp beside it) -- low-edge, high-edge (the EI maximum on a bound: an
infinite interval end), band (the certificate closest to its bar), comb (a
local maximum per tooth: more hot runs than kHotIv under a tie window of 1)
and ties (half-unit values: a panel of the above table is not certified, no
lattice, the slot falls back).  N = 6000, 6 suggestions of 2^18 + 8192 + 37
candidates as in the neighbouring files.

The score the lattice bounds is the map's EI-only score ((M_b - M_a) +
log2(s_b / s_a)) ln 2 of the two tables' sums.  It leaves no per-slot constant
out against the oracle's llik_b - llik_a: a GMM's coefficient constants hold
log(w / sqrt(2 pi sigma^2) / p_accept) (make_coef), so each table carries its
side's truncation mass as the oracle's gmm_lpdf does; an LGMM's hold no
p_accept and neither does the oracle's lgmm_lpdf (the reference applies none
without q), and its log x is the same on both sides and cancels.  The constant
is 0 for both families: the reference below is the oracle's llik_b - llik_a of
plan.mixture's components as it stands.  (The emulation's tables take the
same p_accept, computed by the oracle: table_error.pacc_of.)

Environment switches are read once per process, so their runs are child
interpreters: four in this file (prefilter off; tables off; the comb under
TPE_TABLE_TIE_LOG2=0 with the prefilter and without).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from hyperopt_amd import hp, _engine as E
from hyperopt_amd.base import Domain

from gpu_util import assert_winners_match

import test_gpu_table as T
import test_gpu_tie_gather as G
import test_gpu_table_scalar as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import table_error as TE  # noqa: E402
from oracle import tpe_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

N, NC, NWT = T.N, T.NC, S.NWT
SEEDS6 = T.SEEDS6
BOUND = T.BOUND
CELLS, HOT_IV = TE.CELLS, TE.HOT_IV
NEG_INF = np.array([-np.inf]).view(np.uint64)[0]
NAMED = ('low-edge', 'high-edge', 'band', 'ties', 'comb')
E2E = ('low-edge', 'high-edge', 'band', 'ties')       # (e), and the default-tie children
LATTICE = ('u', 'lu', 'low-edge', 'high-edge', 'band', 'comb')   # certified pairs: (a), (b)
INTERVALS = ('u', 'lu', 'low-edge', 'high-edge')      # (c)
COMB_ENV = {'TPE_TABLE_TIE_LOG2': '0'}                # a tie window of 2^0


def _named_plan(name):
    """A uniform(-5, 5) hp 'e' on a named history of tools/table_error.py,
    and two more hps on the same column: a suggest takes the sorted draw, and
    with it the tables, from 2^22 candidates per level -- three slots at 6
    suggestions.  The tests read 'e'."""
    losses, cols, _ = TE.NAMED[name](N)
    dom = Domain(lambda x: 0.0, {l: hp.uniform(l, -5, 5) for l in ('e', 'e2', 'e3')})
    vals = np.stack([cols['e'] for l in dom.space.labels])
    act = np.ones_like(vals, dtype=np.uint8)
    hps, conds, pprior = dom.space.engine_tables()
    plan = E.Plan(E.default_engine(), hps, conds, pprior, max_trials=N)
    plan.set_history(losses, vals, act)
    plan.fit()
    return dom, plan, (losses, vals, act)


def _f64hex(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes().hex()


def _f64(h, shape=(-1,)):
    return np.frombuffer(bytes.fromhex(h), dtype=np.float64).reshape(shape)


def _run(dom, plan, labels, lattice=False):
    """One 6-suggestion call: S._suggest's records, counts and wave-tile
    scores, with the hot intervals and (lattice) the bound lattices."""
    out = S._suggest(dom, plan, SEEDS6, labels)
    hot = plan.tab_hot(len(SEEDS6))
    for lab in labels:
        i = dom.space.by_label[lab].index
        out['hot_' + lab] = _f64hex(hot[:, i])
        if lattice:
            try:
                out['U_' + lab] = _f64hex(plan.tab_bound(i))
            except ValueError:
                out['U_' + lab] = None
    return out


def case_default_tie(names=E2E, shape=True):
    """The default-tie suggests of the table shape and the named histories
    (children: TPE_TABLE_PREFILTER=0)."""
    out = {}
    if shape:
        dom, plan, _ = T._plan()
        out['shape'] = S._suggest(dom, plan, SEEDS6, ('u', 'lu'))
    for name in names:
        dom, plan, _ = _named_plan(name)
        out[name] = S._suggest(dom, plan, SEEDS6, ('e',))
    return out


def case_records(names=E2E):
    """The records alone (TPE_TABLE=0 keeps no wave scores)."""
    out = {}
    for name in names:
        dom, plan, _ = _named_plan(name)
        out[name] = dict(hex=T._hex(plan.suggest(SEEDS6, NC)))
    return out


def case_comb(lattice):
    dom, plan, _ = _named_plan('comb')
    if not lattice:
        return S._suggest(dom, plan, SEEDS6, ('e',))
    return _run(dom, plan, ('e',), lattice=True)


def _child(case, env):
    code = ("import sys, json; sys.path.insert(0, 'tests'); import test_gpu_table_lattice as L; "
            "print('JSON' + json.dumps(L.%s))" % case)
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.split('JSON')[-1])


# ---- the runs, each made once -------------------------------------------
class Slot:
    """One (plan, hp) of the default process: the plan, the hp's descriptor,
    the device mixtures, lattice, hot intervals and wave-tile scores."""

    def __init__(self, key, dom, plan, hist, lab, run):
        self.key, self.dom, self.plan, self.hist, self.lab, self.run = key, dom, plan, hist, lab, run
        self.i = dom.space.by_label[lab].index
        self.t = dom.space.engine_tables()[0][self.i]
        self.fam = 'lgmm' if self.t.family == E.LGMM else 'gmm'
        self.low, self.high, self.pm = self.t.low, self.t.high, self.t.prior_mu
        self.y_lo, self.y_hi = self.low - self.pm, self.high - self.pm
        self.cw = (self.y_hi - self.y_lo) / CELLS
        self.mix = [plan.mixture(self.i, side) for side in (0, 1)]
        U = run.get('U_' + lab)
        self.U = None if U is None else _f64(U)
        self.hot = _f64(run['hot_' + lab], (len(SEEDS6), 2 + 2 * HOT_IV))
        self._tabs = self._ref = None

    def tabs(self):
        """The emulation's tables of the device's mixtures."""
        if self._tabs is None:
            self._tabs = [TE.build(w, mu, sg, self.low, self.high, self.pm,
                                   TE.pacc_of(self.fam, w, mu, sg, self.low, self.high))
                          for w, mu, sg in self.mix]
        return self._tabs

    def score(self, y):
        """The oracle's fp64 (llik_b, llik_a) of the device's mixtures at
        centred fitted-domain values y, in chunks of at most 1e7 elements."""
        v = np.asarray(y, dtype=np.float64) + self.pm
        x = np.exp(v) if self.fam == 'lgmm' else v
        f = O.lgmm_lpdf if self.fam == 'lgmm' else O.gmm_lpdf
        out = []
        with np.errstate(all='ignore'):
            for w, mu, sg in self.mix:
                rows = max(1, int(1e7) // w.size)
                out.append(np.concatenate([f(x[a:a + rows], w, mu, sg, low=self.low, high=self.high)
                                           for a in range(0, x.size, rows)]))
        return out

    def reference(self):
        """The point set of (a) with its cells and reference scores, once."""
        if self._ref is None:
            y, cell = lattice_points(self.y_lo, self.y_hi, self.tabs())
            lb, la = self.score(np.clip(y, self.y_lo, self.y_hi))
            self._ref = (y, cell, lb, la)
        return self._ref


def lattice_points(y_lo, y_hi, tabs):
    """(y', cell) of the lattice check: per cell both end points, the
    midpoint and two random interior points; the doubles on either side of
    every panel edge of either table; four points outside [y_lo, y_hi], which
    the tables clamp onto the end points of the edge cells."""
    cw = (y_hi - y_lo) / CELLS
    c = np.arange(CELLS, dtype=np.float64)
    lo, hi = y_lo + cw * c, np.minimum(y_hi, y_lo + cw * (c + 1.0))
    rs = np.random.RandomState(17)
    pts = np.stack([lo, hi, 0.5 * (lo + hi), lo + cw * rs.rand(CELLS), lo + cw * rs.rand(CELLS)], 1)
    cell = np.repeat(np.arange(CELLS), pts.shape[1])
    ys, cs = [pts.reshape(-1)], [cell]
    for tab in tabs:
        e = tab['y_lo'] + tab['width'] * np.arange(1, tab['P'])
        e = np.concatenate([np.nextafter(e, -np.inf), np.nextafter(e, np.inf)])
        ys.append(e)
        cs.append(np.clip(np.floor((e - y_lo) / cw), 0, CELLS - 1).astype(int))
    ys.append(np.array([y_lo - 1.0, y_lo - 1e-9, y_hi + 1e-9, y_hi + 1.0]))
    cs.append(np.array([0, 0, CELLS - 1, CELLS - 1]))
    return np.concatenate(ys), np.concatenate(cs)


@pytest.fixture(scope='module')
def slots():
    assert os.environ.get('TPE_TABLE_PREFILTER', '1') != '0', 'the default is under test'
    assert 'TPE_TABLE_TIE_LOG2' not in os.environ, 'the default tie window is under test'
    out = {}
    dom, plan, hist = T._plan()
    run = _run(dom, plan, ('u', 'lu'), lattice=True)
    for lab in ('u', 'lu'):
        out[lab] = Slot(lab, dom, plan, hist, lab, run)
    for name in NAMED:
        dom, plan, hist = _named_plan(name)
        out[name] = Slot(name, dom, plan, hist, 'e', _run(dom, plan, ('e',), lattice=True))
    return out


@pytest.fixture(scope='module')
def pref_off():
    return _child('case_default_tie()', {'TPE_TABLE_PREFILTER': '0'})


@pytest.fixture(scope='module')
def table_off():
    return _child('case_records()', {'TPE_TABLE': '0'})


@pytest.fixture(scope='module')
def comb_on():
    return _child('case_comb(True)', COMB_ENV)


@pytest.fixture(scope='module')
def comb_off():
    return _child('case_comb(False)', dict(COMB_ENV, TPE_TABLE_PREFILTER='0'))


def _off_of(pref_off, key):
    return (pref_off['shape'], key) if key in ('u', 'lu') else (pref_off[key], 'e')


def _wmax(run, lab):
    return np.frombuffer(bytes.fromhex(run['wmax_' + lab]), dtype=np.uint64).reshape(len(SEEDS6), NWT)


def _pilot_best(w):
    """L0 of one suggestion: the best of the first kPilotWaves wave-tile
    scores (a NaN among them: NaN)."""
    p = w[:TE.PILOT_WAVES]
    return np.nan if np.isnan(p).any() else float(p.max())


# ---- (a) the device lattice bounds the reference score -----------------
def test_uncertified_slot_has_no_lattice(slots):
    """ties: a panel of the above table is not certified -- tab_bound fails,
    and so does it for an hp that takes no table (the normal)."""
    assert slots['ties'].U is None
    with pytest.raises(ValueError):
        slots['ties'].plan.tab_bound(slots['ties'].i)
    sl = slots['u']
    with pytest.raises(ValueError):
        sl.plan.tab_bound(sl.dom.space.by_label['n'].index)
    for k in LATTICE:
        assert slots[k].U is not None and slots[k].U.shape == (CELLS,), k


@pytest.mark.parametrize('key', LATTICE)
def test_lattice_bounds_the_oracle_score(slots, key):
    """U[c] >= S_ref(y) - 2^-27 (max(1, |llik_b|) + max(1, |llik_a|)) at every
    point of lattice_points -- the suite's per-side table bound, summed over
    the two sides -- and every U[c] is finite.  The points outside the range
    also go through the device (mode 4): their table score is the reference
    score of the end point they are clamped onto, within the same margin, and
    so under the edge cell's bound."""
    sl = slots[key]
    y, cell, lb, la = sl.reference()
    U = sl.U
    assert np.isfinite(U).all(), int((~np.isfinite(U)).sum())
    assert np.isfinite(lb).all() and np.isfinite(la).all()
    margin = BOUND * (np.maximum(1.0, np.abs(lb)) + np.maximum(1.0, np.abs(la)))
    gap = U[cell] - (lb - la)
    worst = int(np.argmin(gap + margin))
    print('%s: min(U - S_ref) = %.3e over %d points (cell %d, y\' = %.17g, margin there %.3e)'
          % (key, gap.min(), y.size, cell[worst], y[worst], margin[worst]))
    assert (gap >= -margin).all(), (key, int(cell[worst]), float(y[worst]), float(gap[worst]))
    # the clamp on the device (the four points behind 124 cell midpoints: a whole wave tile)
    co = cell[-4:]
    v = np.concatenate([np.clip(y[2:5 * 124:5], sl.y_lo, sl.y_hi), y[-4:]]) + sl.pm
    x = np.exp(v) if sl.fam == 'lgmm' else v
    assert x.size == 128
    dlb, dla, _, _ = sl.plan.score_candidates(sl.i, x, sorted_mode=4)
    sd = (dlb - dla)[-4:]
    print('%s: clamped device scores - reference:' % key, (sd - (lb - la)[-4:]).tolist())
    assert np.isfinite(sd).all()
    assert (np.abs(sd - (lb - la)[-4:]) <= margin[-4:]).all(), (key, sd.tolist())
    assert (sd <= U[co] + margin[-4:]).all(), (key, sd.tolist(), U[co].tolist())


# ---- (b) the lattice is not vacuous --------------------------------------
@pytest.mark.parametrize('key', LATTICE)
def test_lattice_is_as_tight_as_the_emulation(slots, key):
    """Against the emulation's lattice of the same device mixtures: the median
    over cells of U - max_cell(S_ref) is at most twice the emulation's
    (rounding differences are ~1e-10 against medians of ~1e-5), and under a
    threshold T0 that leaves some cells cold the device's hot cells lie
    within the emulation's widened by one cell on each side."""
    sl = slots[key]
    y, cell, lb, la = sl.reference()
    tb, ta = sl.tabs()
    assert tb['ok'].all() and ta['ok'].all()
    U_emu = TE.bound_lattice(tb, ta)
    cmax = np.full(CELLS, -np.inf)
    np.maximum.at(cmax, cell, lb - la)
    med_dev, med_emu = float(np.median(sl.U - cmax)), float(np.median(U_emu - cmax))
    print('%s: median(U - max_cell S_ref): device %.4e, emulation %.4e; max |U_dev - U_emu| = %.3e'
          % (key, med_dev, med_emu, float(np.abs(sl.U - U_emu).max())))
    assert med_emu > 0.0 and med_dev <= 2.0 * med_emu
    L0 = float(cmax.max())
    T0 = L0 - TE.TIE * max(1.0, abs(L0))
    hot_dev, hot_emu = ~(sl.U < T0), ~(U_emu < T0)
    assert hot_dev.any() and not hot_dev.all(), int(hot_dev.sum())
    wide = hot_emu.copy()
    wide[:-1] |= hot_emu[1:]
    wide[1:] |= hot_emu[:-1]
    print('%s: hot cells under T0 = %.6f: device %d, emulation %d'
          % (key, T0, int(hot_dev.sum()), int(hot_emu.sum())))
    assert not (hot_dev & ~wide).any(), np.flatnonzero(hot_dev & ~wide).tolist()


# ---- (c) the hot intervals are the stated function of the lattice ------
def _cells(v, y_lo, cw):
    """Interval ends as cell indices; infinite ends stay infinite."""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        return np.where(np.isfinite(v), np.round((v - y_lo) / cw), v)


def _check_intervals(sl, hot, off_w, tie, msg):
    """Every suggestion's TabHot record against hot_intervals(U_dev, L0):
    y_lo and y_hi exactly, the interval ends as cell indices, infinite ends
    and the unused (+inf, -inf) slots exactly.  Returns per suggestion
    (raw runs, intervals, an end was infinite)."""
    out = []
    for s in range(len(SEEDS6)):
        L0 = _pilot_best(off_w[s].view(np.float64))
        want, hot_cells = TE.hot_intervals(sl.U, L0, sl.y_lo, sl.y_hi, tie)
        rec = hot[s]
        assert rec[0] == sl.y_lo and rec[1] == sl.y_hi, (msg, s, rec[:2].tolist())
        lo = np.full(HOT_IV, np.inf)
        hi = np.full(HOT_IV, -np.inf)
        lo[:len(want)] = [a for a, b in want]
        hi[:len(want)] = [b for a, b in want]
        got_lo, got_hi = rec[2:2 + HOT_IV], rec[2 + HOT_IV:]
        np.testing.assert_array_equal(_cells(got_lo, sl.y_lo, sl.cw), _cells(lo, sl.y_lo, sl.cw),
                                      err_msg='%s s=%d lo' % (msg, s))
        np.testing.assert_array_equal(_cells(got_hi, sl.y_lo, sl.cw), _cells(hi, sl.y_lo, sl.cw),
                                      err_msg='%s s=%d hi' % (msg, s))
        fin = np.isfinite(got_lo)
        assert (np.abs(got_lo[fin] - lo[fin]) <= 1e-9 * sl.cw).all()
        fin = np.isfinite(got_hi)
        assert (np.abs(got_hi[fin] - hi[fin]) <= 1e-9 * sl.cw).all()
        out.append((TE.hot_runs(hot_cells), len(want),
                    bool(np.isinf(got_lo[:len(want)]).any() or np.isinf(got_hi[:len(want)]).any())))
    return out


@pytest.mark.parametrize('key', INTERVALS)
def test_hot_intervals_follow_the_lattice(slots, pref_off, key):
    """tab_hot of the default run = hot_intervals(U_dev, L0, y_lo, y_hi, 2^-16)
    with L0 the best of the unfiltered run's first 64 wave-tile scores (the
    pilot's tiles).  The two edge histories show an infinite end."""
    sl = slots[key]
    off, lab = _off_of(pref_off, key)
    res = _check_intervals(sl, sl.hot, _wmax(off, lab), TE.TIE, key)
    print('%s: per suggestion (raw runs, intervals, infinite end):' % key, res)
    if key in ('low-edge', 'high-edge'):
        assert all(r[2] for r in res), res
        side = sl.hot[:, 2] if key == 'low-edge' else sl.hot[:, 2 + HOT_IV:].max(axis=1)
        assert (side == (-np.inf if key == 'low-edge' else np.inf)).all(), side.tolist()


# ---- the pruned tiles, as test_prefilter_changes_nothing_downstream ------
def _check_pruned(on, off, lab, tie, msg):
    assert on['hex'] == off['hex'], msg
    assert on['counts'] == off['counts'], msg
    a, b = _wmax(on, lab), _wmax(off, lab)
    assert not (b == NEG_INF).any()
    fracs = []
    for s in range(len(SEEDS6)):
        pruned = a[s] == NEG_INF
        np.testing.assert_array_equal(a[s][~pruned], b[s][~pruned])
        w = b[s].view(np.float64)
        tab_max = np.nan if np.isnan(w).any() else w.max()
        thr = tab_max - tie * max(1.0, abs(tab_max))
        assert (w[pruned] < thr).all(), (msg, s, float(w[pruned].max()), thr)
        assert pruned.any() and not pruned.all(), (msg, s, int(pruned.sum()))
        fracs.append(float(pruned.mean()))
    print('%s: pruned fraction of the wave tiles min %.4f median %.4f max %.4f'
          % (msg, min(fracs), float(np.median(fracs)), max(fracs)))
    return fracs


# ---- (d) the merge of more than kHotIv runs ------------------------------
def test_comb_takes_the_merge(slots, comb_on, comb_off):
    """The comb under a tie window of 2^0: U_dev and the unfiltered run's L0
    leave more than kHotIv raw runs in at least one suggestion, the device's
    merged intervals are those of hot_intervals, the records are those of the
    unfiltered run byte for byte, every pruned wave tile's unfiltered score
    lies under tab_max - 1.0 max(1, |tab_max|), and some tile is pruned."""
    sl = slots['comb']
    assert comb_on['U_e'] == _f64hex(sl.U)     # the lattice does not depend on the window
    hot = _f64(comb_on['hot_e'], (len(SEEDS6), 2 + 2 * HOT_IV))
    res = _check_intervals(sl, hot, _wmax(comb_off, 'e'), 1.0, 'comb tie 2^0')
    print('comb tie 2^0: per suggestion (raw runs, merged intervals, infinite end):', res)
    assert any(r[0] > HOT_IV for r in res), res
    assert all(r[1] == HOT_IV for r in res if r[0] > HOT_IV), res
    _check_pruned(comb_on, comb_off, 'e', 1.0, 'comb tie 2^0')


# ---- (e) end to end on the new histories ---------------------------------
@pytest.mark.parametrize('name', E2E)
def test_named_history_end_to_end(slots, pref_off, table_off, name):
    """Mode 4 lpdf within 2^-27 max(1, |ref|) of the oracle on both sides at
    test_table_lpdf_vs_oracle's point set (ties: mode 4 raises); the suggest
    with tables and prefilter gives the winners of a TPE_TABLE=0 run or EI
    ties; certified slots pass the pruned-tile check against the unfiltered
    run (ties: nothing is pruned, every wave tile goes to the direct pass)."""
    from test_gpu_shifted import _oracle_obs, _oracle_score
    sl = slots[name]
    dom, plan, t, i = sl.dom, sl.plan, sl.t, sl.i
    on = _unhex_records(sl.run['hex'], table_off[name]['hex'])
    assert_winners_match(on[0], on[1], msg=name + ', table vs direct')
    if name == 'ties':
        with pytest.raises(Exception):
            plan.score_candidates(i, np.zeros(8), sorted_mode=4)
        assert sl.run['hex'] == pref_off[name]['hex']
        assert not (_wmax(sl.run, 'e') == NEG_INF).any()
        assert (np.asarray(sl.run['counts']) == G.WAVE_TILES).all(), sl.run['counts']
        return
    obs = _oracle_obs(dom, *sl.hist)
    rs = np.random.RandomState(3)
    w, mu, sg = sl.mix[0]
    edge = np.concatenate([T._panel_points(plan, t, i, 0), T._panel_points(plan, t, i, 1)])
    ends = np.array([t.low, np.nextafter(t.high, -np.inf)])
    wide = rs.uniform(t.low, t.high, 1024)
    draws = plan.engine.sample(t.family, w, mu, sg, t.low, t.high, None, seed=99, stream=i,
                               n=4096 - edge.size - ends.size - wide.size)
    x = np.concatenate([draws, wide, ends, edge])
    assert x.size == 4096
    ref = _oracle_score(dom, obs, 'e', x)
    lb, la, bi, bs = plan.score_candidates(i, x, sorted_mode=4)
    T._assert_lpdf(lb, ref['llik_b'], name + ' below')
    T._assert_lpdf(la, ref['llik_a'], name + ' above')
    _check_pruned(sl.run, pref_off[name], 'e', TE.TIE, name)


def _unhex_records(a, b):
    shape = (len(SEEDS6), -1)
    return [np.frombuffer(bytes.fromhex(h), dtype=E.RESULT_DTYPE).reshape(shape) for h in (a, b)]
