"""The large-draw table path away from the default fit parameters (DESIGN
5.10): every named set of tools/table_error.py's FIT_SETS (gamma, gamma_cap,
prior_weight, lf) on test_gpu_table.py's history (N = 6000) and candidate
count (2^18 + 8192 + 37).

What the sets reach: K_below = n_below + 1 picks the draw kernels -- up to 32
the small LDS draw table, up to 2048 the large one (wide-below, huge-below,
lf-long), above it (over-cap) neither the sorted draw nor the tables: the plain
draw without an LDS table (k_draw<false>) and k_score on every pair (k_bucket
only under TPE_SMALL_SORT=1); few-below and prior-only leave a below table of
two panels and of one; pw-zero a -inf coefficient on the widest component,
which is the slot's probe; pw-small, pw-big, lf-off and lf-long change every
weight.

Two spaces on the same columns of the history: u, n, lu (6 suggestions; the
unbounded normal makes every sorted draw the general kernel) for all eleven
sets, and the bounded-only u, lu (8 suggestions, so that the level still
reaches the sorted draw's 2^22 candidates; the inline-draw kernels) for
default, wide-below and huge-below.

Per set: the device mixtures against the oracle's bit for bit (the
loguniform's given the device's own log x, which is within an ulp of numpy's);
the tables
alone (mode 4) within test_gpu_table's derived 2^-27 of the oracle; an argmax
that leans on no switch -- all candidates of a suggestion regenerated from the
counter stream, scored per candidate with exact sums, the near-best set C
(within 1e-4 of the best: 100 times the agreement relied on) rescored by the
oracle, and the suggest's record checked against that; the records and tie
counts byte for byte those of child interpreters under TPE_DRAW_PRUNE=0,
TPE_TABLE_PREFILTER=0 and TPE_TABLE=0 (the switches are read once per
process); tab_wmax against the TPE_DRAW_PRUNE=0 child through
test_gpu_draw_prune's assertions and the census' table pairs, so the layers
are known to be in play (over-cap: known not to be); and TPE_GRAPH=1 replays
across the sets against eager calls.

Measured on an MI355X (DESIGN 5.10 has the figures per set): no set found a
fault in the engine; the module takes 10.2 s, test_gpu_table_lattice.py 10.7 s.
"""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from hyperopt_amd import hp, _engine as E
from hyperopt_amd.base import Domain

from gpu_util import assert_close, assert_winners_match
import test_gpu_table as T
import test_gpu_draw_prune as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import table_error as TE  # noqa: E402

pytestmark = pytest.mark.gpu

N, NC = T.N, T.NC
NWT = (NC + 127) // 128
SETS = tuple(TE.FIT_SETS)
LABELS = ('u', 'lu')
SEEDS = {'three': T.SEEDS6, 'two': [9001 + 13 * s for s in range(8)]}
RUNS = [('three', n) for n in SETS] + [('two', n) for n in ('default', 'wide-below', 'huge-below')]
RUN_IDS = ['%s/%s' % r for r in RUNS]
TABLED = [r for r in RUN_IDS if not r.endswith('over-cap')]
GRAPH_SEQ = ('default', 'wide-below', 'default', 'over-cap', 'pw-zero', 'default')
NEAR = 1e-4          # the cut of the near-best set C
C_MAX = 4096
NEG_INF = P.NEG_INF


def _space(kind):
    sp = T._space()
    if kind == 'two':
        del sp['n']
    return sp


def _plan(kind, name=None):
    """A fresh plan of the space with the history set, fitted with the named
    set's parameters (name None: not fitted)."""
    dom = Domain(lambda x: 0.0, _space(kind))
    hist = T._history(dom)
    hps, conds, pprior = dom.space.engine_tables()
    plan = E.Plan(E.default_engine(), hps, conds, pprior, max_trials=N)
    plan.set_history(*hist)
    if name is not None:
        plan.fit(**TE.fit_params(name))
    return dom, plan, hist


def _suggest(dom, plan, seeds, wmax=True):
    res = plan.suggest(seeds, NC)
    out = dict(hex=T._hex(res), counts=plan.tie_counts(len(seeds)).tolist(),
               labels=list(dom.space.labels))
    if wmax:
        wm = plan.tab_wmax(len(seeds))
        assert wm.shape[:2] == (len(seeds), len(dom.space.labels)), wm.shape
        out['wmax_width'] = int(wm.shape[2])
        for lab in LABELS:
            out['wmax_' + lab] = P.S._u64hex(wm[:, dom.space.by_label[lab].index, :NWT])
    return out


def case_all(wmax=True):
    """Every suggest of the module, a fresh plan each."""
    out = {}
    for kind, name in RUNS:
        dom, plan, _ = _plan(kind, name)
        out['%s/%s' % (kind, name)] = _suggest(dom, plan, SEEDS[kind], wmax)
    return out


def case_graph():
    """fit_suggest on one plan through GRAPH_SEQ, three calls per set, every
    call with a first seed of its own."""
    dom, plan, _ = _plan('three')
    out, i = [], 0
    for name in GRAPH_SEQ:
        for _ in range(3):
            out.append(T._hex(plan.fit_suggest([31 + i] + T.SEEDS6[1:], NC, **TE.fit_params(name))))
            i += 1
    return dict(hex=out)


def _child(case, env):
    code = ("import sys, json; sys.path.insert(0, 'tests'); import test_gpu_fit_params as F; "
            "print('JSON' + json.dumps(F.%s))" % case)
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.split('JSON')[-1])


@pytest.fixture(scope='module')
def runs():
    """The default run: per 'space/set' the plan (kept fitted) and its suggest."""
    for sw in ('TPE_DRAW_PRUNE', 'TPE_TABLE_PREFILTER', 'TPE_TABLE'):
        assert os.environ.get(sw, '1') != '0', 'the default is under test'
    out = {}
    for kind, name in RUNS:
        dom, plan, hist = _plan(kind, name)
        out['%s/%s' % (kind, name)] = dict(dom=dom, plan=plan, hist=hist,
                                           out=_suggest(dom, plan, SEEDS[kind]))
    return out


@pytest.fixture(scope='module')
def no_prune():
    return _child('case_all(True)', {'TPE_DRAW_PRUNE': '0'})


@pytest.fixture(scope='module')
def no_prefilter():
    return _child('case_all(False)', {'TPE_TABLE_PREFILTER': '0'})


@pytest.fixture(scope='module')
def no_table():
    return _child('case_all(False)', {'TPE_TABLE': '0'})


# ---- the oracle with the set's fit parameters (computed once per set and hp)
_SPEC = {'u': ('uniform', (-5.0, 5.0)), 'lu': ('loguniform', (math.log(1e-3), math.log(10)))}
_FITS = {}


def _oracle_fit(name, lab):
    """(family, low, high, below mixture, above mixture, fitted observations
    of both sides, (prior_mu, prior_sigma)) of one bounded hp."""
    from oracle import tpe_oracle as O
    if (name, lab) not in _FITS:
        s = TE.fit_params(name)
        dom = Domain(lambda x: 0.0, _space('three'))
        losses, vals, _ = T._history(dom)
        col = vals[dom.space.by_label[lab].index]
        tids = np.arange(N)
        with np.errstate(all='ignore'):
            fk, pm, ps, low, high, q, tr = O.posterior_spec(*_SPEC[lab], s['prior_weight'])
            sides = O.split_observations(tids, col, tids, losses, s['gamma'], s['gamma_cap'],
                                         kind='stable')
            tobs = [O.transform_obs(obs, tr, low) for obs in sides]
            mix = [O.parzen_fit(o, s['prior_weight'], pm, ps, lf=s['lf'], kind='stable')
                   for o in tobs]
        assert q is None
        _FITS[name, lab] = (fk, low, high, mix[0], mix[1], tobs, (pm, ps))
    return _FITS[name, lab]


def _oracle_lpdf(name, lab, x):
    """(below lpdf, above lpdf) of candidates x, 512 at a time."""
    from oracle import tpe_oracle as O
    fk, low, high, mb, ma = _oracle_fit(name, lab)[:5]
    f = O.lgmm_lpdf if fk == 'lgmm' else O.gmm_lpdf
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    lb, la = np.empty(x.size), np.empty(x.size)
    with np.errstate(all='ignore'):
        for a in range(0, x.size, 512):
            lb[a:a + 512] = f(x[a:a + 512], *mb, low=low, high=high)
            la[a:a + 512] = f(x[a:a + 512], *ma, low=low, high=high)
    return lb, la


def _records(run, n_hp):
    return np.frombuffer(bytes.fromhex(run['hex']), dtype=E.RESULT_DTYPE).reshape(-1, n_hp)


# ---- 1. mixtures
@pytest.mark.parametrize('name', SETS)
def test_mixtures_bit_exact(runs, name):
    """plan.mixture of both bounded hps and both sides against the oracle's
    parzen_fit on the oracle's split: the K of the set, and mu, sigma, w equal
    (test_gpu_ops.test_parzen_bit_exact's comparison).

    The loguniform is fitted on log(x), which the device takes itself: its
    log and numpy's are both within an ulp of the true one and differ in the
    last bit for about 0.7 % of the values here.  So for lu the device's
    sorted means must pair with the oracle's within one ulp of each -- the
    same observations on each side, in the same order, the prior at the same
    place and exact -- and the oracle's fit of the device's own logarithms
    (taken from those means) must then equal the device's bit for bit
    (fit_oracle.assert_mixture_bit_exact)."""
    from fit_oracle import assert_mixture_bit_exact
    s = TE.FIT_SETS[name]
    r = runs['three/' + name]
    for lab in LABELS:
        i = r['dom'].space.by_label[lab].index
        fk, _, _, mb, ma, tobs, (pm, ps) = _oracle_fit(name, lab)
        for side, ref in enumerate((mb, ma)):
            w, mu, sg = r['plan'].mixture(i, side)
            assert w.size == (s['K_below'], s['K_above'])[side], (name, lab, side, w.size)
            msg = '%s %s side %d ' % (name, lab, side)
            assert_mixture_bit_exact((w, mu, sg), tobs[side], s['prior_weight'], pm, ps, s['lf'],
                                     fk == 'lgmm', msg, ref=ref)


# ---- 2. the tables alone
@pytest.mark.parametrize('name', SETS)
def test_table_lpdf_vs_oracle(runs, name):
    """Mode 4 on test_gpu_table.test_table_lpdf_vs_oracle's candidates (below
    draws, the prior range, low, the last double under high, every panel
    boundary of both tables at this set's panel counts): both lpdfs within
    2^-27 of the oracle.  over-cap included: the tables are built on demand."""
    r = runs['three/' + name]
    dom, plan = r['dom'], r['plan']
    tabs = dom.space.engine_tables()[0]
    rs = np.random.RandomState(3)
    for lab in LABELS:
        i = dom.space.by_label[lab].index
        t = tabs[i]
        w, mu, sg = plan.mixture(i, 0)
        edge = np.concatenate([T._panel_points(plan, t, i, 0), T._panel_points(plan, t, i, 1)])
        ends = np.array([t.low, np.nextafter(t.high, -np.inf)])
        if t.family == E.LGMM:
            ends = np.array([math.exp(t.low), np.nextafter(math.exp(t.high), -np.inf)])
        wide = rs.uniform(t.low, t.high, 1024)
        wide = np.exp(wide) if t.family == E.LGMM else wide
        draws = plan.engine.sample(t.family, w, mu, sg, t.low, t.high, None, seed=99, stream=i,
                                   n=4096 - edge.size - ends.size - wide.size)
        x = np.concatenate([draws, wide, ends, edge])
        assert x.size == 4096
        ref_b, ref_a = _oracle_lpdf(name, lab, x)
        assert np.isfinite(ref_b).all() and np.isfinite(ref_a).all()
        lb, la, bi, bs = plan.score_candidates(i, x, sorted_mode=4)
        T._assert_lpdf(lb, ref_b, '%s %s below (%d panel edges)' % (name, lab, edge.size))
        T._assert_lpdf(la, ref_a, '%s %s above' % (name, lab))


# ---- 3. an argmax that leans on no switch
@pytest.mark.parametrize('name', SETS)
def test_independent_argmax(runs, name):
    from gpu_util import RTOL
    r = runs['three/' + name]
    dom, plan = r['dom'], r['plan']
    tabs = dom.space.engine_tables()[0]
    res = _records(r['out'], len(dom.space.labels))
    pick = np.random.RandomState(21).choice(NC, 512, replace=False)
    for s in (0, 5):
        for lab in LABELS:
            i = dom.space.by_label[lab].index
            t = tabs[i]
            w, mu, sg = plan.mixture(i, 0)
            x = plan.engine.sample(t.family, w, mu, sg, t.low, t.high, None, seed=T.SEEDS6[s],
                                   stream=i, offset=0, n=NC)
            lb, la, bi, bs = plan.score_candidates(i, x)
            ei = lb - la
            assert np.isfinite(ei).all(), (name, lab, s)
            best = ei.max()
            C = np.flatnonzero(ei >= best - NEAR * max(1.0, abs(best)))
            rec = res[s, i]
            print('%s %s s=%d: |C| = %d, best EI %.9g, record index %d score %.9g'
                  % (name, lab, s, C.size, best, int(rec['index']), float(rec['score'])))
            assert 1 <= C.size <= C_MAX, (name, lab, s, C.size)
            msg = '%s %s s=%d ' % (name, lab, s)
            for idx, what in ((C, 'near-best'), (pick, 'random 512')):
                ob, oa = _oracle_lpdf(name, lab, x[idx])
                assert np.isfinite(ob).all() and np.isfinite(oa).all(), msg + what
                assert_close(lb[idx], ob, msg=msg + what + ' below')
                assert_close(la[idx], oa, msg=msg + what + ' above')
                if what == 'near-best':
                    omax = (ob - oa).max()
            assert rec['active'] and 0 <= rec['index'] < NC, (name, lab, s, rec)
            assert np.float64(rec['value']).tobytes() == x[int(rec['index'])].tobytes(), \
                (name, lab, s, rec, x[int(rec['index'])])
            ob, oa = _oracle_lpdf(name, lab, rec['value'])
            oei = float(ob[0] - oa[0])
            assert_close([rec['score']], [oei], msg=msg + 'record score vs oracle')
            assert abs(oei - omax) <= RTOL * max(1.0, abs(omax)), (name, lab, s, oei, omax)


# ---- 4. the switches change nothing
@pytest.mark.parametrize('run', RUN_IDS)
def test_switches_change_nothing(runs, no_prune, no_prefilter, no_table, run):
    on = runs[run]['out']
    print('%s: tie counts per (suggestion, hp) %s' % (run, on['counts']))
    for other, what in ((no_prune, 'TPE_DRAW_PRUNE=0'), (no_prefilter, 'TPE_TABLE_PREFILTER=0')):
        assert other[run]['labels'] == on['labels']
        assert other[run]['hex'] == on['hex'], (run, what)
        assert other[run]['counts'] == on['counts'], (run, what)
    n_hp = len(on['labels'])
    a, b = _records(on, n_hp), _records(no_table[run], n_hp)
    assert_winners_match(a, b, msg=run + ': table vs direct')
    # (as test_gpu_table.test_suggest_table_vs_direct: the direct pass scores
    # again every wave tile in the tie window, so the records are its own)
    assert no_table[run]['hex'] == on['hex'], run
    cnt = np.asarray(no_table[run]['counts'])
    assert (cnt == -1).all(), cnt          # the child took no table


# ---- 5. the layers are in play
@pytest.mark.parametrize('run', TABLED)
def test_draw_prune_in_play(runs, no_prune, run):
    on, off = runs[run]['out'], no_prune[run]
    n_sug = len(SEEDS[run.split('/')[0]])
    assert on['wmax_width'] >= NWT and off['wmax_width'] >= NWT
    cnt = np.asarray(on['counts'])
    for lab in LABELS:
        a = np.frombuffer(bytes.fromhex(on['wmax_' + lab]), dtype=np.uint64).reshape(n_sug, NWT)
        b = np.frombuffer(bytes.fromhex(off['wmax_' + lab]), dtype=np.uint64).reshape(n_sug, NWT)
        c = cnt[:, on['labels'].index(lab)]
        assert ((c > 0) & (c < NWT)).all(), (run, lab, c)   # a tie window, not every tile
        fracs, extras = [], 0
        for s in range(n_sug):
            frac, extra = P.check_wmax_pair(a[s], b[s], (run, lab, s))
            fracs.append(frac)
            extras += extra
        print('%s %s: -inf share of the wave tiles min %.4f median %.4f max %.4f; %d entries -inf '
              'beyond the map prefilter\'s; direct-pass wave tiles %s'
              % (run, lab, min(fracs), float(np.median(fracs)), max(fracs), extras, c.tolist()))


@pytest.mark.parametrize('run', TABLED)
def test_census_credits_the_tables(runs, run):
    """The census on, in a call of its own: exactly the bounded hps' pairs."""
    r = runs[run]
    seeds = SEEDS[run.split('/')[0]]
    r['plan'].census(True)
    r['plan'].suggest(seeds, NC)
    census = r['plan'].census(False, n=13)
    assert census[12] == T._pairs(r['dom'], r['plan'], LABELS, len(seeds)), census
    assert census[12] > 0


def test_over_cap_takes_no_table(runs):
    """K_below = 2480 > 2048: run_level's gates leave the sorted draw and with
    it the tables -- no table launch on this plan (no tab_wmax row, let alone
    a -inf in one; no tile gathered), no pair credited to the tables."""
    r = runs['three/over-cap']
    on = r['out']
    for lab in LABELS:
        a = np.frombuffer(bytes.fromhex(on['wmax_' + lab]), dtype=np.uint64)
        assert not (a == NEG_INF).any(), lab
    assert on['wmax_width'] == 0, on['wmax_width']
    assert (np.asarray(on['counts']) == -1).all(), on['counts']
    r['plan'].census(True)
    r['plan'].suggest(T.SEEDS6, NC)
    census = r['plan'].census(False, n=13)
    assert census[12] == 0, census


# ---- 6. graph replay
def test_graph_replay_across_the_sets():
    """TPE_GRAPH=1 (child): default, wide-below, default, over-cap, pw-zero,
    default, three calls each (eager, capture, replay) -- the captured step is
    keyed on the draw table class, prior_weight and lf, and n_below is patched
    per replay: every call equals the eager one."""
    eager = case_graph()['hex']
    graph = _child('case_graph()', {'TPE_GRAPH': '1'})['hex']
    assert len(eager) == 3 * len(GRAPH_SEQ)
    for k, (g, e) in enumerate(zip(graph, eager)):
        assert g == e, 'call %d (%s)' % (k, GRAPH_SEQ[k // 3])
    assert len(set(eager)) == len(eager)    # (every call has its own first seed)
