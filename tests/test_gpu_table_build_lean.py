"""The lean build of the Chebyshev tables (k_table_terms +
k_table_build_lean: each component's certificate terms once per slot, and no
addition that changes no bit) against k_table_build, which the same library
keeps behind TPE_TABLE_LEAN=0.  The switch is read once per process: the
TPE_TABLE_LEAN=0 side is a child interpreter.

Compared for every (hp, side), byte for byte: the header and the panels
(Plan.tab_panels), the certificate's three logarithms per panel
(Plan.tab_cert) and the bound lattice (Plan.tab_bound).

Fixtures, on test_gpu_table.py's history (N = 6000) and the space u, lu:
tools/table_error.py's fit sets default (K 21 / 5981), prior-only (K_below =
1), few-below (3), huge-below (1241 / 4761) and pw-zero (a -inf term first: the
prior's weight is zero); the --gap u:-3:0 history, whose above table of u has
two panels that do not certify -- in both forms; a history of 300 trials
(K_above = 296: a second, partial round of the build's 256 threads) and one of
250 (K_above = 247 < 256: some threads own no component, and K is no multiple
of 8, the coefficient block).  The numpy emulation (tools/table_error.py
build) certifies every other slot: checked here on the CPU, so a slot that
fails on the device is the device's doing.

This module also holds the cases the map's and the gather's tests share
(test_gpu_table_map_lean.py, test_gpu_tie_gather_lean.py): one child process
per environment runs them all.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from hyperopt_amd import hp, _engine as E
from hyperopt_amd.base import Domain

import test_gpu_table as T
import test_gpu_tie_gather as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import table_error as TE  # noqa: E402
from oracle import tpe_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

N, NC = T.N, T.NC
NWT = (NC + 127) // 128            # 2113 wave tiles hold a candidate: 2 x 1024 + 65
LABELS = ('u', 'lu')
SEEDS8 = [9001 + 13 * s for s in range(8)]   # (8 x 2 slots reach the sorted draw's 2^22)
FIT_NAMES = ('default', 'prior-only', 'few-below', 'huge-below', 'pw-zero')
BUILDS = [(n, N, None) for n in FIT_NAMES] + [('default', N, ('u',) + T.GAP), ('default', 300, None),
                                                   ('default', 250, None)]
BUILD_IDS = ['%s-%d%s' % (n, k, '-gap' if g else '') for n, k, g in BUILDS]
LEAN_OFF = {'TPE_TABLE_LEAN': '0'}


def _hex(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes().hex()


def _plan(n=N, gap=None, fit=None, fitted=True):
    """u, lu on tools/table_error.py's test history (test_gpu_table.py's)."""
    losses, cols, _ = TE.test_shape(n, gap)
    dom = Domain(lambda x: 0.0, {l: T._space()[l] for l in LABELS})
    vals = np.stack([cols[l] for l in dom.space.labels])
    act = np.ones_like(vals, dtype=np.uint8)
    hps, conds, pprior = dom.space.engine_tables()
    plan = E.Plan(E.default_engine(), hps, conds, pprior, max_trials=N)
    plan.set_history(losses, vals, act)
    if fitted:
        plan.fit(**TE.fit_params(fit or 'default'))
    return dom, plan


# ---- the build ------------------------------------------------------------
def case_build():
    out = {}
    for key, (name, n, gap) in zip(BUILD_IDS, BUILDS):
        dom, plan = _plan(n, gap, name)
        for lab in LABELS:
            i = dom.space.by_label[lab].index
            for side in (0, 1):
                t = plan.tab_panels(i, side)
                cert = plan.tab_cert(i, side)
                assert cert.shape == (t['P'], 3)
                out['%s/%s/%d' % (key, lab, side)] = dict(
                    hdr=[_hex(np.array([t['y_lo'], t['inv_w']])), t['P'], t['ncert']],
                    panels=_hex(t['panels']), cert=_hex(cert),
                    K=int(plan.mixture(i, side)[0].size))
            try:
                out['%s/%s/U' % (key, lab)] = _hex(plan.tab_bound(i))
            except ValueError:
                out['%s/%s/U' % (key, lab)] = None
    return out


GRAPH_FITS = ('default', 'huge-below', 'default', 'pw-zero', 'default')


def case_graph():
    """fit_suggest on one plan, twice per fit set: under TPE_GRAPH=1 the second
    call of a set replays the captured step, and a set seen again replays after
    a refit with other parameters."""
    dom, plan = _plan(fitted=False)
    out, i = [], 0
    for name in GRAPH_FITS:
        for _ in range(2):
            out.append(T._hex(plan.fit_suggest([31 + i] + SEEDS8[1:], NC, **TE.fit_params(name))))
            i += 1
    return dict(hex=out)


# ---- the suggests the map's and the gather's tests read --------------------
def _suggest(dom, plan, seeds, labels, census=False):
    if census:
        plan.census(True)
    res = plan.suggest(seeds, NC)
    counts = plan.tie_counts(len(seeds))
    out = dict(hex=T._hex(res), counts=counts.tolist(), labels=list(dom.space.labels))
    if census:
        out['census'] = list(plan.census(False, n=13))
    wm = plan.tab_wmax(len(seeds))
    assert wm.shape[:2] == (len(seeds), len(dom.space.labels)), wm.shape
    out['width'] = int(wm.shape[2])
    for lab in labels:
        i = dom.space.by_label[lab].index
        out['wmax_' + lab] = _hex(wm[:, i, :])
        lists = [plan.tie_list(s, i) for s in range(len(seeds))]
        assert [l.size for l in lists] == [max(0, c) for c in counts[:, i]]
        out['list_' + lab] = [_hex(l.astype(np.int32)) for l in lists]
    return out


def _named_plan(name):
    """test_gpu_table_lattice.py's plan of a named history (three copies of
    one uniform hp)."""
    losses, cols, _ = TE.NAMED[name](N)
    dom = Domain(lambda x: 0.0, {l: hp.uniform(l, -5, 5) for l in ('e', 'e2', 'e3')})
    vals = np.stack([cols['e'] for l in dom.space.labels])
    hps, conds, pprior = dom.space.engine_tables()
    plan = E.Plan(E.default_engine(), hps, conds, pprior, max_trials=N)
    plan.set_history(losses, vals, np.ones_like(vals, dtype=np.uint8))
    plan.fit()
    return dom, plan


def case_shape(census=False):
    dom, plan = _plan()
    return _suggest(dom, plan, SEEDS8, LABELS, census)


def case_gap():
    dom, plan = _plan(gap=('u',) + T.GAP)
    return _suggest(dom, plan, SEEDS8, LABELS)


def case_low_edge():
    dom, plan = _named_plan('low-edge')
    return _suggest(dom, plan, T.SEEDS6, ('e',))


def case_cond():
    dom, plan = G._cond_plan()
    out = _suggest(dom, plan, T.SEEDS11, ('u', 'a', 'b'))
    return out


CASES = dict(shape=case_shape, census=lambda: case_shape(True), gap=case_gap,
             low_edge=case_low_edge, cond=case_cond, build=case_build, graph=case_graph)


def run_cases(names):
    return {n: CASES[n]() for n in names}


def child(names, env):
    code = ("import sys, json; sys.path.insert(0, 'tests'); import test_gpu_table_build_lean as B; "
            "print('JSON' + json.dumps(B.run_cases(%r)))" % (list(names),))
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.split('JSON')[-1])


# the environments of the three modules: the cases each runs, in the default
# form (this process for the plain environment, else a child) and under
# TPE_TABLE_LEAN=0 (a child)
ENVS = {
    'plain': ({}, ('shape', 'census', 'gap', 'low_edge', 'cond')),
    'wide': (G.WIDE, ('shape',)),                       # every wave tile hot
    'narrow': ({'TPE_TABLE_TIE_LOG2': '-1074'}, ('shape',)),
    'noprune': ({'TPE_DRAW_PRUNE': '0'}, ('shape',)),   # no dropped tiles: tab_pref 1
}
_runs = {}


def pair(env):
    """(default form, TPE_TABLE_LEAN=0) runs of an environment, made once."""
    if env not in _runs:
        assert os.environ.get('TPE_TABLE_LEAN', '1') != '0', 'the default form is under test'
        extra, names = ENVS[env]
        on = child(names, extra) if extra else run_cases(names)
        _runs[env] = (on, child(names, dict(extra, **LEAN_OFF)))
    return _runs[env]


def unhex(h, dtype):
    return np.frombuffer(bytes.fromhex(h), dtype=dtype)


# ---- tests ------------------------------------------------------------------
@pytest.fixture(scope='module')
def builds():
    return case_build(), child(['build'], LEAN_OFF)['build']


def _emulated_ok(name, n, gap, lab, side):
    losses, cols, specs = TE.test_shape(n, gap)
    dist, args = specs[lab]
    fp = TE.fit_params(name)
    fit, (low, high, pm) = TE.mixtures(losses, cols, lab, dist, args, **fp)
    fam = O.posterior_spec(dist, args, fp['prior_weight'])[0]
    w, mu, sg = fit[side]
    with np.errstate(all='ignore'):
        tab = TE.build(w, mu, sg, low, high, pm, TE.pacc_of(fam, w, mu, sg, low, high))
    assert tab is not None
    return tab['P'], tab['ok']


@pytest.mark.parametrize('key,build', list(zip(BUILD_IDS, BUILDS)), ids=BUILD_IDS)
def test_build_bytes(builds, key, build):
    """Header, panels, certificate and lattice of every (hp, side): the lean
    build's bytes are k_table_build's.  Every slot the emulation certifies is
    certified on the device; the gap history's above table of u is short of
    two panels in both forms."""
    on, off = builds
    name, n, gap = build
    for lab in LABELS:
        for side in (0, 1):
            k = '%s/%s/%d' % (key, lab, side)
            a, b = on[k], off[k]
            P, ok = _emulated_ok(name, n, gap, lab, side)
            print(k, 'K', a['K'], 'P', a['hdr'][1], 'ncert', a['hdr'][2], 'emulated', int(ok.sum()))
            assert a['hdr'] == b['hdr'], k
            assert a['panels'] == b['panels'], k
            cert_a, cert_b = unhex(a['cert'], np.uint64), unhex(b['cert'], np.uint64)
            print(k, 'certificate words differing:', int((cert_a != cert_b).sum()), 'of', cert_a.size)
            assert a['cert'] == b['cert'], k
            assert a['hdr'][1] == P and len(a['panels']) == 2 * 144 * P
            if gap and lab == gap[0] and side == 1:
                assert not ok.all() and a['hdr'][2] == int(ok.sum()) == P - 2, (k, a['hdr'])
            else:
                assert ok.all(), k                       # (the fixture is a certified one)
                assert a['hdr'][2] == P, (k, a['hdr'])
            # the recorded certificate is the one the count came from
            le, lr, lg = unhex(a['cert'], np.float64).reshape(P, 3).T
            with np.errstate(invalid='ignore'):
                passed = np.isfinite(le) & np.isfinite(lg) & (np.maximum(le, lr) + 1.0 <= lg - 28.0)
            assert int(passed.sum()) == a['hdr'][2], k
        assert on['%s/%s/U' % (key, lab)] == off['%s/%s/U' % (key, lab)], (key, lab)
        assert (on['%s/%s/U' % (key, lab)] is None) == bool(gap and lab == gap[0])
    K = on['%s/u/1' % key]['K']
    if n == 300:
        assert K == 296, K
    if n == 250:
        assert K < 256 and K % 8 != 0, K


def test_graph_replay_after_refit():
    """TPE_GRAPH=1 (child): the build with its extra node inside the captured
    step, replayed after refits with other parameters, equals the eager calls."""
    eager = case_graph()['hex']
    graph = child(['graph'], {'TPE_GRAPH': '1'})['graph']['hex']
    assert graph == eager
