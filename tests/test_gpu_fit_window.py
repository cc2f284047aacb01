"""k_fit's sort of a continuous side of 4097..10000 observations on a 32-bit
window of its keys (tpe_fit.hip window_sort_perm: at most four
stable radix passes over (window key, position) pairs, short runs of equal
window keys ranked by their full keys, every adjacent pair checked, the sort
over all key bytes as the fallback) against that sort, which the same library
keeps behind TPE_FIT_WINDOW=0.  The switch is read once per process: this
process runs the default, one child interpreter runs every case with the
switch off, one more replays the captured step (TPE_GRAPH=1).

Compared in every case, for every hp and both sides, byte for byte: the
mixture (w, mu, sigma), the coefficient table, the block-local fp32 table,
the block envelopes and the two moment tables of the 16-component chunks
(every plan here holds 4000 components or more, the width-16 form) -- the
written part of each: a table is sized for the plan's capacity, its entries
end in padding that nothing writes and that differs between a fresh process
and one that has run other fits; a quantized or categorical slot writes its K
components of the first table alone.  The default's mixtures also against
the oracle through fit_oracle.assert_mixture_bit_exact, with that file's rule
for the log families.

Sizes (the above side of an always-active hp holds n - 25 observations): m =
4096 (the merge tier, as before), 4097 and 4160 (five 64-rows per wave, the
last wave's row short or empty), 9999 and 10000 = kSortCap (ten rows), 10001
(the global-memory sort, as before).

Key patterns at m = 5000: uniform doubles on (-5, 5) (a lossy window in which
some keys meet: ranked); quniform with 51 distinct values (long runs of equal
keys, in position order); loguniform; values 1 + j 2^-52, j < 2^20 (the keys
share all high bits: the window holds every varying bit, no check); values
1 + i 2^-50 in shuffled order with one value at 1e6 (the window holds none of
the bits that order them: one long mixed run, the check fails and the block
takes the fallback -- asserted on the result only); a conditional hp, whose
inactive rows make m differ from n.
"""
import hashlib
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from hyperopt_amd import hp, _engine as E
from hyperopt_amd.base import Domain

from oracle import tpe_oracle as O
from fit_oracle import assert_mixture_bit_exact
import spaces

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (4096, 4097, 4160, 9999, 10000, 10001)
M_PAT = 5000
N_COND = 10001
N_CAND = 4096
SEEDS = [11, 12]


def _n_of(m):
    """The history whose above side holds m observations of an active hp."""
    for n in range(m, m + 40):
        if n - O.n_below_count(n, 0.25) == m:
            return n
    raise AssertionError(m)


def space_sizes(hp):
    return {'u': hp.uniform('u', -5, 5), 'l': hp.loguniform('l', math.log(1e-4), 0)}


def space_patterns(hp):
    return {'u': hp.uniform('u', -5, 5), 'q': hp.quniform('q', 0, 10, 0.2),
            'l': hp.loguniform('l', math.log(1e-4), 0), 'h': hp.uniform('h', 1, 2)}


def space_fallback(hp):
    return {'f': hp.uniform('f', 0, 2e6), 'u': hp.uniform('u', -5, 5)}


def space_cond(hp):
    return hp.choice('top', [{'a': hp.uniform('a', -5, 5)}, {'b': hp.uniform('b', 0, 1)}])


SPACES = dict(sizes=space_sizes, patterns=space_patterns, fallback=space_fallback,
              cond=space_cond)


def _column(lab, h, n, rs):
    if lab == 'h':      # the keys differ in their low 20 bits only
        return 1.0 + rs.randint(1 << 20, size=n) * 2.0 ** -52
    if lab == 'f':      # ordered by bits under the window that the outlier lifts
        v = 1.0 + rs.permutation(n) * 2.0 ** -50
        v[n // 2] = 1e6
        return v
    return O.prior_sample(rs, h['dist'], h['args'], n)


def history(kind, n):
    """(domain, specs, losses[n], vals[P, n], active[P, n]) in label order."""
    dom = Domain(lambda x: 0.0, SPACES[kind](hp))
    specs = spaces.describe(SPACES[kind](spaces.RecordingHP()))
    labels = dom.space.labels
    rs = np.random.RandomState(n + len(labels))
    vals = np.zeros((len(labels), n))
    active = np.ones((len(labels), n), dtype=np.uint8)
    top = rs.randint(2, size=n)
    for i, lab in enumerate(labels):
        if lab == 'top':
            vals[i] = top
            continue
        vals[i] = _column(lab, specs[lab], n, rs)
        for parent, b in specs[lab]['conds']:
            active[i] = top == b
    return dom, specs, rs.rand(n), vals, active


def _plan(kind, n):
    dom, specs, losses, vals, active = history(kind, n)
    hps, conds, pprior = dom.space.engine_tables()
    plan = E.Plan(E.default_engine(), hps, conds, pprior, max_trials=n)
    plan.set_history(losses, np.ascontiguousarray(vals), np.ascontiguousarray(active))
    return dom, specs, plan, (losses, vals, active)


def _sha(a):
    return hashlib.sha1(np.ascontiguousarray(a).view(np.uint8).tobytes()).hexdigest()


def _written(plan, i, side, K, lse):
    """The written part of slot (i, side)'s tables, by table."""
    out = {}
    t0 = plan.table(i, side, 0)
    blocks = t0.view(np.float64).reshape(-1, 4, 8)
    nb = (K + 7) // 8
    if lse:
        # rows x, y, z of every block; the w-row holds the block envelope, 4 floats
        out['coef'] = _sha(blocks[:nb, :3])
        out['env'] = _sha(np.ascontiguousarray(blocks[:nb, 3]).view(np.float32)[:, :4])
        # (a Coef32 block ends in 16 bytes of padding that nothing writes)
        t = plan.table(i, side, 1)
        assert t.size % (t0.size // 256) == 0               # (kcap / 8 blocks)
        out['coef32'] = _sha(t.reshape(t0.size // 256, -1)[:nb, :112])
        # the moment forms of the 16-component chunks, written whole for every
        # chunk, eligible or not (a degree-15 entry is 88 bytes and padding)
        nc, cap = (K + 15) // 16, (t0.size // 32 + 15) // 16
        for which, name, used in ((2, 'mom16', 64), (4, 'mom16h', 88)):
            t = plan.table(i, side, which)
            assert t.size % cap == 0
            out[name] = _sha(t.reshape(cap, -1)[:nc, :used])
    else:
        k = np.arange(K)
        out['coef'] = _sha(blocks[k // 8, :, k % 8])
    return out


def fitted(kind, n, keep=False):
    """Hashes of everything the fit wrote (and the mixtures themselves on
    request), per label and side."""
    dom, specs, plan, hist = _plan(kind, n)
    plan.fit()
    out, mix = {}, {}
    for i, lab in enumerate(dom.space.labels):
        d = specs[lab]['dist']
        lse = d in ('uniform', 'loguniform', 'normal', 'lognormal')
        for side in (0, 1):
            w, mu, sg = plan.mixture(i, side)
            rec = dict(K=int(w.size), w=_sha(w), mu=_sha(mu), sg=_sha(sg))
            rec.update(_written(plan, i, side, w.size, lse))
            out['%s/%d' % (lab, side)] = rec
            mix[lab, side] = (w, mu, sg)
    return (out, mix, specs, dom, hist) if keep else out


def graph_calls(n):
    """fit_suggest three times on one plan (under TPE_GRAPH=1 the later calls
    replay the captured step), then fit() + suggest() on a second."""
    _, _, one, _ = _plan('sizes', n)
    calls = [_sha(one.fit_suggest([31 + i] + SEEDS[1:], N_CAND)) for i in range(3)]
    _, _, two, _ = _plan('sizes', n)
    two.fit()
    return dict(calls=calls, eager=_sha(two.suggest([31] + SEEDS[1:], N_CAND)))


def run_cases(names):
    out = {}
    for name in names:
        kind, n = name.split(':')
        out[name] = graph_calls(int(n)) if kind == 'graph' else fitted(kind, int(n))
    return out


N_PAT = _n_of(M_PAT)
N_GRAPH = _n_of(9999)
FIT_CASES = ['sizes:%d' % _n_of(m) for m in SIZES] + \
    ['patterns:%d' % N_PAT, 'fallback:%d' % N_PAT, 'cond:%d' % N_COND]
_child_runs = {}


def _child(key, names, env):
    if key not in _child_runs:
        code = ("import sys, json; sys.path.insert(0, 'tests'); import test_gpu_fit_window as W; "
                "print('JSON' + json.dumps(W.run_cases(%r)))" % (list(names),))
        r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=dict(os.environ, **env),
                           capture_output=True, text=True, timeout=280)
        assert r.returncode == 0, r.stderr[-3000:]
        _child_runs[key] = json.loads(r.stdout.split('JSON')[-1])
    return _child_runs[key]


def _off():
    """Every case on the sort over all key bytes (one child process)."""
    assert os.environ.get('TPE_FIT_WINDOW', '1') != '0', 'the default form is under test'
    return _child('off', FIT_CASES + ['graph:%d' % N_GRAPH], {'TPE_FIT_WINDOW': '0'})


_default = {}


def _on(name):
    if name not in _default:
        kind, n = name.split(':')
        _default[name] = fitted(kind, int(n), keep=True)
    return _default[name]


def _check_oracle(name, only=None):
    _, mix, specs, dom, (losses, vals, active) = _on(name)
    n = losses.size
    tids = np.arange(n)
    for i, lab in enumerate(dom.space.labels):
        h = specs[lab]
        if h['dist'] in ('randint', 'categorical') or (only and lab not in only):
            continue
        on = active[i] == 1
        sides = O.split_observations(tids[on], vals[i][on], tids, losses, 0.25, 25, kind='stable')
        for side, obs in enumerate(sides):
            msg = '%s %s side %d (m = %d) ' % (name, lab, side, obs.size)
            with np.errstate(all='ignore'):
                fk, pm, ps, low, high, q, tr = O.posterior_spec(h['dist'], h['args'], 1.0)
                tobs = O.transform_obs(obs, tr, low)
            assert mix[lab, side][0].size == obs.size + 1, msg
            assert_mixture_bit_exact(mix[lab, side], tobs, 1.0, pm, ps, O.DEFAULT_LF,
                                     fk == 'lgmm', msg)


def _same(on, off):
    diff = ['%s %s' % (slot, f) for slot in on for f in on[slot] if on[slot][f] != off[slot].get(f)]
    assert on.keys() == off.keys() and not diff, diff


@pytest.mark.parametrize('m', SIZES)
def test_sizes(m):
    name = 'sizes:%d' % _n_of(m)
    on = _on(name)[0]
    assert on['u/1']['K'] == m + 1 and on['l/1']['K'] == m + 1
    _same(on, _off()[name])
    _check_oracle(name)


def test_key_patterns():
    name = 'patterns:%d' % N_PAT
    on, mix = _on(name)[:2]
    assert all(on['%s/1' % lab]['K'] == M_PAT + 1 for lab in 'uqlh')
    assert np.unique(mix['q', 1][1]).size <= 52                 # 51 values and the prior
    bits = np.ascontiguousarray(_on(name)[4][1][_on(name)[3].space.labels.index('h')]).view(np.uint64)
    assert (np.bitwise_or.reduce(bits) ^ np.bitwise_and.reduce(bits)) >> 20 == 0
    _same(on, _off()[name])
    _check_oracle(name)


def test_window_cannot_decide():
    """One long run of equal window keys in shuffled order: the result is the
    full sort's (the block's fallback), byte for byte."""
    name = 'fallback:%d' % N_PAT
    on, mix = _on(name)[:2]
    mu = mix['f', 1][1]
    assert mu.size == M_PAT + 1 and (np.diff(mu) >= 0).all()
    assert mu.max() == 1e6          # the outlier is on this side: the window is lifted off the low bits
    assert np.unique(mu).size >= M_PAT                          # (distinct: no tie to hide behind)
    _same(on, _off()[name])
    _check_oracle(name)


def test_conditional_hp():
    name = 'cond:%d' % N_COND
    on = _on(name)[0]
    assert 4 * 1024 < on['a/1']['K'] - 1 < N_COND - 25 and 4 * 1024 < on['b/1']['K'] - 1
    _same(on, _off()[name])
    _check_oracle(name)


def test_fit_suggest_and_graph_replay():
    """m = 9999: fit_suggest equals fit() + suggest(); the replays of the
    captured step equal the eager calls; each equals the other sort's."""
    name = 'graph:%d' % N_GRAPH
    eager = graph_calls(N_GRAPH)
    assert eager['calls'][0] == eager['eager']
    assert len(set(eager['calls'])) == 3                        # (three different seeds)
    graph = _child('graph', [name], {'TPE_GRAPH': '1'})[name]
    assert graph == eager
    assert _off()[name] == eager
