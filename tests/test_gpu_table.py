"""Large draws scored from certified Chebyshev tables of both mixtures
(k_table_build / k_score_table).

Common shape: uniform(-5, 5), loguniform(log 1e-3, log 10) and a normal that
takes no table; N = 6000 trials (K_above = 5981: the 16-wide moment class);
n = 2^18 + 8192 + 37 candidates per suggestion -- just over the table's gate,
ending in a partial sort block.  A suggest call takes the sorted draw (and with
it the wave tiles the tables replace) from 2^22 candidates per level and chunk,
so the calls here carry 6 suggestions (11 where a chunk or shard must stay
above that size on its own).

The lpdf bound 2^-27 max(1, |lpdf|) is derived: 2^-28 from the panel
certificate plus fp64 rounding.  Environment switches are read once per
process: their runs are child interpreters.
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

from golden_io import load, load_json, unpack
from gpu_util import assert_winners_match

pytestmark = pytest.mark.gpu

N = 6000
NC = (1 << 18) + 8192 + 37
SEEDS6 = [9001 + 13 * s for s in range(6)]
SEEDS11 = [7001 + 17 * s for s in range(11)]
SEEDS12 = SEEDS6 + [5001 + 19 * s for s in range(6)]
CUT = 17 * 8192          # a shard / chunk boundary: whole sort blocks
GAP = (-3.0, 0.0)        # tools/table_error.py --gap u:-3:0: 2 uncertified panels of u above
BOUND = 2.0 ** -27
GROW = (3984, 3990, 3996, 4002, 4008, 4014)   # history lengths across mom_width's 4000


def _space():
    return {'u': hp.uniform('u', -5, 5), 'n': hp.normal('n', 0.5, 2.0),
            'lu': hp.loguniform('lu', math.log(1e-3), math.log(10))}


def _history(dom, gap=False):
    rs = np.random.RandomState(11)
    cols = {'u': rs.uniform(-5, 5, N), 'n': rs.normal(0.5, 2.0, N),
            'lu': np.exp(rs.uniform(math.log(1e-3), math.log(10), N))}
    if gap:   # (tools/table_error.py apply_gap)
        x, (lo, hi) = cols['u'], GAP
        ins, mid = (x > lo) & (x < hi), 0.5 * (lo + hi)
        cols['u'] = np.where(ins & (x < mid), x - (hi - lo), np.where(ins, x + (hi - lo), x))
    vals = np.stack([cols[l] for l in dom.space.labels])
    return np.random.RandomState(12).rand(N), vals, np.ones_like(vals, dtype=np.uint8)


def _plan(gap=False):
    dom = Domain(lambda x: 0.0, _space())
    L, vals, act = _history(dom, gap)
    hps, conds, pprior = dom.space.engine_tables()
    plan = E.Plan(E.default_engine(), hps, conds, pprior, max_trials=N)
    plan.set_history(L, vals, act)
    plan.fit()
    return dom, plan, (L, vals, act)


def _pairs(dom, plan, labels, n_sug):
    """Pairs a table-scored suggest credits to the hps ``labels``."""
    k = sum(plan.mixture(dom.space.by_label[l].index, s)[0].size for l in labels for s in (0, 1))
    return n_sug * NC * k


def _hex(a):
    return a.view(np.uint8).tobytes().hex()


def _unhex(h, like):
    return np.frombuffer(bytes.fromhex(h), dtype=like.dtype).reshape(like.shape)


def case_suggest(gap=False):
    """One 6-suggestion call: records and the census."""
    dom, plan, _ = _plan(gap)
    plan.census(True)
    res = plan.suggest(SEEDS6, NC)
    return dict(hex=_hex(res), census=list(plan.census(False, n=13)))


def case_chunks():
    dom, plan, _ = _plan()
    plan.profile(16)
    res = plan.suggest(SEEDS11, NC)
    return dict(hex=_hex(res), launches=plan.profile_read(0)[1])


def case_grow():
    """fit_suggest over a history growing across mom_width's threshold."""
    dom = Domain(lambda x: 0.0, _space())
    L, vals, act = _history(dom)
    hps, conds, pprior = dom.space.engine_tables()
    plan = E.Plan(E.default_engine(), hps, conds, pprior, max_trials=N)
    out = []
    for i, n in enumerate(GROW):
        plan.set_history(L[:n], np.ascontiguousarray(vals[:, :n]), np.ascontiguousarray(act[:, :n]))
        out.append(_hex(plan.fit_suggest([31 + i] + SEEDS6[1:], NC)))
    return dict(hex=out)


def _child(case, env):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, json; sys.path.insert(0, 'tests'); import test_gpu_table as T; "
            "print('JSON' + json.dumps(T.%s))" % case)
    r = subprocess.run([sys.executable, '-c', code], cwd=root, env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.split('JSON')[-1])


@pytest.fixture(scope='module')
def common():
    dom, plan, hist = _plan()
    from test_gpu_shifted import _oracle_obs
    return dom, plan, _oracle_obs(dom, *hist)


@pytest.fixture(scope='module')
def off_runs():
    return {g: _child('case_suggest(%r)' % g, {'TPE_TABLE': '0'}) for g in (False, True)}


def _panel_points(plan, t, i, side):
    """Panel boundaries of the (hp, side) table in the hp's own domain."""
    sg = plan.mixture(i, side)[2]
    P = int(math.ceil((t.high - t.low) / (2.0 * sg.min())))
    x = t.low + (t.high - t.low) * np.arange(1, P) / P
    return np.exp(x) if t.family == E.LGMM else x


def _assert_lpdf(got, want, msg):
    got, want = np.asarray(got), np.asarray(want)
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print('%s: max |lpdf - ref| / max(1, |ref|) = %.3e (bound %.3e)' % (msg, err.max(), BOUND))
    assert np.isfinite(got).all() and err.max() <= BOUND, (msg, float(err.max()))


def test_table_lpdf_vs_oracle(common):
    """Mode 4 (the tables alone) on both bounded hps: 4096 candidates -- below
    posterior draws, the prior range, low, the last double under high and every
    panel boundary of both tables -- within 2^-27 of the oracle on both sides;
    the normal has no table."""
    from test_gpu_shifted import _oracle_score
    dom, plan, obs = common
    tabs = dom.space.engine_tables()[0]
    plan.fit()
    rs = np.random.RandomState(3)
    for lab in ('u', 'lu'):
        i = dom.space.by_label[lab].index
        t = tabs[i]
        w, mu, sg = plan.mixture(i, 0)
        edge = np.concatenate([_panel_points(plan, t, i, 0), _panel_points(plan, t, i, 1)])
        ends = np.array([t.low, np.nextafter(t.high, -np.inf)])
        if t.family == E.LGMM:
            ends = np.array([math.exp(t.low), np.nextafter(math.exp(t.high), -np.inf)])
        wide = rs.uniform(t.low, t.high, 1024)
        wide = np.exp(wide) if t.family == E.LGMM else wide
        draws = plan.engine.sample(t.family, w, mu, sg, t.low, t.high, None, seed=99, stream=i,
                                   n=4096 - edge.size - ends.size - wide.size)
        x = np.concatenate([draws, wide, ends, edge])
        assert x.size == 4096
        ref = _oracle_score(dom, obs, lab, x)
        lb, la, bi, bs = plan.score_candidates(i, x, sorted_mode=4)
        _assert_lpdf(lb, ref['llik_b'], lab + ' below')
        _assert_lpdf(la, ref['llik_a'], lab + ' above')
    with pytest.raises(Exception):
        plan.score_candidates(dom.space.by_label['n'].index, np.zeros(8), sorted_mode=4)


def test_table_lpdf_cfg4_reference(cfg4_plan):
    """Four labels of suggest_cfg4.npz (the reference's own candidates and
    lliks, K_a = 9976) through mode 4, same bound."""
    dom, plan = cfg4_plan
    meta = load_json('suggest_big_meta.json')['cfg4']
    d = load('suggest_cfg4.npz')
    for k, lab in list(enumerate(meta['labels']))[:4]:
        x = unpack(d, 'samples', k)
        lb, la, bi, bs = plan.score_candidates(dom.space.by_label[lab].index, x, sorted_mode=4)
        _assert_lpdf(lb, unpack(d, 'llik_b', k), 'cfg4 %s below' % lab)
        _assert_lpdf(la, unpack(d, 'llik_a', k), 'cfg4 %s above' % lab)


def test_suggest_table_vs_direct(common, off_runs):
    """TPE_TABLE on (here) against off (child): the same winners or EI ties
    (in fact the same bytes), every winner against the oracle; the census credits exactly the bounded
    hps' pairs to the tables, none with the switch off."""
    from test_gpu_shifted import _check_winners
    dom, plan, obs = common
    plan.fit()
    plan.census(True)
    on = plan.suggest(SEEDS6, NC)
    census = plan.census(False, n=13)
    off = _unhex(off_runs[False]['hex'], on)
    assert_winners_match(on, off, msg='table vs direct')
    # (more than the ties that allows: k_score_wave scores again every wave
    # within its own error of the best table score, so the records are its own)
    np.testing.assert_array_equal(on.view(np.uint8), off.view(np.uint8))
    for s, sd in enumerate(SEEDS6):
        _check_winners(dom, plan, on[s], sd, NC, obs, 'table s=%d' % s)
    # (exact: both bounded hps, every candidate; nothing from the normal)
    assert census[12] == _pairs(dom, plan, ('u', 'lu'), len(SEEDS6)), census
    assert census[12] > 0 and off_runs[False]['census'][12] == 0


def test_uncertified_slot_falls_back(off_runs):
    """A 3-unit empty gap in u's history leaves two panels of its above table
    uncertified (tools/table_error.py --gap u:-3:0): u's records are those of
    the TPE_TABLE=0 run byte for byte, lu still takes its tables."""
    dom, plan, _ = _plan(gap=True)
    plan.census(True)
    on = plan.suggest(SEEDS6, NC)
    census = plan.census(False, n=13)
    off = _unhex(off_runs[True]['hex'], on)
    iu = dom.space.by_label['u'].index
    np.testing.assert_array_equal(np.ascontiguousarray(on[:, iu]).view(np.uint8),
                                  np.ascontiguousarray(off[:, iu]).view(np.uint8))
    assert census[12] == _pairs(dom, plan, ('lu',), len(SEEDS6)), census
    with pytest.raises(Exception):
        plan.score_candidates(iu, np.zeros(8), sorted_mode=4)
    assert_winners_match(on, off, msg='gap history, table vs direct')


def test_table_invariances(common):
    """Bit for bit: fit_suggest = fit + suggest; a 12-suggestion call = two
    calls of 6; several candidate chunks (TPE_CHUNK_MB=36, child) = one; two
    shards passed the same n_total and merged = the single run."""
    torch = pytest.importorskip('torch')
    dom, plan, obs = common
    plan.fit()
    plan.census(True)
    plan.suggest(SEEDS6, NC)
    assert plan.census(False, n=13)[12] > 0   # the tables are in play
    # (census off from here: the counting kernels are instantiations of their
    # own, whose scores may differ from the plain ones' in the last bits, with
    # or without tables)
    a = plan.suggest(SEEDS6, NC)
    b = plan.fit_suggest(SEEDS6, NC)
    np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
    both = plan.suggest(SEEDS12, NC)
    halves = np.concatenate([plan.suggest(SEEDS12[:6], NC), plan.suggest(SEEDS12[6:], NC)])
    np.testing.assert_array_equal(both.view(np.uint8), halves.view(np.uint8))
    one = plan.suggest(SEEDS11, NC)
    ch = _child('case_chunks()', {'TPE_CHUNK_MB': '36'})
    assert ch['launches'] >= 2, ch['launches']
    np.testing.assert_array_equal(_unhex(ch['hex'], one).view(np.uint8), one.view(np.uint8))
    parts = [plan.suggest(SEEDS11, CUT, cand_begin=0, n_total=NC),
             plan.suggest(SEEDS11, NC - CUT, cand_begin=CUT, n_total=NC)]
    raw = torch.from_numpy(np.stack(parts).view(np.uint8).reshape(-1).copy()).cuda()
    merged = plan.merge(raw.data_ptr(), world=2, level=0, n_suggest=len(SEEDS11))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(merged.view(np.uint8), one.view(np.uint8))


def test_table_graph_replay_matches_eager():
    """TPE_GRAPH=1 (child) over a history that grows across the 16-wide
    moment threshold -- the table choice is part of the captured step's key:
    every call equals the eager one."""
    eager = case_grow()['hex']
    graph = _child('case_grow()', {'TPE_GRAPH': '1'})['hex']
    assert graph == eager
