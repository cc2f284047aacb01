"""c-TPE on the GPU (tpe_plan_ctpe_*) against ctpe_oracle: the bank's fits, the
totals and the acquisition, dead models, the draws, the picks of the public entry points."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import hyperopt_amd as H
from hyperopt_amd import hp, tpe, rand, Trials, trials_from_docs
from hyperopt_amd import _engine as E
from hyperopt_amd.base import Domain

import ctpe_oracle as CO
import spaces
from test_gpu_points import _term_bound     # the bar of a total: its terms' 1e-6 lpdf bars, summed

pytestmark = pytest.mark.gpu

SPACES = {'many_dists': spaces.many_dists_space, 'cond': spaces.cond_space}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _history(name, n, C, feasible='mixed'):
    """(cs, losses, G[C, n], vals, active) of n prior draws.  'distinct': constraint c feasible in
    about (c + 1) / (C + 2) of the rows -- every model live, each with its own good side -- with
    a NaN value, a pending row, a failed trial; 'mixed': and constraint 1 feasible in all (a
    dead model between live ones); 'all' / 'none': every value -1 / +1."""
    dom = Domain(lambda x: 0.0, SPACES[name](hp))
    docs = rand.suggest(list(range(n)), dom, Trials(), 11)
    rs = np.random.RandomState(n + C)
    losses = rs.rand(n)
    for d, l in zip(docs, losses):
        d['state'] = H.JOB_STATE_DONE
        d['result'] = {'status': 'ok', 'loss': float(l)}
    _, _, vals, act = tpe.build_history(dom, trials_from_docs(docs))
    if feasible in ('all', 'none'):
        return dom.space, losses, np.full((C, n), -1.0 if feasible == 'all' else 1.0), vals, act
    G = rs.rand(C, n) - (np.arange(C)[:, None] + 1.0) / (C + 2.0)
    if C > 1 and feasible == 'mixed':
        G[1] = -rs.rand(n)
    G[0, 3] = np.nan
    losses[5] = np.inf
    G[:, 9] = np.nan                            # (a trial that is not ok)
    losses[9] = np.inf
    for a in (losses, G, vals, act):
        a.setflags(write=False)
    return dom.space, losses, G, vals, act


def _new_plan(cs, losses, vals, act):
    hps, conds, pprior = cs.engine_tables()
    plan = E.Plan(E.default_engine(), hps, conds, pprior, max_trials=losses.size)
    plan.set_history(losses, vals, act)
    return plan


@functools.lru_cache(maxsize=None)
def _fitted(name, n, C, feasible='mixed'):
    cs, losses, G, vals, act = _history(name, n, C, feasible)
    plan = _new_plan(cs, losses, vals, act)
    nb, ghat = tpe.ctpe_counts(losses, G)
    plan.ctpe_fit(np.ascontiguousarray(G), nb, ghat)
    return plan, nb, ghat, CO.counts(losses, G)[2]


@pytest.mark.parametrize('n', [40, 300])
@pytest.mark.parametrize('C', [1, 2, 16])
@pytest.mark.parametrize('name', sorted(SPACES))
def test_bank_fit_is_the_plain_fit_of_each_key_column(name, C, n):
    cs, losses, G, vals, act = _history(name, n, C)
    plan, nb, ghat, live = _fitted(name, n, C)
    got_live, feas = plan.ctpe_info()
    assert got_live.tolist() == live and (C == 1 or 2 not in live)
    ok = np.isfinite(losses)
    with np.errstate(invalid='ignore'):
        assert feas.tolist() == [ok.sum()] + [(ok & (G[m - 1] <= 0)).sum() for m in live[1:]]
    key = CO.keys(losses, G)
    ref = _new_plan(cs, losses, vals, act)
    for m in live:
        ref.set_history(key[m], vals, act)
        ref.fit(gamma=CO.BIG_GAMMA, gamma_cap=int(nb[m]))
        for i in range(len(cs.labels)):
            for side in (0, 1):
                a, b = plan.ctpe_mixture(m, i, side), ref.mixture(i, side)
                assert all(_bits(x).tobytes() == _bits(y).tobytes() for x, y in zip(a, b)), (m, i)


def _configs(name, M):
    """The history's rows in turn; from 63 on one out-of-range choice, one normal hp in a tail."""
    cs, _, _, vals, act = _history(name, 300, 4)
    idx = np.arange(M) % 300
    v = np.where(act[:, idx] == 1, vals[:, idx], np.nan)
    if M >= 63:
        lab = cs.labels.index
        v[lab('top' if name == 'cond' else 'a'), 1] = 3.0        # a choice of 3: upper
        if name == 'cond':                      # normal(0, 1) of the row's own branch
            v[lab('zz%d' % int(v[lab('top'), 2])), 2] = 9.0
        else:
            v[lab('h'), 2] = 400.0                  # lognormal(-2, 2): 4 sigma out
    return v, (1 if M >= 63 else None)


@functools.lru_cache(maxsize=None)
def _scored(name, M):
    plan = _fitted(name, 300, 4)[0]
    return plan.ctpe_score_points(_configs(name, M)[0], want_T=True, want_active=True)


@pytest.mark.parametrize('M', [1, 63, 64, 65, 257])
@pytest.mark.parametrize('name', sorted(SPACES))
def test_totals_and_acquisition_match_the_oracle(name, M):
    cs, losses, G, hv, ha = _history(name, 300, 4)
    plan, nb, ghat, live = _fitted(name, 300, 4)     # four models, each with its own good side
    assert live == [0, 1, 3, 4] and len(set(nb[live])) == 4
    v, bad = _configs(name, M)
    acq, T, active = _scored(name, M)
    want_active = tpe.active_columns(cs, v)
    np.testing.assert_array_equal(active, want_active)
    assert T.shape == (len(live), M) and (name != 'cond' or not want_active.all())
    ok = np.ones(M, dtype=bool)
    if bad is not None:
        ok[bad] = False
        assert np.isnan(T[:, bad]).all() and np.isnan(acq[bad])
        assert name != 'cond' or active[:, bad].sum() == 2      # and it activates no child
    key = CO.keys(losses, G)
    want_T, bar = [], np.zeros(M)
    vo = np.where(ok[None, :], v, hv[:, :1])    # (the oracle is not asked about the NaN one)
    ao = np.where(ok[None, :], want_active, ha[:, :1] == 1).astype(np.uint8)
    for l, m in enumerate(live):
        lb, la = CO.model_lliks(cs, key[m], nb[m], hv, ha, vo, ao)
        with np.errstate(all='ignore'):
            want_T.append(np.where(ao == 1, lb - la, 0.0).sum(axis=0))
        b = _term_bound(lb, la, ao).sum(axis=0)
        bar = bar + b                           # |dL/dT| < 1: the totals' bars add
        err = np.abs(T[l] - want_T[-1])[ok]
        assert np.isfinite(want_T[-1][ok]).all() and (err <= b[ok]).all(), (m, err.max())
    want = CO.acquisition(ghat[live], np.array(want_T))
    assert (np.abs(acq - want)[ok] <= (bar + 1e-12 * np.abs(want))[ok]).all()
    # and it is the rule on the device's own totals, to a few ulps of the L (3 calls and an add)
    Ls = np.array([CO.log_ratio(g, t) for g, t in zip(ghat[live], T)])
    slack = 16 * np.finfo(float).eps * (1.0 + np.abs(Ls).sum(axis=0))
    assert (np.abs(acq + Ls.sum(axis=0))[ok] <= slack[ok]).all()
    if bad is not None:                         # the tail column takes L's hi = v branch
        l = int(T[:, 2].argmin())
        assert T[l, 2] < -5 and np.log1p(-ghat[live][l]) - T[l, 2] > np.log(ghat[live][l])


def test_chunked_walk_changes_no_number():
    """TPE_CHUNK_MB=0 leaves one block of 256 configurations per chunk: 257 take two."""
    code = ("import sys, json; sys.path.insert(0, 'tests'); import test_gpu_ctpe as T; "
            "a = T._scored('cond', 257); print('JSON' + json.dumps("
            "[T._bits(a[0]).tolist(), T._bits(a[1]).tolist(), a[2].tolist()]))")
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=120,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                       env=dict(os.environ, TPE_CHUNK_MB='0'))
    assert r.returncode == 0, r.stderr[-3000:]
    want = _scored('cond', 257)
    assert json.loads(r.stdout.split('JSON')[-1]) == [
        _bits(want[0]).tolist(), _bits(want[1]).tolist(), want[2].tolist()]


def test_dead_models():
    (plan, nb, ghat, live), v = _fitted('cond', 300, 2, 'all'), _configs('cond', 65)[0]
    assert live == [0] and plan.ctpe_info()[0].tolist() == [0] and nb.tolist() == [5, 300, 300]
    acq, T = plan.ctpe_score_points(v, want_T=True)
    total = plan.score_points(v)                # model 0 is the plan's own fit
    assert T.shape == (1, 65) and _bits(T[0]).tobytes() == _bits(total).tobytes()
    L0 = CO.log_ratio(ghat[0], total)
    fin = np.isfinite(L0)                       # (all but the out-of-range choice)
    assert (np.isnan(acq) == np.isnan(L0)).all() and fin.sum() >= 60
    assert (np.abs(acq + L0)[fin] <= 16 * np.finfo(float).eps * (1.0 + np.abs(L0[fin]))).all()
    plan, nb, ghat, live = _fitted('cond', 300, 2, 'none')    # live on the least-violating rows
    assert (live, nb.tolist(), plan.ctpe_info()[1].tolist()) == ([0, 1, 2], [5] * 3, [300, 0, 0])


def _replay(plan, cs, live, seed, lo, hi):
    """Configurations lo .. hi - 1 from tpe_sample on the fetched below mixtures, parents first."""
    hps, conds, _ = cs.engine_tables()
    P = len(hps)
    out = np.full((P, hi - lo), np.nan)
    order = []
    while len(order) < P:
        order += [i for i in range(P) if i not in order and all(par in order for par, _ in conds[
            hps[i].cond_begin:hps[i].cond_begin + hps[i].cond_count])]
    for r, m in enumerate(live):
        cols = np.array([j - lo for j in range(lo, hi) if j % len(live) == r], dtype=int)
        for i in order:
            t = hps[i]
            w, mu, sg = plan.ctpe_mixture(m, i, 0)
            cat = t.family == E.CAT
            draws = plan.engine.sample(
                t.family, w, None if cat else mu, None if cat else sg,
                t.low if t.flags & E.HAS_LOW else None, t.high if t.flags & E.HAS_HIGH else None,
                t.q if t.flags & E.HAS_Q else None, seed=seed, stream=i, offset=lo,
                n=hi - lo)[cols]
            on = np.ones(cols.size, dtype=bool)
            if t.cond_count:
                on[:] = False
                for par, br in conds[t.cond_begin:t.cond_begin + t.cond_count]:
                    on |= out[par, cols] == float(br)
            out[i, cols[on]] = draws[on]
    return out


@pytest.mark.parametrize('C,n_live', [(1, 1), (1, 2), (2, 3), (16, 17)])
@pytest.mark.parametrize('name', sorted(SPACES))
def test_draws_come_from_each_live_model_in_turn(name, C, n_live):
    feasible = 'all' if n_live == 1 else 'distinct'
    cs = _history(name, 40, C, feasible)[0]
    plan, nb, ghat, live = _fitted(name, 40, C, feasible)
    assert len(live) == n_live and len(set(nb[live])) >= min(n_live, 3)    # different good sides
    for seed, m, begin in ((77, 40, 0), (77, 40, 1), (77, 40, 63), (77, 40, 1000)):
        vals, acq, T, active = plan.ctpe_sample_points(seed, m, begin=begin, want_T=True,
                                                       want_active=True)
        want = _replay(plan, cs, live, seed, begin, begin + m)
        assert _bits(vals).tobytes() == _bits(want).tobytes(), begin
        a2, T2, act2 = plan.ctpe_score_points(vals, want_T=True, want_active=True)
        assert _bits(acq).tobytes() == _bits(a2).tobytes()
        assert _bits(T).tobytes() == _bits(T2).tobytes() and (active == act2).all()
        lo = plan.ctpe_sample_points(seed, 17, begin=begin)            # the range in two calls
        hi = plan.ctpe_sample_points(seed, m - 17, begin=begin + 17)
        assert _bits(np.concatenate([lo[0], hi[0]], axis=1)).tobytes() == _bits(vals).tobytes()
        assert _bits(np.concatenate([lo[1], hi[1]])).tobytes() == _bits(acq).tobytes()


def test_draws_past_the_table_take_the_rejection_sampler():
    """2080 feasible trials: 2081 below components, past the 2048 of a draw table."""
    dom = Domain(lambda x: 0.0, spaces.cfg4_space(hp, 2))
    rs = np.random.RandomState(21)
    hv, losses, G = rs.uniform(-5, 5, (2, 2100)), rs.rand(2100), np.full((1, 2100), -1.0)
    G[0, ::105] = 1.0
    plan = _new_plan(dom.space, losses, hv, np.ones((2, 2100), dtype=np.uint8))
    nb, ghat = tpe.ctpe_counts(losses, G)
    plan.ctpe_fit(G, nb, ghat)
    assert nb.tolist() == [12, 2080] and plan.ctpe_mixture(1, 0)[0].size == 2081
    vals, acq = plan.ctpe_sample_points(3, 40, begin=5)
    assert _bits(vals).tobytes() == _bits(_replay(plan, dom.space, [0, 1], 3, 5, 45)).tobytes()
    assert _bits(acq).tobytes() == _bits(plan.ctpe_score_points(vals)).tobytes()


def _trials(name, n, C, objectives=False):
    cs, losses, G, _, _ = _history(name, n, C)
    dom = Domain(lambda x: 0.0, SPACES[name](hp))
    docs = rand.suggest(list(range(n)), dom, Trials(), 11)
    for d, l, g in zip(docs, losses, G.T):
        d['state'] = H.JOB_STATE_DONE
        d['result'] = ({'status': 'ok', 'loss': float(l), 'constraints': [float(x) for x in g]}
                       if np.isfinite(l) else {'status': 'fail'})
        if objectives and np.isfinite(l):
            d['result']['objectives'] = [float(l), float(g[-1])]
    return dom, trials_from_docs(docs)


def test_objectives_feed_the_counts_from_the_device_column():
    dom, trials = _trials('cond', 300, 2, objectives=True)
    _, _, G, _, _ = _history('cond', 300, 2)
    kw = dict(objectives=2, constraints=2, constraint_model='ctpe')
    column = tpe.pareto_ranks(dom, trials, objectives=2)[3]     # the ranking without constraints
    nb, ghat, live = CO.counts(column, np.where(np.isfinite(column)[None, :], G, np.nan))
    tpe.score_configs(_configs('cond', 65)[0], dom, trials, **kw)
    plan = dom._tpe_state.plan
    got_live, feas = plan.ctpe_info()
    assert got_live.tolist() == live == [0, 1] and feas.tolist() == [298, nb[1]]
    aa = dom.space.labels.index('aa')
    assert (plan.mixture(aa, 0)[0].size, plan.ctpe_mixture(1, aa)[0].size) == (nb[0] + 1, nb[1] + 1)


def test_picks_are_the_ranking_of_the_device_acquisition():
    (dom, trials), kw = _trials('cond', 300, 2), dict(constraints=2, constraint_model='ctpe')
    cs = dom.space
    vals, acq = tpe.sample_configs(512, dom, trials, 5, **kw)
    hist = dom._tpe_state.history(dom, trials)
    hv, ha = hist.vals[:, :hist.n], hist.active[:, :hist.n]
    want = tpe.joint_select(acq, None, vals, hv, ha, 3)
    docs = tpe.suggest_joint([300, 301, 302], dom, trials, 5, n_configs=512, n_startup_jobs=0, **kw)
    got = [{lab: v[0] for lab, v in d['misc']['vals'].items() if v} for d in docs]
    assert got == tpe.columns_to_configs(cs, vals[:, want], ~np.isnan(vals[:, want]))
    pool = np.ascontiguousarray(vals[:, :200])
    a, T, active, live = tpe.score_configs(pool, dom, trials, return_terms=True, **kw)
    assert _bits(a).tobytes() == _bits(acq[:200]).tobytes() and live.tolist() == [0, 1]
    assert T.shape == (2, 200) and active['top'].all()
    picks = tpe.rank_pool(a, np.ones(200, dtype=bool), 2)
    docs = tpe.suggest_from_pool([300, 301], dom, trials, 1, pool=pool, n_startup_jobs=0,
                                 skip_seen=False, **kw)
    got = [{lab: v[0] for lab, v in d['misc']['vals'].items() if v} for d in docs]
    assert got == tpe.columns_to_configs(cs, pool[:, picks], ~np.isnan(pool[:, picks]))
    r1 = tpe.sample_configs(64, dom, trials, 5, constraints=2)
    tpe.sample_configs(8, dom, trials, 5, **kw)
    for r in (tpe.sample_configs(64, dom, trials, 5, constraints=2, constraint_model='rank'),
              tpe.sample_configs(64, *_trials('cond', 300, 2), 5, constraints=2)):
        assert all(_bits(x).tobytes() == _bits(y).tobytes() for x, y in zip(r1, r))
