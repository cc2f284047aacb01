"""anneal.suggest on the device (tpe_plan_anneal, k_anneal_order + k_anneal)
against the host statement of the algorithm in hyperopt_amd.anneal, through
the debug trace (tpe_plan_anneal_trace): anchors, ranks and values replayed
from the uniforms each hp consumed; distributions; conditional routing; the
loss order of a large tied history; determinism, batching, a pending history
patch; and fmin / mix.suggest end to end.

Value checks per kind (replay): 'uniform' bit for bit (pure fp64 arithmetic,
compiled without contraction); the normal kinds within 1e-12 * max(1, |x|)
(Box-Muller's log and cospi are device library calls); quantized kinds the
same lattice point; categorical kinds the same category, leaving out draws
whose u * sum(p) lies within 1e-12 of a partial sum (at most 0.1 % of them).

loguniform is exp(a + (b - a) u) with a, b = mid -+ half and mid the clipped
log of the anchor: fp64 arithmetic between two library calls.  The device's
log and exp (OCML, 1 ulp) and numpy's (1 ulp) need not round alike, so bit
equality cannot be had; the check is the tightest the formats give.  With L =
max(|low|, |high|) of the log-space bounds, the two sides' log(anchor) differ
by at most 2 ulp(L); clipping is monotone, and the five roundings from mid to
the draw fall alike or one ulp(L) apart, so the log-space draws differ by at
most tol_x = 4 ulp(L); exp turns that into a relative difference and adds
its own 2 ulp.  Asserted: |got - want| <= (tol_x + 4 ulp(1)) |want| (2.7e-15
for hp d, 8e-15 for the lr hps, against 1e-12 for the normal kinds), log(got)
within tol_x of [a, b), and at most a quarter of the values not bit-equal: a
wrong formula or a contracted multiply-add moves nearly all of them, two 1-ulp
libraries a minority.  Measured on the MI355X: 137 of 1491 differ, by one ulp
(2.2e-16 relative).
"""
import functools
import math

import numpy as np
import pytest
from scipy import stats

import spaces
from hyperopt_amd import anneal, fmin, hp, mix, rand, tpe, Trials
from hyperopt_amd import JOB_STATE_DONE
from hyperopt_amd import _engine as E
from hyperopt_amd.base import Domain

pytestmark = pytest.mark.gpu
ALPHA = 1e-4


# --------------------------------------------------------------------------
# histories and plans
# --------------------------------------------------------------------------
def _domain(space):
    return Domain(lambda x: 0.0, space)


def _docs(dom, n, seed):
    return rand.suggest(list(range(n)), dom, Trials(), seed)


def _columns(cs, docs):
    n = len(docs)
    vals = np.zeros((len(cs.labels), n))
    active = np.zeros((len(cs.labels), n), dtype=np.uint8)
    for r, d in enumerate(docs):
        for lab, v in d['misc']['vals'].items():
            if v:
                vals[cs.by_label[lab].index, r] = float(v[0])
                active[cs.by_label[lab].index, r] = 1
    return vals, active


def _history(kind, n):
    """(domain, losses, vals, active): n rows of `kind`'s space.  cond
    histories of more than 64 rows keep branch 2 out of rows < 64, so its
    children's first anchor lies in the second 64-row chunk of the order."""
    dom = _domain({'many_dists': spaces.many_dists_space, 'cond': spaces.cond_space}[kind](hp))
    cs = dom.space
    docs = _docs(dom, 4 * n + 8, 100 + n)
    if kind == 'cond' and n > 64:
        top = [d['misc']['vals']['top'][0] for d in docs]
        head = [d for d, b in zip(docs, top) if b != 2][:64]
        late = [d for d, b in zip(docs, top) if b == 2][:(n - 64 + 1) // 2]
        rest = [d for d in docs if not any(d is x for x in head + late)]
        docs = head + late + rest
    docs = docs[:n]
    vals, active = _columns(cs, docs)
    losses = np.random.RandomState(200 + n).rand(n)
    if n == 3:
        losses[:] = np.inf                      # every trial pending
    if n == 7:
        losses[4] = np.inf
    if n == 130:
        losses = np.round(losses * 100) / 100   # ties
        losses[[17, 60, 129]] = np.inf
    if kind == 'cond' and n > 64:
        j = cs.by_label['lr2'].index
        assert active[j, :64].sum() == 0 and active[j, 64:].sum() >= 1
    return dom, losses, vals, active


def _plan(dom, losses, vals, active, cap=None):
    cs = dom.space
    hps, conds, pprior = cs.engine_tables()
    plan = E.Plan(E.default_engine(), hps, conds, pprior, max(len(losses), 1) if cap is None else cap)
    plan.set_anneal_order([cs.by_label[lab].index for lab in cs.draw_order])
    plan.set_history(losses, vals, active)
    return plan


# --------------------------------------------------------------------------
# host replay of one call from its trace
# --------------------------------------------------------------------------
def _replay(cs, losses, vals, active, res, trace, abi, sc):
    """Check every (s, hp) record of an anneal call; returns (categorical
    draws, of those left out as too close to a partial sum, fresh anchors,
    reused anchors, prior draws, loguniform draws, of those not bit-equal
    to the host's)."""
    order = anneal.loss_order(losses)
    n_cat = n_near = n_fresh = n_reuse = n_prior = n_log = n_log_diff = 0
    for s in range(res.shape[0]):
        best, chosen = [], {}
        for lab in cs.draw_order:
            h = cs.by_label[lab]
            j = h.index
            r, t = res[s, j], trace[s, j]
            act = cs.is_active(lab, chosen)
            assert bool(r['active']) == act, (s, lab)
            u = [float(x) for x in t['u']]
            if not act:
                assert r['index'] == -1 and math.isnan(r['value']) and math.isnan(r['score'])
                assert t['row'] == -1 and t['rank'] == -1 and all(math.isnan(x) for x in u)
                continue
            col = active[j]
            T = int(np.count_nonzero(col))
            n_val = 2 if h.dist in anneal.NORMAL else 1
            prior = T == 0
            if prior:
                assert t['row'] == -1 and t['rank'] == -1 and r['index'] == 0 and r['score'] == 0
                params = anneal.value_params(h.dist, h.args, None, 1.0)
                uv = u
                n_prior += 1
            else:
                row = anneal.reuse_anchor(best, col)
                if row is None:
                    rank = anneal.rank_from_uniform(u[0], abi, T)
                    assert t['rank'] == rank, (s, lab, u[0], t['rank'], rank)
                    row = anneal.choose_anchor(order, col, rank)
                    best.append(row)
                    uv = u[1:]
                    n_fresh += 1
                else:
                    assert t['rank'] == -1, (s, lab)
                    uv = u
                    n_reuse += 1
                assert t['row'] == row and r['index'] == row, (s, lab, t['row'], r['index'], row)
                assert r['score'] == losses[row]
                params = anneal.value_params(h.dist, h.args, vals[j, row], anneal.shrink(T, sc))
            assert not any(math.isnan(x) for x in uv[:n_val]), (s, lab, u)
            assert all(math.isnan(x) for x in uv[n_val:]), (s, lab, u)
            want = anneal.value_from_uniforms(h.dist, h.args, params, uv[:n_val], prior=prior)
            got = float(r['value'])
            if h.dist in anneal.CATEGORICAL:
                n_cat += 1
                p = params[1]
                near = False
                if not (prior and h.dist == 'randint'):
                    x = uv[0] * float(np.sum(p))
                    near = bool(np.any(np.abs(np.cumsum(p) - x) <= 1e-12))
                if near:
                    n_near += 1
                else:
                    assert got == want, (s, lab, got, want)
                assert got == int(got) and 0 <= got < len(p)
            elif h.dist == 'uniform':
                assert got == want, (s, lab, got.hex(), want.hex())
            elif h.dist == 'loguniform':
                n_log += 1
                n_log_diff += got != want
                tol_x = 4 * np.spacing(max(abs(float(h.args[0])), abs(float(h.args[1]))))
                assert abs(got - want) <= (tol_x + 4 * np.spacing(1.0)) * abs(want), \
                    (s, lab, got.hex(), want.hex())
                assert params[1] - tol_x <= math.log(got) < params[2] + tol_x, (s, lab, got, params)
            elif h.dist.startswith('q'):
                assert got == want, (s, lab, got, want)
            else:
                assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (s, lab, got, want)
            chosen[lab] = int(got) if h.is_categorical else got
    return n_cat, n_near, n_fresh, n_reuse, n_prior, n_log, n_log_diff


# --------------------------------------------------------------------------
# 1. exact replay from the trace
# --------------------------------------------------------------------------
@pytest.mark.parametrize('n', [0, 1, 3, 7, 65, 130])
@pytest.mark.parametrize('kind', ['many_dists', 'cond'])
def test_exact_replay_from_trace(kind, n):
    dom, losses, vals, active = _history(kind, n)
    plan = _plan(dom, losses, vals, active)
    S = 257
    for abi, sc in ((2.0, 0.1), (50.0, 0.0)):
        res = plan.anneal(tpe.batch_seeds(1000 + n, S), abi, sc)
        trace = plan.anneal_trace(S)
        assert res.tobytes() == plan.results().tobytes()
        n_cat, n_near, n_fresh, n_reuse, n_prior, n_log, n_log_diff = _replay(
            dom.space, losses, vals, active, res, trace, abi, sc)
        assert n_near <= 0.001 * n_cat
        assert n_log >= S // 4 and n_log_diff <= 0.25 * n_log, (n_log, n_log_diff)
        if n == 0:
            assert n_fresh == n_reuse == 0 and n_prior > 0
        else:
            assert n_fresh >= S
            assert n_reuse > 0 or kind == 'cond'
    if kind == 'cond' and n == 130:
        # the children of branch 2 are active from row 64 on only: their anchors
        j = dom.space.by_label['lr2'].index
        rows = trace[:, j]['row']
        assert (rows[rows >= 0] >= 64).all() and (rows >= 64).any()


# --------------------------------------------------------------------------
# 2. rank clip and spread
# --------------------------------------------------------------------------
def test_rank_clip_and_spread():
    dom = _domain({'x': hp.uniform('x', -5, 5)})
    losses = np.array([0.3, 0.1, 0.2])
    vals = np.array([[1.0, -2.0, 4.0]])
    active = np.ones((1, 3), dtype=np.uint8)
    plan = _plan(dom, losses, vals, active)
    S = 20000
    res = plan.anneal(tpe.batch_seeds(7, S), 50.0, 0.1)
    tr = plan.anneal_trace(S)[:, 0]
    assert tr['rank'].min() >= 0 and tr['rank'].max() <= 2
    p = 1.0 / 50.0
    want = np.array([p, p * (1 - p), (1 - p) ** 2]) * S
    cnt = np.bincount(tr['rank'], minlength=3)
    assert stats.chisquare(cnt, want).pvalue > ALPHA, cnt
    np.testing.assert_array_equal(tr['row'], np.array([1, 2, 0])[tr['rank']])
    np.testing.assert_array_equal(res[:, 0]['index'], tr['row'])
    plan.anneal(tpe.batch_seeds(8, S), 1.0, 0.1)
    tr = plan.anneal_trace(S)[:, 0]
    assert (tr['rank'] == 0).all() and (tr['row'] == 1).all()


def test_argument_checks():
    dom, losses, vals, active = _history('many_dists', 7)
    plan = _plan(dom, losses, vals, active)
    for abi, sc in ((0.5, 0.1), (2.0, -0.1), (math.inf, 0.1), (2.0, math.nan), (math.nan, 0.1)):
        with pytest.raises(ValueError):
            plan.anneal([1], abi, sc)
    with pytest.raises(ValueError):
        plan.anneal([], 2.0, 0.1)


def test_hp_order_is_the_hosts():
    """The walk order comes from the host (CompiledSpace.draw_order).  z is
    unconditional and also sits under choice c: the host visits c first, so c
    draws the fresh anchor and z reuses it; ids descending alone would not."""
    z = hp.uniform('z', 0, 1)
    dom = _domain({'c': hp.choice('c', [{'zz': z}, 1]), 'z': z})
    cs = dom.space
    assert cs.draw_order == ['c', 'z'] and cs.by_label['z'].conds() == ()
    vals, active = _columns(cs, _docs(dom, 9, 3))
    losses = np.random.RandomState(4).rand(9)
    plan = _plan(dom, losses, vals, active)
    res = plan.anneal(tpe.batch_seeds(6, 65), 2.0, 0.1)
    trace = plan.anneal_trace(65)
    _replay(cs, losses, vals, active, res, trace, 2.0, 0.1)
    assert (trace[:, cs.by_label['c'].index]['rank'] >= 0).all()
    assert (trace[:, cs.by_label['z'].index]['rank'] == -1).all()
    # an order is required, and checked: a permutation, choices before their hps
    hps, conds, pprior = cs.engine_tables()
    bare = E.Plan(E.default_engine(), hps, conds, pprior, 9)
    bare.set_history(losses, vals, active)
    with pytest.raises(ValueError):
        bare.anneal([1], 2.0, 0.1)
    for bad in ([0], [0, 0], [0, 2]):
        with pytest.raises(ValueError):
            bare.set_anneal_order(bad)
    cd = _domain(spaces.cond_space(hp)).space
    h2, c2, p2 = cd.engine_tables()
    order = [cd.by_label[lab].index for lab in cd.draw_order]
    with pytest.raises(ValueError):
        E.Plan(E.default_engine(), h2, c2, p2, 4).set_anneal_order(order[::-1])


# --------------------------------------------------------------------------
# 3. distributions
# --------------------------------------------------------------------------
@pytest.fixture(scope='module')
def many120():
    dom = _domain(spaces.many_dists_space(hp))
    docs = _docs(dom, 120, 31)
    vals, active = _columns(dom.space, docs)
    losses = np.random.RandomState(32).rand(120)
    return dom, losses, vals, active, _plan(dom, losses, vals, active)


def test_distributions_all_kinds(many120):
    dom, losses, vals, active, plan = many120
    cs = dom.space
    S, sc = 20000, 0.1
    res = plan.anneal(tpe.batch_seeds(99, S), 2.0, sc)
    assert res['active'].all()
    # a flat space: the first hp draws the anchor, every later one reuses it
    row = res[:, 0]['index']
    assert (res['index'] == row[:, None]).all()
    assert len(np.unique(row)) > 5
    shr = anneal.shrink(120, sc)
    col = {h.label: res[:, h.index]['value'] for h in cs.hps}
    anchor = {h.label: vals[h.index][row] for h in cs.hps}
    # bounded: back through [mid - half, mid + half) to U(0, 1)
    for lab, low, high, lg in (('c', 4.0, 7.0, False), ('d', -2.0, 0.0, True)):
        half = .5 * (high - low) * shr
        mid = np.clip(np.log(anchor[lab]) if lg else anchor[lab], low + half, high - half)
        x = np.log(col[lab]) if lg else col[lab]
        t = (x - (mid - half)) / (2 * half)
        assert t.min() >= -1e-12 and t.max() < 1 + 1e-12
        assert stats.kstest(t, 'uniform').pvalue > ALPHA, lab
    # normal: standardized residuals to N(0, 1)
    for lab, sigma, lg in (('g', 7.0, False), ('h', 2.0, True)):
        mu = np.log(anchor[lab]) if lg else anchor[lab]
        z = ((np.log(col[lab]) if lg else col[lab]) - mu) / (sigma * shr)
        assert stats.kstest(z, 'norm').pvalue > ALPHA, lab
    # quantized: on the lattice
    for lab, q in (('e', 3.0), ('f', 2.0), ('i', 2.0), ('j', 1.0)):
        assert np.all(col[lab] == np.round(col[lab] / q) * q), lab
    # categorical: conditional on the anchor's category, the blended p
    for lab, prior in (('a', np.full(3, 1 / 3)), ('b', np.full(10, 0.1)),
                       ('k', np.array([.1, .9]))):
        tested = 0
        for c in np.unique(anchor[lab]).astype(int):
            sel = anchor[lab].astype(int) == c
            p = shr * prior
            p[c] += 1 - shr
            exp = p / p.sum() * sel.sum()
            if exp.min() < 5:
                continue
            cnt = np.bincount(col[lab][sel].astype(int), minlength=len(prior))
            assert stats.chisquare(cnt, exp).pvalue > ALPHA, (lab, c, cnt)
            tested += 1
        assert tested >= 1, lab


def test_no_shrink_keeps_the_prior_width(many120):
    dom, losses, vals, active, plan = many120
    cs = dom.space
    res = plan.anneal(tpe.batch_seeds(5, 20000), 2.0, 0.0)
    c = res[:, cs.by_label['c'].index]['value']
    d = res[:, cs.by_label['d'].index]['value']
    assert stats.kstest(c, stats.uniform(4, 3).cdf).pvalue > ALPHA
    assert stats.kstest(np.log(d), stats.uniform(-2, 2).cdf).pvalue > ALPHA
    e = res[:, cs.by_label['e'].index]['value']
    assert set(np.unique(e)) <= {0.0, 3.0, 6.0, 9.0}


# --------------------------------------------------------------------------
# 4. conditional routing
# --------------------------------------------------------------------------
def test_conditional_routing_and_unobserved_branch():
    dom = _domain(spaces.cond_space(hp))
    cs = dom.space
    docs = [d for d in _docs(dom, 400, 11) if d['misc']['vals']['top'][0] != 2][:120]
    vals, active = _columns(cs, docs)
    losses = np.random.RandomState(12).rand(120)
    plan = _plan(dom, losses, vals, active)
    S = 4096
    res = plan.anneal(tpe.batch_seeds(3, S), 2.0, 0.1)
    trace = plan.anneal_trace(S)
    top = res[:, cs.by_label['top'].index]['value'].astype(int)
    assert set(np.unique(top)) == {0, 1, 2}
    for b in range(3):
        for lab in ('lr%d' % b, 'units%d' % b, 'act%d' % b, 'zz%d' % b):
            j = cs.by_label[lab].index
            np.testing.assert_array_equal(res[:, j]['active'].astype(bool), top == b)
            if b == 2:      # never observed: prior draws, no anchor
                assert (trace[top == 2, j]['row'] == -1).all()
                assert (res[top == 2, j]['index'] == 0).all()
    u = res[top == 2, cs.by_label['units2'].index]['value']
    assert len(u) > 20 and np.all((u >= 1) & (u <= 1024) & (u == np.round(u)))
    # the anchor lists of the suggestions that took branch 2 (host best-list logic)
    pick = np.where(top == 2)[0][:64]
    _replay(cs, losses, vals, active, res[pick], trace[pick], 2.0, 0.1)


# --------------------------------------------------------------------------
# 5. large history
# --------------------------------------------------------------------------
def test_large_tied_history_order():
    """n = 20000 rows, losses rounded to two decimals (101 distinct values:
    tie groups of ~200 rows), x active in the rows r % 3 != 0 and y in the
    rows r % 3 == 0, so each hp of every suggestion draws a fresh anchor.  The
    loss order has one path for every history size -- a stable LSD radix sort
    by one block, 16 passes of 4 bits over global ping-pong buffers, each wave
    ranking 64-row chunks by ballot; no LDS-resident variant -- so this size
    runs the same code as the small ones, at 20 chunks per wave and 313 order
    chunks per walk."""
    n, S = 20000, 4096
    dom = _domain({'x': hp.uniform('x', 0, 1), 'y': hp.uniform('y', 0, 1)})
    cs = dom.space
    rng = np.random.RandomState(77)
    losses = np.round(rng.rand(n) * 100) / 100
    vals = rng.rand(2, n)
    active = np.zeros((2, n), dtype=np.uint8)
    jx, jy = cs.by_label['x'].index, cs.by_label['y'].index
    active[jy, 0::3] = 1
    active[jx] = 1 - active[jy]
    plan = _plan(dom, losses, vals, active)
    abi = 400.0
    res = plan.anneal(tpe.batch_seeds(21, S), abi, 0.1)
    trace = plan.anneal_trace(S)
    order = anneal.loss_order(losses)
    for j in (jx, jy):
        rows = order[active[j][order] != 0]
        T = len(rows)
        t = trace[:, j]
        g = np.ceil(np.log1p(-t['u'][:, 0]) / math.log1p(-1.0 / abi))
        rank = np.clip(g - 1, 0, T - 1).astype(int)
        np.testing.assert_array_equal(t['rank'], rank)
        assert rank.max() > 640                       # beyond ten chunks of the walk
        np.testing.assert_array_equal(t['row'], rows[rank])
        np.testing.assert_array_equal(res[:, j]['index'], rows[rank])
        np.testing.assert_array_equal(res[:, j]['score'], losses[rows[rank]])


# --------------------------------------------------------------------------
# 6. determinism and batching
# --------------------------------------------------------------------------
def test_determinism_and_batching():
    dom, losses, vals, active = _history('cond', 65)
    plan = _plan(dom, losses, vals, active)
    seeds = tpe.batch_seeds(424242, 16)
    a = plan.anneal(seeds, 2.0, 0.1)
    b = plan.anneal(seeds, 2.0, 0.1)
    assert a.tobytes() == b.tobytes()
    for s in range(16):
        one = plan.anneal([seeds[s]], 2.0, 0.1)
        assert one.tobytes() == a[s:s + 1].tobytes(), s


# --------------------------------------------------------------------------
# 7. pending history patch
# --------------------------------------------------------------------------
def test_anneal_flushes_a_pending_history_patch():
    dom = _domain(spaces.many_dists_space(hp))
    docs = _docs(dom, 51, 9)
    L = np.random.RandomState(10).rand(51)
    for d, l in zip(docs, L):
        d['state'] = JOB_STATE_DONE
        d['result'] = {'status': 'ok', 'loss': float(l)}
    trials = Trials()
    trials.insert_trial_docs(docs[:50])
    trials.refresh()
    st = tpe._state(dom)
    hist = st.history(dom, trials).sync(trials)
    plan = st.plan_for(dom, 64, E.default_engine())
    plan.set_anneal_order([dom.space.by_label[lab].index for lab in dom.space.draw_order])
    hist.push(plan)
    plan.fit()
    trials.insert_trial_docs(docs[50:])
    trials.refresh()
    hist.sync(trials)
    assert hist.n == 51
    hist.push(plan)                     # one row: deferred, pending on the host
    seeds = tpe.batch_seeds(5, 33)
    got = plan.anneal(seeds, 2.0, 0.1)  # no fit in between
    _, losses, vals, active = hist.columns()
    fresh = _plan(dom, losses, vals, active, cap=64)
    want = fresh.anneal(seeds, 2.0, 0.1)
    assert got.tobytes() == want.tobytes()
    assert plan.anneal_trace(33)['row'].max() <= 50


# --------------------------------------------------------------------------
# 8. through the public interface
# --------------------------------------------------------------------------
def test_fmin_with_anneal_reaches_the_optimum():
    # Loss bar from the reference semantics, not from the device run: the host
    # 'numpy' path over rstate seeds 0..31 (80 evals each) has a worst
    # best-loss of 1.459e-3 (median 3.9e-5); a fixed-seed device run is one
    # more draw from that distribution and the loss is quadratic in the miss,
    # so the bar is 4 x 1.459e-3 = 5.84e-3.
    t = Trials()
    fmin(lambda x: (x - 3) ** 2, hp.uniform('x', -5, 5), algo=anneal.suggest, max_evals=80,
         trials=t, rstate=np.random.RandomState(4))
    assert len(t) == 80
    assert min(t.losses()) < 5.84e-3, min(t.losses())


def test_fmin_with_the_documented_mix_recipe():
    t = Trials()
    algo = functools.partial(mix.suggest, p_suggest=[
        (.1, rand.suggest), (.2, anneal.suggest), (.7, tpe.suggest)])
    space = spaces.cond_space(hp)
    fmin(lambda cfg: cfg['aa'], space, algo=algo, max_evals=60, trials=t,
         rstate=np.random.RandomState(2))
    assert len(t) == 60
    labels = Domain(lambda x: 0.0, space).space.labels
    for d in t.trials:
        v = d['misc']['vals']
        b = v['top'][0]
        assert isinstance(b, int) and len(v['aa']) == 1
        for lab in labels:
            assert d['misc']['idxs'][lab] == [d['tid']] * len(v[lab])
            if lab[:-1] in ('lr', 'units', 'act', 'zz'):
                assert (len(v[lab]) == 1) == (int(lab[-1]) == b)


def test_fmin_queue_of_eight_is_one_engine_call(monkeypatch):
    calls = []
    orig = E.Plan.anneal

    def counting(self, seeds, *a, **k):
        calls.append(len(seeds))
        return orig(self, seeds, *a, **k)
    monkeypatch.setattr(E.Plan, 'anneal', counting)
    t = Trials()
    fmin(lambda x: (x - 3) ** 2, hp.uniform('x', -5, 5), algo=anneal.suggest, max_evals=24,
         trials=t, rstate=np.random.RandomState(1), max_queue_len=8)
    assert len(t) == 24 and calls == [8, 8, 8]
    xs = [d['misc']['vals']['x'][0] for d in t.trials]
    assert len(set(xs)) == 24


def test_suggest_batch_on_the_device():
    dom, losses, vals, active = _history('cond', 7)
    idxs, vals_ = anneal.suggest_batch([0, 1, 2, 3], dom, Trials(), 3)
    assert idxs['top'] == [0, 1, 2, 3] and len(vals_['aa']) == 4
    for lab in dom.space.labels:
        assert len(idxs[lab]) == len(vals_[lab])
