"""Multivariate TPE with one joint model per group of hps on the GPU
(tpe_plan_group_*, ``multivariate='groups'``) against ``group_oracle``'s numpy
restatement of the model.

Tolerances: the project's 1e-6 bar (gpu_util.RTOL) on each side's
log-density, |d J| <= RTOL max(1, |J|); everything the engine defines in terms
of its own outputs -- which row owns which marginal component, joint_g as a
difference and the total as a float64 sum, the draws as tpe_sample's values,
and group 0 as the root model of ``multivariate=True`` -- is compared bit for
bit."""
import functools

import numpy as np
import pytest

import hyperopt_amd as H
from hyperopt_amd import fmin, hp, tpe, rand, Trials, trials_from_docs
from hyperopt_amd import _engine as E
from hyperopt_amd.base import Domain

from oracle import tpe_oracle as O
from golden_io import load, load_json
from gpu_util import RTOL
from oracle_algo import oracle_hps
import group_oracle as G
import joint_oracle as J
import spaces

pytestmark = pytest.mark.gpu

GAMMA, PRIOR_WEIGHT = 0.25, 1.0
JOINT_STREAM = 1 << 29
FIXTURES = {'cfg2': spaces.cfg2_space, 'cond': spaces.cond_space, 'cfg3_small': spaces.cfg3_space}
SHAPES = {'cfg2': (20, 1000), 'cond': (14, 120), 'cfg3_small': (50, 300), 'nested': (9, 80)}
NAMES = sorted(SHAPES)
NESTED_SEED = 7
# below rows of every group but the root's (the fixtures' edge: prior-only
# sides, K = 2 and K = 3)
BELOW_ROWS = {'cond': [2, 1, 0], 'cfg3_small': [0, 1, 1, 1, 2, 0, 0]}
TILE = 8      # components per block of the scoring tables
BOUNDED = ('uniform', 'quniform', 'qloguniform')


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b, msg=''):
    np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=msg)


def _same_bytes(a, b, msg=''):
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint8),
                                  np.ascontiguousarray(b).view(np.uint8), err_msg=msg)


def _done(docs, losses):
    for d, l in zip(docs, losses):
        d['state'] = H.JOB_STATE_DONE
        d['result'] = {'status': 'ok', 'loss': float(l)}
    return trials_from_docs(docs)


def _nested_trials():
    dom = Domain(lambda x: 0.0, G.nested_space(hp))
    docs = rand.suggest(list(range(80)), dom, Trials(), NESTED_SEED)
    return dom, _done(docs, np.random.RandomState(NESTED_SEED + 100).rand(80))


@functools.lru_cache(maxsize=None)
def _history(name):
    """(domain, losses, vals, active) of a named history."""
    if name in FIXTURES:
        meta = load_json('suggest_meta.json')[name]
        d = load('suggest_%s.npz' % name)
        dom = Domain(lambda x: 0.0, FIXTURES[name](hp))
        assert list(meta['labels']) == dom.space.labels
        out = dom, d['losses'], d['vals'], d['active']
    else:
        dom, trials = _nested_trials()
        _, losses, vals, active = tpe.build_history(dom, trials)
        out = dom, losses, vals, active
    assert out[2].shape == SHAPES[name]
    for a in out[1:]:
        a.setflags(write=False)
    return out


def _new_plan(name, n=None):
    dom, losses, vals, active = _history(name)
    n = losses.size if n is None else n
    hps, conds, pprior = dom.space.engine_tables()
    plan = E.Plan(E.default_engine(), hps, conds, pprior, max_trials=n)
    plan.set_history(np.ascontiguousarray(losses[:n]), np.ascontiguousarray(vals[:, :n]),
                     np.ascontiguousarray(active[:, :n]))
    plan.fit(gamma=GAMMA, prior_weight=PRIOR_WEIGHT)
    plan.group_fit()
    return plan


_plan = functools.lru_cache(maxsize=None)(_new_plan)


@functools.lru_cache(maxsize=None)
def _model(name, n=None):
    dom, losses, vals, active = _history(name)
    n = losses.size if n is None else n
    h = oracle_hps(dom.space)
    return G.GroupModel([(lab, h[lab]) for lab in dom.space.labels], losses[:n], vals[:, :n],
                        active[:, :n], GAMMA, PRIOR_WEIGHT)


@functools.lru_cache(maxsize=None)
def _scored(name):
    """The fixture's own rows as configurations: (total, active, joint[G, M],
    J_below[G, M], J_above[G, M]), computed once."""
    _, _, vals, _ = _history(name)
    plan = _plan(name)
    total, active, joint = plan.group_score_points(vals, want_active=True, want_joint=True)
    sides = [plan.group_sides(g, vals.shape[1]) for g in range(joint.shape[0])]
    out = (total, active, joint, np.stack([s[0] for s in sides]), np.stack([s[1] for s in sides]))
    for a in out:
        a.setflags(write=False)
    return out


# ------------------------------------------------------------ the partition
@pytest.mark.parametrize('name', NAMES)
def test_engine_groups_are_hp_groups(name):
    dom = _history(name)[0]
    cs = dom.space
    group_of, n_groups = _plan(name).group_info()
    groups = tpe.hp_groups(cs)
    assert n_groups == len(groups)
    want = np.empty(len(cs.labels), dtype=np.int32)
    for g, labs in enumerate(groups):
        want[[cs.labels.index(lab) for lab in labs]] = g
    np.testing.assert_array_equal(group_of, want)
    assert [[cs.labels[i] for i in g] for g in _model(name).groups] == [list(g) for g in groups]


def test_the_fixtures_sit_on_the_edge():
    """Prior-only sides (K = 1), K = 2 and K = 3 are all hit."""
    for name, want in BELOW_ROWS.items():
        assert [r[0].size for r in _model(name).rows[1:]] == want, name
    m = _model('nested')
    labels = _history('nested')[0].space.labels
    empty = [tuple(labels[i] for i in g) for g, r in zip(m.groups, m.rows) if r[0].size == 0]
    assert empty == [('p', 'q'), ('z',)]


# ------------------------------------------------------------------ the fit
def _check_fit(name, n=None):
    dom, losses, vals, _ = _history(name)
    plan, model = _plan(name, n), _model(name, n)
    tables = dom.space.engine_tables()[0]
    for g, hp_ids in enumerate(model.groups):
        for s in range(2):
            rows_want = np.concatenate([[-1], model.rows[g][s]])
            wj, _, _, rj = plan.group_mixture(g, -1, s)
            np.testing.assert_array_equal(rj, rows_want)
            np.testing.assert_allclose(wj, model.w[g][s], rtol=1e-14, atol=0)
            for d, i in zip(model.dims[g][s], hp_ids):
                w, mu, sg, rows = plan.group_mixture(g, i, s)
                msg = '%s n=%s group %d hp %d side %d' % (name, n, g, i, s)
                np.testing.assert_array_equal(rows, rows_want, err_msg=msg)
                if tables[i].family == E.CAT:
                    _same(w, wj, msg)
                    np.testing.assert_array_equal(
                        mu, np.concatenate([[-1.0], vals[i][model.rows[g][s]]]))
                    assert (np.abs(sg - d.a) <= 1e-12 * abs(d.a)).all(), msg
                    continue
                # sorted by (mu, row) the components are the marginal mixture, bit for bit
                order = np.lexsort((rows, mu))
                for got, want in zip((w, mu, sg), plan.mixture(i, s)):
                    _same(got[order], want, msg)
                np.testing.assert_allclose(mu[1:], d.obs, rtol=1e-14, atol=1e-14, err_msg=msg)
                np.testing.assert_array_equal(d.mu[0], mu[0])
    with pytest.raises(ValueError):     # an hp of another group
        plan.group_mixture(0, model.groups[-1][0] if len(model.groups) > 1 else plan.n_hp, 0)


@pytest.mark.parametrize('name', NAMES)
def test_fit_components_are_the_marginal_mixtures(name):
    _check_fit(name)


@functools.lru_cache(maxsize=None)
def _n_for_k_above(k):
    """(n, group): the shortest `cond` history in which a branch group's
    above side has k components."""
    for n in range(1, 121):
        for g, r in enumerate(_model('cond', n).rows):
            if g and r[1].size + 1 == k:
                return n, g
    raise AssertionError(k)


@pytest.mark.parametrize('k_above', [1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1])
def test_fit_at_the_component_tile_boundaries(k_above):
    n, g = _n_for_k_above(k_above)
    plan = _plan('cond', n)
    assert plan.group_mixture(g, -1, 1)[0].size == k_above
    _check_fit('cond', n)
    # and the scores of the fixture's rows at this size
    _, _, vals, _ = _history('cond')
    model = _model('cond', n)
    joint = plan.group_score_points(vals, want_joint=True)[1]
    _check_groups(plan, model, vals, joint, 'cond n=%d' % n)


def test_group_fit_needs_a_fit_and_a_later_fit_invalidates_it():
    dom, losses, vals, active = _history('cond')
    hps, conds, pprior = dom.space.engine_tables()
    plan = E.Plan(E.default_engine(), hps, conds, pprior, max_trials=losses.size)
    plan.set_history(losses, vals, active)
    assert plan.group_info()[1] == 4            # (needs no fit)
    with pytest.raises(ValueError):
        plan.group_fit()
    plan.fit(gamma=GAMMA, prior_weight=PRIOR_WEIGHT)
    with pytest.raises(ValueError):
        plan.group_score_points(vals)
    with pytest.raises(ValueError):
        plan.group_sample_points(1, 4)
    plan.group_fit()
    _same(plan.group_score_points(vals), _scored('cond')[0])
    assert np.isfinite(plan.group_sides(0, 4)[0]).all()
    plan.fit(gamma=GAMMA, prior_weight=PRIOR_WEIGHT)
    with pytest.raises(ValueError):
        plan.group_score_points(vals)
    with pytest.raises(ValueError):     # (the sides of the dropped model are not handed out)
        plan.group_sides(0, 4)


# ---------------------------------------------------------------- the score
def _check_groups(plan, model, cfg, joint, msg):
    """Per group both sides against the oracle where the group is active; NaN
    sides and a +0.0 joint where it is not; joint_g = J_b - J_a bit for bit."""
    on = model.active(cfg)
    want_b, want_a = model.sides(cfg)
    worst = 0.0
    for g in range(on.shape[0]):
        jb, ja = plan.group_sides(g, cfg.shape[1])
        sel = on[g]
        assert np.isnan(jb[~sel]).all() and np.isnan(ja[~sel]).all(), (msg, g)
        assert (_bits(joint[g][~sel]) == 0).all(), (msg, g)
        _same(joint[g][sel], (jb - ja)[sel], '%s group %d' % (msg, g))
        for got, want, side in ((jb, want_b[g], 'below'), (ja, want_a[g], 'above')):
            assert np.isfinite(want[sel]).all(), (msg, g, side)
            err = np.abs(got[sel] - want[sel])
            bound = RTOL * np.maximum(1.0, np.abs(want[sel]))
            if err.size:
                worst = max(worst, (err / bound).max())
            assert (err <= bound).all(), (msg, g, side, np.argwhere(~(err <= bound))[:5])
    print('%s: max |d J| / bound = %.3g' % (msg, worst))


@pytest.mark.parametrize('name', NAMES)
def test_fixture_rows_match_oracle(name):
    dom, _, vals, active = _history(name)
    plan, model = _plan(name), _model(name)
    total, act, joint, jb, ja = _scored(name)
    _check_groups(plan, model, vals, joint, name)
    _same(total, G.ordered_sum(joint), name)
    # activity: score_points', and the history's own
    _, mact = plan.score_points(vals, want_active=True)
    np.testing.assert_array_equal(act, mact)
    np.testing.assert_array_equal(act, active)
    on = model.active(vals)
    for g, hp_ids in enumerate(model.groups):
        np.testing.assert_array_equal(act[hp_ids] == 1, np.broadcast_to(on[g], (len(hp_ids),) + on[g].shape))
    if len(model.groups) > 1:
        assert (~on).any()              # (some group is inactive somewhere: the +0.0 path)
    # the outputs are optional
    _same(plan.group_score_points(vals), total)


@pytest.mark.parametrize('m', [1, 63, 64, 65, 257])
def test_launch_shape_does_not_change_a_configuration(m):
    _, _, vals, _ = _history('cfg3_small')
    plan = _plan('cfg3_small')
    total, act, joint, jb, ja = _scored('cfg3_small')
    pick = np.random.RandomState(m).permutation(300)[:m]
    sub = np.ascontiguousarray(vals[:, pick])
    got = plan.group_score_points(sub, want_active=True, want_joint=True)
    for g, w in zip(got, (total[pick], act[:, pick], joint[:, pick])):
        _same_bytes(g, w)
    Gn = joint.shape[0]
    for g in range(Gn):
        gb, ga = plan.group_sides(g, m)
        _same_bytes(gb, jb[g][pick])
        _same_bytes(ga, ja[g][pick])
    # device pointers, rows longer than m, sentinels behind them
    eng, P, ld = plan.engine, plan.n_hp, m + 9
    pad = np.full((P, ld), np.nan)
    pad[:, :m] = sub
    v = E.DeviceBuffer(eng, 8 * P * ld).upload(pad)
    tot = E.DeviceBuffer(eng, 8 * ld).upload(np.full(ld, -7.0))
    jnt = E.DeviceBuffer(eng, 8 * Gn * ld).upload(np.full((Gn, ld), -7.0))
    ac = E.DeviceBuffer(eng, P * ld).upload(np.full((P, ld), 9, dtype=np.uint8))
    plan.group_score_points_device(v.ptr, m, ld, tot.ptr, jnt.ptr, ac.ptr)
    eng.synchronize()
    dt, dj = tot.download(np.empty(ld)), jnt.download(np.empty((Gn, ld)))
    da = ac.download(np.empty((P, ld), dtype=np.uint8))
    assert (dt[m:] == -7.0).all() and (dj[:, m:] == -7.0).all() and (da[:, m:] == 9).all()
    _same(dt[:m], got[0])
    _same(dj[:, :m], got[2])
    np.testing.assert_array_equal(da[:, :m], got[1])
    # without the optional outputs
    tot.upload(np.full(ld, -7.0))
    plan.group_score_points_device(v.ptr, m, ld, tot.ptr)
    eng.synchronize()
    _same(tot.download(np.empty(ld))[:m], got[0])


# ------------------------------------------------------------ the identities
def _joint_plan(name):
    """A plan of the same history with the root model of multivariate=True."""
    dom, losses, vals, active = _history(name)
    hps, conds, pprior = dom.space.engine_tables()
    plan = E.Plan(E.default_engine(), hps, conds, pprior, max_trials=losses.size)
    plan.set_history(losses, vals, active)
    plan.fit(gamma=GAMMA, prior_weight=PRIOR_WEIGHT)
    plan.joint_fit()
    return plan


def test_without_conditions_groups_is_the_root_model():
    _, _, vals, _ = _history('cfg2')
    gp, jp = _plan('cfg2'), _joint_plan('cfg2')
    total, act, joint, jb, ja = _scored('cfg2')
    jt, jact, jj = jp.joint_score_points(vals, want_active=True, want_joint=True)
    assert joint.shape[0] == 1
    _same(total, jt)
    _same(joint[0], jj)
    np.testing.assert_array_equal(act, jact)
    for got, want in zip((jb[0], ja[0]), jp.joint_sides(vals.shape[1])):
        _same(got, want)
    gv, gt, gj, gc = gp.group_sample_points(6, 300, begin=1, want_joint=True, want_comp=True)
    jv, jt, jj, jc = jp.joint_sample_points(6, 300, begin=1, want_joint=True, want_comp=True)
    _same(gv, jv)
    _same(gt, jt)
    _same(gj[0], jj)
    np.testing.assert_array_equal(gc[0], jc)


def test_group_0_is_the_root_model():
    dom, _, vals, _ = _history('cond')
    roots = tpe.root_indices(dom.space)
    gp, jp = _plan('cond'), _joint_plan('cond')
    _same(_scored('cond')[2][0], jp.joint_score_points(vals, want_joint=True)[1])
    gv, gt, gc = gp.group_sample_points(8, 300, begin=5, want_comp=True)
    jv, jt, jc = jp.joint_sample_points(8, 300, begin=5, want_comp=True)
    _same(gv[roots], jv[roots])
    np.testing.assert_array_equal(gc[0], jc)


@pytest.mark.parametrize('label', ['r', 'v', 'z', 'shared'])
def test_a_one_hp_group_is_the_marginal_term(label):
    """The host test's identity against score_points' term of the hp, within
    the bound of the two lpdfs of a term (test_gpu_joint.py)."""
    dom, losses, vals, active = _history('nested')
    plan, model = _plan('nested'), _model('nested')
    i = dom.space.labels.index(label)
    g = model.group_of[i]
    assert model.groups[g] == [i]
    h = oracle_hps(dom.space)[label]
    on = active[i] == 1
    assert on.sum() >= 5
    joint = _scored('nested')[2][g]
    term = plan.score_points(vals, want_terms=True)[1][i]
    tids = np.arange(losses.size)
    bo, ao = O.split_observations(tids[on], vals[i][on], tids, losses, GAMMA, kind='stable')
    with np.errstate(all='ignore'):
        r = O.score_hp(h['dist'], h['args'], bo, ao, PRIOR_WEIGHT, vals[i][on], kind='stable')
        const = 0.0
        if h['dist'] in BOUNDED:
            # the two truncation masses the joint kernels leave out
            fk, pm, ps, low, high, q, tr = O.posterior_spec(h['dist'], h['args'], PRIOR_WEIGHT)
            pacc = [O._truncation_mass(*r[k], low, high) for k in ('below', 'above')]
            const = np.log(pacc[0]) - np.log(pacc[1])
    bound = RTOL * (np.maximum(1.0, np.abs(r['llik_b'])) + np.maximum(1.0, np.abs(r['llik_a'])))
    err = np.abs(joint[on] - const - term[on])
    print('%s: max |joint - term| / bound = %.3g (constant %.3g)' % (label, (err / bound).max(),
                                                                     const))
    assert np.isfinite(joint[on]).all() and (err <= bound).all()
    assert (_bits(joint[~on]) == 0).all()


def test_bad_values_in_a_branch():
    dom, _, vals, active = _history('cond')
    cs = dom.space
    plan = _plan('cond')
    top, act0, lr0 = (cs.labels.index(l) for l in ('top', 'act0', 'lr0'))
    cols = np.flatnonzero(vals[top] == 0)[:4]
    cfg = np.array(vals[:, cols])
    cfg[act0, 0] = 1.5          # not an option index
    cfg[lr0, 1] = np.nan
    cfg[act0, 2] = 3.0          # upper
    total, act, joint = plan.group_score_points(cfg, want_active=True, want_joint=True)
    ref_total, ref_act, ref_joint = (a[..., cols] for a in _scored('cond')[:3])
    assert np.isnan(joint[1][:3]).all() and np.isnan(total[:3]).all()
    _same(joint[[0, 2, 3]], ref_joint[[0, 2, 3]])      # the other groups keep their bits
    _same(joint[:, 3], ref_joint[:, 3])
    _same(total[3], ref_total[3])
    np.testing.assert_array_equal(act, ref_act)         # (act0 has no child: routing unchanged)
    # a bad value of a choice with children activates none of them
    dn, _, nvals, _ = _history('nested')
    labs = dn.space.labels
    inner = labs.index('inner')
    ncols = np.flatnonzero(_history('nested')[3][inner] == 1)[:3]
    ncfg = np.array(nvals[:, ncols])
    ncfg[inner, 0] = 0.5
    ncfg[inner, 1] = np.nan
    np_ = _plan('nested')
    ntotal, nact, njoint = np_.group_score_points(ncfg, want_active=True, want_joint=True)
    kids = [labs.index(l) for l in ('p', 'q', 'r')]
    assert (nact[kids][:, :2] == 0).all() and nact[kids][:, 2].sum() >= 1
    g_inner = _model('nested').group_of[inner]
    assert np.isnan(njoint[g_inner][:2]).all() and np.isnan(ntotal[:2]).all()
    assert (_bits(njoint[[2, 3]][:, :2]) == 0).all()    # {p, q} and {r}: inactive, +0.0
    _same(ntotal[2], _scored('nested')[0][ncols[2]])


# ----------------------------------------------------------------- the draw
DRAW = {'cfg2': (6, 1), 'cond': (8, 5), 'cfg3_small': (9, (1 << 32) + 3), 'nested': (12, 2)}


def _sample_args(t):
    return (t.low if t.flags & E.HAS_LOW else None, t.high if t.flags & E.HAS_HIGH else None,
            t.q if t.flags & E.HAS_Q else None)


@pytest.mark.parametrize('name', sorted(DRAW))
def test_draws_are_tpe_samples_of_the_groups_components(name):
    dom, _, _, _ = _history(name)
    cs = dom.space
    plan, model = _plan(name), _model(name)
    eng = plan.engine
    seed, begin = DRAW[name]
    m, P = 257, plan.n_hp
    vals, total, active, joint, comp = plan.group_sample_points(
        seed, m, begin=begin, want_active=True, want_joint=True, want_comp=True)
    tables, _, pprior = cs.engine_tables()
    # a child is drawn only under its parent's drawn branch; inactive hps are NaN
    on = tpe.active_columns(cs, vals)
    np.testing.assert_array_equal(active == 1, on)
    np.testing.assert_array_equal(np.isnan(vals), ~on)
    for g, hp_ids in enumerate(model.groups):
        sel_g = on[hp_ids[0]]
        assert (on[hp_ids] == sel_g).all()
        # 1. the group's component: one categorical draw over its below weights
        wb = plan.group_mixture(g, -1, 0)[0]
        pick = eng.sample(E.CAT, wb, seed=seed, stream=JOINT_STREAM | (P + g), offset=begin, n=m)
        np.testing.assert_array_equal(comp[g], np.where(sel_g, pick, -1).astype(np.int32))
        # 2. every value of the group: tpe_sample of that component's kernel alone
        for i in hp_ids:
            t = tables[i]
            w, mu, sg, rows = plan.group_mixture(g, i, 0)
            want = np.full(m, np.nan)
            for k in np.unique(comp[g][sel_g]):
                sel = comp[g] == k
                if t.family == E.CAT:
                    pi = (np.asarray(pprior[t.pprior_begin:t.pprior_begin + t.upper])
                          if t.flags & E.PCHOICE else np.full(t.upper, 1.0 / t.upper))
                    kap = pi if k == 0 else J.kappa([int(mu[k])], sg[k], pi)[1]
                    s = eng.sample(E.CAT, kap, seed=seed, stream=JOINT_STREAM | i, offset=begin,
                                   n=m)
                else:
                    s = eng.sample(t.family, [1.0], [mu[k]], [sg[k]], *_sample_args(t), seed=seed,
                                   stream=JOINT_STREAM | i, offset=begin, n=m)
                want[sel] = s[sel]
            _same(vals[i], want, '%s hp %d' % (name, i))
    assert np.unique(comp[0]).size > 1
    # 3. the scores are group_score_points' of the drawn array
    want = plan.group_score_points(np.ascontiguousarray(vals), want_active=True, want_joint=True)
    for got, w_ in zip((total, active, joint), want):
        _same_bytes(got, w_)
    assert np.isfinite(total).all()
    # 4. a range split into two calls is one call
    parts = [plan.group_sample_points(seed, n_, begin=begin + b_, want_comp=True)
             for b_, n_ in ((0, 100), (100, 157))]
    _same(np.concatenate([p[0] for p in parts], axis=1), vals)
    _same(np.concatenate([p[1] for p in parts]), total)
    np.testing.assert_array_equal(np.concatenate([p[2] for p in parts], axis=1), comp)


def test_device_draw_equals_host_draw():
    plan = _plan('cond')
    eng, P, m, ld, Gn = plan.engine, plan.n_hp, 65, 70, 4
    host = plan.group_sample_points(8, m, begin=5, want_active=True, want_joint=True,
                                    want_comp=True)
    v = E.DeviceBuffer(eng, 8 * P * ld).upload(np.full((P, ld), -7.0))
    tot = E.DeviceBuffer(eng, 8 * ld).upload(np.full(ld, -7.0))
    jnt = E.DeviceBuffer(eng, 8 * Gn * ld).upload(np.full((Gn, ld), -7.0))
    cmp_ = E.DeviceBuffer(eng, 4 * Gn * ld).upload(np.full((Gn, ld), -7, dtype=np.int32))
    ac = E.DeviceBuffer(eng, P * ld).upload(np.full((P, ld), 9, dtype=np.uint8))
    plan.group_sample_points_device(8, 5, m, ld, v.ptr, tot.ptr, cmp_.ptr, jnt.ptr, ac.ptr)
    eng.synchronize()
    dv, dt = v.download(np.empty((P, ld))), tot.download(np.empty(ld))
    dj, dc = jnt.download(np.empty((Gn, ld))), cmp_.download(np.empty((Gn, ld), dtype=np.int32))
    da = ac.download(np.empty((P, ld), dtype=np.uint8))
    assert (dv[:, m:] == -7.0).all() and (dt[m:] == -7.0).all() and (dc[:, m:] == -7).all()
    assert (dj[:, m:] == -7.0).all() and (da[:, m:] == 9).all()
    _same(dv[:, :m], host[0])
    _same(dt[:m], host[1])
    np.testing.assert_array_equal(da[:, :m], host[2])
    _same(dj[:, :m], host[3])
    np.testing.assert_array_equal(dc[:, :m], host[4])
    # without the optional outputs
    plan.group_sample_points_device(8, 5, m, ld, v.ptr, tot.ptr)
    eng.synchronize()
    _same(v.download(np.empty((P, ld)))[:, :m], host[0])
    _same(tot.download(np.empty(ld))[:m], host[1])


# --------------------------------------------------------- the entry points
def _fixture_trials(name):
    meta = load_json('suggest_meta.json')[name]
    dom = Domain(lambda x: 0.0, FIXTURES[name](hp))
    docs = rand.suggest(list(range(meta['n'])), dom, Trials(), meta['hist_seed'])
    return dom, _done(docs, _history(name)[1])


def _values(docs):
    return [{lab: v[0] for lab, v in d['misc']['vals'].items() if v} for d in docs]


def test_entry_points_are_the_plan_calls():
    dom, trials = _fixture_trials('cond')
    cs = dom.space
    _, _, vals, active = _history('cond')
    ei, terms, act, joint = tpe.score_configs(np.where(active == 1, vals, np.nan), dom, trials,
                                              return_terms=True, multivariate='groups')
    total, a_, j_, _, _ = _scored('cond')
    _same(ei, total)
    _same(joint, j_)
    assert joint.shape[0] == len(tpe.hp_groups(cs))
    for i, lab in enumerate(cs.labels):
        assert (_bits(terms[lab]) == 0).all()
        np.testing.assert_array_equal(act[lab], a_[i] == 1)
    drawn, dei = tpe.sample_configs(200, dom, trials, 5, begin=3, multivariate='groups')
    ref = _plan('cond').group_sample_points(tpe.batch_seeds(5, 1)[0], 200, begin=3)
    _same(drawn, ref[0])
    _same(dei, ref[1])
    _same(dei, tpe.score_configs(drawn, dom, trials, multivariate='groups'))
    # the other two modes are untouched
    _same(tpe.sample_configs(200, dom, trials, 5, begin=3)[0],
          _plan('cond').sample_points(tpe.batch_seeds(5, 1)[0], 200, begin=3)[0])
    _same(tpe.sample_configs(200, dom, trials, 5, begin=3, multivariate=True)[0],
          _joint_plan('cond').joint_sample_points(tpe.batch_seeds(5, 1)[0], 200, begin=3)[0])
    with pytest.raises(ValueError):
        tpe.sample_configs(200, dom, trials, 5, multivariate='group')


def test_suggest_joint_groups_picks_follow_the_rule():
    dom, trials = _fixture_trials('cond')
    cs = dom.space
    n, ids = 1000, [120, 121, 122]
    vals, ei = tpe.sample_configs(n, dom, trials, 21, multivariate='groups')
    _, _, hv, ha = tpe.build_history(dom, trials)
    want = tpe.joint_select(ei, None, vals, hv, ha, 3)
    docs = tpe.suggest_joint(ids, dom, trials, 21, n_configs=n, n_startup_jobs=0,
                             multivariate='groups')
    assert [d['tid'] for d in docs] == ids
    assert _values(docs) == tpe.columns_to_configs(cs, vals[:, want], ~np.isnan(vals[:, want]))
    # a pool ranked by the group models, on the device-resident path
    pool = np.ascontiguousarray(vals[:, :300])
    docs = tpe.suggest_from_pool(ids, dom, trials, 1, pool=pool, n_startup_jobs=0,
                                 multivariate='groups')
    top = tpe.rank_pool(ei[:300], np.ones(300, dtype=bool), 3)
    assert _values(docs) == tpe.columns_to_configs(cs, pool[:, top], ~np.isnan(pool[:, top]))


def test_fmin_groups():
    def loss(c):
        b = c['top']
        k = b['kind']
        return float((np.log(b['lr%d' % k]) + 3) ** 2 + 0.1 * b['zz%d' % k] ** 2 + c['aa'] + k)

    t = Trials()
    algo = functools.partial(tpe.suggest_joint, n_configs=512, n_startup_jobs=10,
                             multivariate='groups')
    best = fmin(loss, spaces.cond_space(hp), algo=algo, max_evals=30, trials=t,
                rstate=np.random.RandomState(3))
    assert len(t) == 30 and np.isfinite(min(t.losses()))
    # the returned configuration is consistent with its own choices
    b = best['top']
    assert set(best) == {'aa', 'top', 'lr%d' % b, 'units%d' % b, 'act%d' % b, 'zz%d' % b}
