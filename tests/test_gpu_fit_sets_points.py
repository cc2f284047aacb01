"""The whole-configuration models away from the default fit (DESIGN 5.12 -
5.16): every named set of ``fit_set_cases`` (gamma, gamma_cap, prior_weight,
lf) on its 3000-trial history -- the large tier of k_fit under the joint and
the group fit -- over its 257 configurations.

What the sets reach (K = components of the below side: root group / branch 1 /
branch 0; above likewise):
    default      15 / 10 / 6        above 2987 / 1526 / 1462   the anchor
    wide-below   84 / 46 / 39             2918 / 1490 / 1429   more than a wave
    huge-below   1301 / 667 / 635         1701 / 869 / 833     scans > 4 a thread
    over-cap     2101 / 1069 / 1033       901 / 467 / 435      roots by rejection
    few-below    3 / 2 / 2                2999 / 1534 / 1466
    prior-only   1 / 1 / 1                3001 / 1535 / 1467
    pw-zero, pw-small, pw-big   the default split, prior_weight 0, 1e-3, 50
    lf-short, lf-off            wide-below's split, prior_weight 0.5, lf 20, 0

Per set: the joint and the group fit's components against the oracle's rows,
weights and places in the marginal mixtures (the check that a tie order of the
large tier's sort other than the row's cannot pass: test_fit_sets_points_host.py);
the three score calls against the oracles at test_gpu_joint / _group /
_points' tolerances, entries that are not finite by class; the draws bit for
bit tpe_sample's and within draw_replay's bars of the host replay; the
component picks against a host pick of the oracle's weights; over-cap's
refusal by the joint and the group draw; the pending batch against
batch_oracle; two host entry points.  No tolerance is new except the one on a
continuous component's weight, derived where it is used.

Measured on an MI355X: the 97 cases take 7.2 s (the slowest 0.5 s), and no
set found a fault in the engine.  The 257 joint draws of huge-below pick a
component >= 256 in 244 draws and >= 1024 in 96 (the group draw's root group
the same; its branches >= 256 in 111 and 107); no other set has a below
component past 84.  The largest error over its bound: 0.068 on a marginal
term, 0.058 on a side of the joint model, 0.144 on a side of a group, 0.013 on
a round's score of the pending batch.  What the sets did find is in the
oracle: ``joint_oracle.side_weights`` read lf = 0 as a ramp over the whole
side where the engine, like ``parzen_fit`` (``if lf and lf < n``), reads it as
no forgetting (k_joint_rows: ``lfw = A.lf && A.lf < ns``); it was corrected,
and lf-off's component weights are checked against the corrected one.
"""
import functools

import numpy as np
import pytest

from hyperopt_amd import tpe
from hyperopt_amd import _engine as E

from oracle import tpe_oracle as O
from gpu_util import RTOL
import batch_oracle as B
import draw_replay as R
import fit_set_cases as C
import group_oracle as G
import joint_oracle as J
from test_gpu_batch import _check_identities
from test_gpu_joint import JOINT_STREAM, _bits, _check_total, _same, _sample_args
from test_gpu_points import _check_total_is_the_sum, _term_bound

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
SEED = 0x51ED270B1F2E3D4C          # a Philox key with a nonzero high word
BEGIN = {name: 7 for name in C.NAMES}
BEGIN['huge-below'] = (1 << 32) + 3
DRAW_SETS = tuple(n for n in C.NAMES if n != 'over-cap')
SIZES = (1, 64, 65)
# two normalisers of at most N + 1 positive terms, each summed in an order of
# its own: a relative (N + 1) 2^-53 apiece
W_RTOL = 2 * (C.N + 1) * 2.0 ** -53


def _same_bytes(a, b, msg=''):
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint8),
                                  np.ascontiguousarray(b).view(np.uint8), err_msg=msg)


def _tables():
    return C.history()[0].space.engine_tables()


def _new_plan(name=None, n=C.N, **fit):
    dom, losses, vals, active = C.history()
    hps, conds, pprior = _tables()
    plan = E.Plan(E.default_engine(), hps, conds, pprior, max_trials=n)
    plan.set_history(np.ascontiguousarray(losses[:n]), np.ascontiguousarray(vals[:, :n]),
                     np.ascontiguousarray(active[:, :n]))
    plan.fit(**(C.fit_kwargs(name) if name else fit))
    return plan


@functools.lru_cache(maxsize=None)
def _joint_plan(name):
    plan = _new_plan(name)
    plan.joint_fit()
    return plan


@functools.lru_cache(maxsize=None)
def _group_plan(name):
    plan = _new_plan(name)
    plan.group_fit()
    return plan


def _cfg():
    return np.ascontiguousarray(C.configs()[0])


def test_the_cases_are_the_stated_ones():
    C.assert_sets_reach()
    over = _joint_plan('over-cap')
    for i, lab in enumerate(C.labels()):
        K = over.mixture(i, 0)[0].size
        assert (K > R.TAB_CAP) == (lab in C.ROOTS and _tables()[0][i].family != E.CAT), lab
    assert R.TAB_CAP == C.TAB_CAP


# ------------------------------------------------------------------ the fit
def _check_components(plan, get, dims, hp_ids, w_model, rows_model, msg):
    """One model (the joint one, or a group of the group one): per side the
    component weights, the rows, and per hp the components."""
    _, _, hv, _ = C.history()
    tables = _tables()[0]
    for s in range(2):
        rows_want = np.concatenate([[-1], rows_model[s]])
        wj, _, _, rj = get(-1, s)
        np.testing.assert_array_equal(rj, rows_want, err_msg=msg)
        np.testing.assert_allclose(wj, w_model[s], rtol=1e-14, atol=0, err_msg=msg)
        for d, i in zip(dims[s], hp_ids):
            w, mu, sg, rows = get(i, s)
            m = '%s hp %d side %d' % (msg, i, s)
            np.testing.assert_array_equal(rows, rows_want, err_msg=m)
            if tables[i].family == E.CAT:
                _same(w, wj, m)
                np.testing.assert_array_equal(mu, np.concatenate([[-1.0], hv[i][rows_model[s]]]))
                assert (np.abs(sg - d.a) <= 1e-12 * abs(d.a)).all(), m
                continue
            # component k is the marginal mixture's entry at the oracle's place of
            # row k, bit for bit ...
            mix = plan.mixture(i, s)
            for got, want in zip((w, mu, sg), mix):
                _same(got, want[d.place], m)
            order = np.lexsort((rows, mu))
            for got, want in zip((w, mu, sg), mix):
                _same(got[order], want, m)
            # ... that entry carries the row's own weight (tied rows differ in
            # it wherever the ramp is on: a sort that ordered them otherwise
            # would hand row k another row's) ...
            np.testing.assert_allclose(w, w_model[s], rtol=W_RTOL, atol=0, err_msg=m)
            # ... and the row's transformed observation
            np.testing.assert_allclose(mu[1:], d.obs, rtol=1e-14, atol=1e-14, err_msg=m)
            np.testing.assert_array_equal(d.mu[0], mu[0])


@pytest.mark.parametrize('name', C.NAMES)
def test_joint_fit_components(name):
    plan, model = _joint_plan(name), C.joint_model(name)
    assert plan.joint_mixture(-1, 0)[0].size == C.N_BELOW[name] + 1
    _check_components(plan, plan.joint_mixture, model.dims, model.roots, model.w, model.rows,
                      name)


@pytest.mark.parametrize('name', C.NAMES)
def test_group_fit_components(name):
    plan, model = _group_plan(name), C.group_model(name)
    group_of, n_groups = plan.group_info()
    assert n_groups == 3 == len(model.groups)
    for g, hp_ids in enumerate(model.groups):
        assert (group_of[hp_ids] == g).all()
        _check_components(plan, functools.partial(plan.group_mixture, g), model.dims[g], hp_ids,
                          model.w[g], model.rows[g], '%s group %d' % (name, g))


# ---------------------------------------------------------------- the score
def _check_values(got, want, bound, msg):
    """Entries that are not finite by class (NaN, +inf, -inf), the others
    within ``bound``; returns the largest error over its bound."""
    got, want = np.asarray(got), np.asarray(want)
    np.testing.assert_array_equal(C.klass(got), C.klass(want), err_msg=msg)
    fin = C.klass(want) == 0
    err = np.abs(got[fin] - want[fin])
    b = np.broadcast_to(bound, want.shape)[fin]
    assert (err <= b).all(), (msg, np.argwhere(~(err <= b))[:5])
    return float((err / b).max()) if err.size else 0.0


def _side_bound(want):
    with np.errstate(all='ignore'):
        return RTOL * np.maximum(1.0, np.abs(np.where(np.isfinite(want), want, 0.0)))


@functools.lru_cache(maxsize=None)
def _lliks(name):
    cfg, act, _ = C.configs()
    return C.marginal_lliks(name, cfg, act)


def _check_terms(terms, name, hp_ids, msg):
    """score_points' terms of the hps ``hp_ids`` against the oracle's lliks."""
    _, act, _ = C.configs()
    lb, la = _lliks(name)
    with np.errstate(all='ignore'):
        want = np.where(act == 1, lb - la, 0.0)
    bound = np.where(act == 1, _term_bound(lb, la, act), 1.0)
    assert (_bits(terms)[act == 0] == 0).all(), msg
    return _check_values(terms[hp_ids], want[hp_ids], bound[hp_ids], msg)


@pytest.mark.parametrize('name', C.NAMES)
def test_marginal_scores(name):
    cfg, act, _ = C.configs()
    plan = _joint_plan(name)
    total, terms, active = plan.score_points(_cfg(), want_terms=True, want_active=True)
    np.testing.assert_array_equal(active, act)
    worst = _check_terms(terms, name, list(range(10)), name)
    _check_total_is_the_sum(total, terms, name)
    lb, la = _lliks(name)
    want = C.marginal_total(lb, la, act)
    _check_values(total, want, _term_bound(lb, la, act).sum(axis=0), name)
    print('%s: max |d term| / bound = %.3g' % (name, worst))
    _same(plan.score_points(_cfg()), total)
    for m in SIZES:
        got = plan.score_points(np.ascontiguousarray(cfg[:, :m]), want_terms=True, want_active=True)
        for g, w in zip(got, (total[:m], terms[:, :m], active[:, :m])):
            _same_bytes(g, w, '%s m=%d' % (name, m))


@pytest.mark.parametrize('name', C.NAMES)
def test_joint_scores(name):
    cfg, act, _ = C.configs()
    plan, model = _joint_plan(name), C.joint_model(name)
    total, terms, active, joint = plan.joint_score_points(_cfg(), want_terms=True,
                                                          want_active=True, want_joint=True)
    jb, ja = plan.joint_sides(C.M)
    worst = 0.0
    for got, want, side in zip((jb, ja), model.sides(cfg), ('below', 'above')):
        worst = max(worst, _check_values(got, want, _side_bound(want), '%s J_%s' % (name, side)))
    print('%s: max |d J| / bound = %.3g' % (name, worst))
    with np.errstate(all='ignore'):
        _same(joint, jb - ja, name)
    _check_total(total, joint, terms, name)
    np.testing.assert_array_equal(active, act)
    cond = [i for i in range(10) if i not in model.roots]
    _check_terms(terms, name, cond, name)
    _same(terms[cond], plan.score_points(_cfg(), want_terms=True)[1][cond], name)
    assert (_bits(terms[model.roots]) == 0).all()
    for m in SIZES:
        got = plan.joint_score_points(np.ascontiguousarray(cfg[:, :m]), want_terms=True,
                                      want_active=True, want_joint=True) + plan.joint_sides(m)
        for g, w in zip(got, (total[:m], terms[:, :m], active[:, :m], joint[:m], jb[:m], ja[:m])):
            _same_bytes(g, w, '%s m=%d' % (name, m))


def _group_sides(plan, m):
    sides = [plan.group_sides(g, m) for g in range(3)]
    return np.stack([s[0] for s in sides]), np.stack([s[1] for s in sides])


@pytest.mark.parametrize('name', C.NAMES)
def test_group_scores(name):
    cfg, act, _ = C.configs()
    plan, model = _group_plan(name), C.group_model(name)
    total, active, joint = plan.group_score_points(_cfg(), want_active=True, want_joint=True)
    jb, ja = _group_sides(plan, C.M)
    on = model.active(cfg)
    want_b, want_a = B.sides(model, cfg)
    worst = 0.0
    for g in range(3):
        sel = on[g]
        assert np.isnan(jb[g][~sel]).all() and np.isnan(ja[g][~sel]).all(), (name, g)
        assert (_bits(joint[g][~sel]) == 0).all(), (name, g)
        with np.errstate(all='ignore'):
            _same(joint[g][sel], (jb[g] - ja[g])[sel], '%s group %d' % (name, g))
        for got, want, side in ((jb[g], want_b[g], 'below'), (ja[g], want_a[g], 'above')):
            worst = max(worst, _check_values(got[sel], want[sel], _side_bound(want[sel]),
                                             '%s group %d J_%s' % (name, g, side)))
    print('%s: max |d J| / bound = %.3g' % (name, worst))
    _same(total, G.ordered_sum(joint), name)
    np.testing.assert_array_equal(C.klass(total), C.klass(model.total(cfg)), err_msg=name)
    np.testing.assert_array_equal(active, act)
    for m in SIZES:
        got = plan.group_score_points(np.ascontiguousarray(cfg[:, :m]), want_active=True,
                                      want_joint=True) + _group_sides(plan, m)
        for g, w in zip(got, (total[:m], active[:, :m], joint[:, :m], jb[:, :m], ja[:, :m])):
            _same_bytes(g, w, '%s m=%d' % (name, m))


def test_a_configuration_no_below_row_supports():
    """prior_weight = 0: the prior's component and every miss of a categorical
    kernel weigh log(0).  The randint option no below row holds has no finite
    term under the joint and the group model -- NaN -- and probability 0
    under the marginal one: -inf."""
    cfg, _, what = C.configs()
    unseen, both = C.unseen_randint_options('pw-zero')
    j, k = what.index('ri=%d' % unseen[0]), what.index('ri=%d' % both[0])
    sub = np.ascontiguousarray(cfg[:, [j, k]])
    ri = C.labels().index('ri')
    jp, gp = _joint_plan('pw-zero'), _group_plan('pw-zero')
    total, joint = jp.joint_score_points(sub, want_joint=True)
    assert np.isnan(joint[0]) and np.isnan(total[0]) and np.isnan(jp.joint_sides(2)[0][0])
    assert np.isfinite(jp.joint_sides(2)[1]).all()
    gt, gj = gp.group_score_points(sub, want_joint=True)
    assert np.isnan(gj[0][0]) and np.isnan(gt[0])
    mt, terms = jp.score_points(sub, want_terms=True)
    assert terms[ri][0] == -np.inf and mt[0] == -np.inf and np.isfinite(terms[ri][1])
    # the same configurations under the default fit are finite throughout
    assert np.isfinite(_joint_plan('default').joint_score_points(sub)).all()
    assert np.isfinite(_group_plan('default').group_score_points(sub)).all()


# ----------------------------------------------------------------- the draw
def _check_replay(t, x, r, msg):
    """test_gpu_draw_replay's bars on the draws x against their replay r."""
    fam, (low, high, q) = t.family, _sample_args(t)
    deep = r['deep']
    assert np.isfinite(x).all() and not r['ambiguous_pick'].any(), msg
    if fam == E.CAT:
        np.testing.assert_array_equal(x, r['k'], err_msg=msg)
    elif q is not None:
        vs = np.exp(r['x']) if fam == R.LGMM else r['x']
        lo_n, hi_n = np.floor(vs / q) * q, np.ceil(vs / q) * q
        ok = (x == r['value']) | (r['ambiguous_round'] & ((x == lo_n) | (x == hi_n)))
        assert (ok | deep).all(), (msg, np.flatnonzero(~(ok | deep))[:5])
    else:
        xd = np.log(x) if fam == R.LGMM else x
        tol = r['tol']
        if fam == R.LGMM:
            tol = tol + 4.0 * EPS + np.spacing(np.abs(r['x']))
        ok = (np.abs(xd - r['x']) <= tol) | deep
        assert ok.all(), (msg, np.flatnonzero(~ok)[:5])


def _mixture_args(plan, t, i):
    w, mu, sg = plan.mixture(i, 0)
    cat = t.family == E.CAT
    return (w, None if cat else mu, None if cat else sg) + _sample_args(t)


@pytest.mark.parametrize('name', C.NAMES)
def test_marginal_draws(name):
    """Every set: the rejection sampler for over-cap's continuous roots, the
    tables for everything else."""
    assert (R.GMM, R.LGMM, R.CAT) == (E.GMM, E.LGMM, E.CAT)
    cs = C.history()[0].space
    plan = _joint_plan(name)
    eng, begin = plan.engine, BEGIN[name]
    vals, total, terms, active = plan.sample_points(SEED, C.M, begin=begin, want_terms=True,
                                                    want_active=True)
    on = active == 1
    np.testing.assert_array_equal(on, tpe.active_columns(cs, vals))
    assert np.isnan(vals[~on]).all() and not np.isnan(vals[on]).any()
    for i, t in enumerate(_tables()[0]):
        args = _mixture_args(plan, t, i)
        if name == 'over-cap':
            assert (args[0].size > R.TAB_CAP) == (C.labels()[i] in C.ROOTS and t.family != E.CAT)
        ref = eng.sample(t.family, *args, seed=SEED, stream=i, offset=begin, n=C.M)
        _same(vals[i][on[i]], ref[on[i]], '%s hp %d' % (name, i))
        rep = R.replay(t.family, *args, SEED, i, begin, C.M)
        if name == 'over-cap' and args[0].size > R.TAB_CAP:
            assert not rep['table'].any()
        sel = on[i]
        _check_replay(t, vals[i][sel], {k: v[sel] for k, v in rep.items()},
                      '%s hp %d' % (name, i))
    want = plan.score_points(np.ascontiguousarray(vals), want_terms=True, want_active=True)
    for g, w in zip((total, terms, active), want):
        _same_bytes(g, w, name)


def _check_pick(comp, w_oracle, stream, begin, sel, msg):
    """comp against the host pick of the oracle's weights at the replayed
    uniform; a neighbour only where the uniform is within PICK_RTOL of a step."""
    rep = R.replay(R.CAT, w_oracle, None, None, None, None, None, SEED, stream, begin, C.M)
    k, amb = rep['k'][sel], rep['ambiguous_pick'][sel]
    ok = (comp[sel] == k) | (amb & (np.abs(comp[sel] - k) == 1))
    assert ok.all(), (msg, np.flatnonzero(~ok)[:5])


def _check_component_draws(plan, get, hp_ids, comp, sel, vals, begin, msg):
    """Every value of the hps ``hp_ids`` where ``sel``: tpe_sample of the
    picked component's kernel alone (test_gpu_joint's criterion)."""
    eng = plan.engine
    tables, _, pprior = _tables()
    for i in hp_ids:
        t = tables[i]
        w, mu, sg, rows = get(i, 0)
        want = np.full(C.M, np.nan)
        for k in np.unique(comp[sel]):
            at = sel & (comp == k)
            if t.family == E.CAT:
                pi = (np.asarray(pprior[t.pprior_begin:t.pprior_begin + t.upper])
                      if t.flags & E.PCHOICE else np.full(t.upper, 1.0 / t.upper))
                kap = pi if k == 0 else J.kappa([int(mu[k])], sg[k], pi)[1]
                s = eng.sample(E.CAT, kap, seed=SEED, stream=JOINT_STREAM | i, offset=begin,
                               n=C.M)
            else:
                s = eng.sample(t.family, [1.0], [mu[k]], [sg[k]], *_sample_args(t), seed=SEED,
                               stream=JOINT_STREAM | i, offset=begin, n=C.M)
            want[at] = s[at]
        _same(vals[i], want, '%s hp %d' % (msg, i))


def _count_high(comp):
    return int((comp >= 256).sum()), int((comp >= 1024).sum())


@pytest.mark.parametrize('name', DRAW_SETS)
def test_joint_draws(name):
    cs = C.history()[0].space
    plan, model = _joint_plan(name), C.joint_model(name)
    eng, begin, P = plan.engine, BEGIN[name], plan.n_hp
    vals, total, terms, active, joint, comp = plan.joint_sample_points(
        SEED, C.M, begin=begin, want_terms=True, want_active=True, want_joint=True, want_comp=True)
    wb = plan.joint_mixture(-1, 0)[0]
    assert ((comp >= 0) & (comp < wb.size)).all() and wb.size == C.N_BELOW[name] + 1
    every = np.ones(C.M, dtype=bool)
    pick = eng.sample(E.CAT, wb, seed=SEED, stream=JOINT_STREAM | P, offset=begin, n=C.M)
    np.testing.assert_array_equal(comp, pick.astype(np.int32))
    _check_pick(comp, model.w[0], JOINT_STREAM | P, begin, every, name)
    print('%s: comp >= 256: %d, >= 1024: %d of %d' % ((name,) + _count_high(comp) + (C.M,)))
    if name == 'huge-below':
        assert min(_count_high(comp)) >= 1
    if name == 'prior-only':
        assert (comp == 0).all()
        for i in model.roots:
            t = _tables()[0][i]
            w, mu, sg, _ = plan.joint_mixture(i, 0)
            if t.family != E.CAT:
                pm, ps = O.posterior_spec(*[C.hp_list()[i][1][k] for k in ('dist', 'args')], 1.0)[1:3]
                assert (w.tolist(), mu.tolist(), sg.tolist()) == ([1.0], [pm], [ps])
    elif name != 'few-below':
        assert np.unique(comp).size > 2
    _check_component_draws(plan, plan.joint_mixture, model.roots, comp, every, vals, begin, name)
    # the conditional hps: sample_points' rule
    on = tpe.active_columns(cs, vals)
    np.testing.assert_array_equal(active == 1, on)
    tables = _tables()[0]
    for i in range(P):
        if i in model.roots:
            continue
        s = eng.sample(tables[i].family, *_mixture_args(plan, tables[i], i), seed=SEED, stream=i,
                       offset=begin, n=C.M)
        _same(vals[i][on[i]], s[on[i]], '%s hp %d' % (name, i))
        assert np.isnan(vals[i][~on[i]]).all()
    want = plan.joint_score_points(np.ascontiguousarray(vals), want_terms=True, want_active=True,
                                   want_joint=True)
    for g, w in zip((total, terms, active, joint), want):
        _same_bytes(g, w, name)


@pytest.mark.parametrize('name', DRAW_SETS)
def test_group_draws(name):
    cs = C.history()[0].space
    plan, model = _group_plan(name), C.group_model(name)
    eng, begin, P = plan.engine, BEGIN[name], plan.n_hp
    vals, total, active, joint, comp = plan.group_sample_points(
        SEED, C.M, begin=begin, want_active=True, want_joint=True, want_comp=True)
    on = tpe.active_columns(cs, vals)
    np.testing.assert_array_equal(active == 1, on)
    np.testing.assert_array_equal(np.isnan(vals), ~on)
    for g, hp_ids in enumerate(model.groups):
        sel = on[hp_ids[0]]
        assert (on[hp_ids] == sel).all() and sel.any()
        wb = plan.group_mixture(g, -1, 0)[0]
        assert ((comp[g][sel] >= 0) & (comp[g][sel] < wb.size)).all() and (comp[g][~sel] == -1).all()
        pick = eng.sample(E.CAT, wb, seed=SEED, stream=JOINT_STREAM | (P + g), offset=begin,
                          n=C.M)
        np.testing.assert_array_equal(comp[g], np.where(sel, pick, -1).astype(np.int32))
        _check_pick(comp[g], model.w[g][0], JOINT_STREAM | (P + g), begin, sel,
                    '%s group %d' % (name, g))
        if name == 'prior-only':
            assert (comp[g][sel] == 0).all()
        _check_component_draws(plan, functools.partial(plan.group_mixture, g), hp_ids, comp[g],
                               sel, vals, begin, '%s group %d' % (name, g))
    print('%s: group 0 comp >= 256: %d, >= 1024: %d; branches >= 256: %d, %d' % (
        (name,) + _count_high(comp[0]) + (_count_high(comp[1])[0], _count_high(comp[2])[0])))
    if name == 'huge-below':
        assert min(_count_high(comp[0])) >= 1
        assert _count_high(comp[1])[0] >= 1 and _count_high(comp[2])[0] >= 1
    want = plan.group_score_points(np.ascontiguousarray(vals), want_active=True, want_joint=True)
    for g, w in zip((total, active, joint), want):
        _same_bytes(g, w, name)


def test_over_cap_is_refused_by_the_joint_and_the_group_draw():
    """2101 below components: more than a draw table holds.  Both draws say
    so (TPE_E_INVALID) and leave the plan as it was."""
    jp, gp = _joint_plan('over-cap'), _group_plan('over-cap')
    assert jp.joint_mixture(-1, 0)[0].size == 2101 > R.TAB_CAP
    before_j = jp.joint_score_points(_cfg())
    before_g = gp.group_score_points(_cfg())
    msg = 'more below components than a draw table holds'
    with pytest.raises(ValueError, match='joint_sample_points: ' + msg):
        jp.joint_sample_points(SEED, C.M)
    with pytest.raises(ValueError, match='group_sample_points: ' + msg):
        gp.group_sample_points(SEED, C.M)
    lib = jp.engine.lib
    buf = np.zeros(10 * 8)
    assert lib.tpe_plan_joint_sample_points(jp.p, 1, 0, 4, 4, buf.ctypes.data, None,
                                            buf.ctypes.data, None, None, None, 0,
                                            None) == E.TPE_E_INVALID
    assert lib.tpe_plan_group_sample_points(gp.p, 1, 0, 4, 4, buf.ctypes.data, None,
                                            buf.ctypes.data, None, None, 0,
                                            None) == E.TPE_E_INVALID
    _same(jp.joint_score_points(_cfg()), before_j)
    _same(gp.group_score_points(_cfg()), before_g)
    # the marginal draw of the same plan goes through (test_marginal_draws)
    assert np.isfinite(jp.sample_points(SEED, 8)[1]).all()


# ----------------------------------------------------------- the pending batch
@pytest.mark.parametrize('name', C.BATCH_SETS)
def test_pending_batch(name):
    _, _, pw, lf = C.FIT_SETS[name]
    plan, model = _group_plan(name), C.group_model(name)
    vals, k = _cfg(), C.K_BATCH
    total = plan.group_score_points(vals)
    idx, gain, trace = plan.group_batch_points(vals, k, want_trace=True)
    _check_identities(plan, model, vals, k, total, idx, gain, trace, msg=name)
    # the device's scores against the oracle replayed on the device's picks
    res = B.run(model, vals, k, forced=idx, prior_weight=pw, lf=lf)
    nan = np.isnan(res.scores)
    np.testing.assert_array_equal(np.isnan(trace), nan, err_msg=name)
    with np.errstate(all='ignore'):
        err = np.abs(trace - res.scores)
        ok = nan | (err <= res.bound)
        worst = float(np.max(np.where(nan, 0.0, err / res.bound)))
    print('%s: picks %s, max |d score| / bound = %.3g' % (name, idx.tolist(), worst))
    assert ok.all(), (name, np.argwhere(~ok)[:5])
    assert (trace[-1] != trace[0]).sum() > 1
    # the picks are the oracle's; where its two best scores of a round are
    # closer than twice the bound (at most one round per set:
    # test_fit_sets_points_host.py) either is accepted
    free = C.batch_run(name)
    if (free.ratio >= 2.0).all():
        np.testing.assert_array_equal(idx, free.picks, err_msg=name)
    assert (res.ratio > -2.0).all(), (name, res.ratio)


# --------------------------------------------------------- the entry points
def test_score_configs_passes_gamma_and_prior_weight():
    """tpe.score_configs with gamma = 0 (no below row: the prior alone) and
    with prior_weight = 0 under the group model, on a 40-trial history: the
    plan calls with those parameters."""
    n = 40
    cfg, _, _ = C.configs()
    pool = _cfg()
    dom, trials = C.make_trials(n)
    ei, terms, active = tpe.score_configs(pool, dom, trials, gamma=0.0, return_terms=True)
    plan = _new_plan(n=n, gamma=0.0, prior_weight=1.0)
    assert all(plan.mixture(i, 0)[0].size == (t.upper if t.family == E.CAT else 1)
               for i, t in enumerate(_tables()[0]))
    total, t_, a_ = plan.score_points(pool, want_terms=True, want_active=True)
    _same(ei, total)
    for i, lab in enumerate(C.labels()):
        _same(terms[lab], t_[i])
        np.testing.assert_array_equal(active[lab], a_[i] == 1)
    assert np.isfinite(ei).all()
    dom, trials = C.make_trials(n)
    ei, _, _, joint = tpe.score_configs(pool, dom, trials, prior_weight=0.0, return_terms=True,
                                        multivariate='groups')
    plan = _new_plan(n=n, gamma=0.25, prior_weight=0.0)
    plan.group_fit()
    assert plan.group_mixture(0, -1, 0)[0][0] == 0.0
    total, gj = plan.group_score_points(pool, want_joint=True)
    _same(ei, total)
    _same(joint, gj)
    assert np.isnan(ei).any() and np.isfinite(ei).any()
