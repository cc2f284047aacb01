"""Host side of multivariate TPE with one joint model per group of hps (no
GPU): the partition -- in Python and, by a stand-alone sanitized program, in
the engine's host header --, the oracle's anchors to the marginal model and to
the root model, the interaction inside a branch that the groups exist for, the
ABI additions, and the ``multivariate='groups'`` plumbing over a stub plan."""
import os
import re
import subprocess

import numpy as np
import pytest

import hyperopt_amd as H
from hyperopt_amd import hp, rand, tpe, Trials, trials_from_docs
from hyperopt_amd import _engine as E
from hyperopt_amd.base import Domain

from oracle import tpe_oracle as O
from oracle_algo import oracle_hps
import group_oracle as G
import joint_oracle as J
import spaces
import test_joint_host as TJ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
GAMMA, PRIOR_WEIGHT = 0.25, 1.0
NESTED_GROUPS = [('top',), ('inner', 'w'), ('p', 'q'), ('r',), ('shared',), ('v',), ('z',)]


# ------------------------------------------------------------ the partition
def test_hp_groups_of_cond_space():
    cs = Domain(lambda x: 0.0, spaces.cond_space(hp)).space
    assert tpe.hp_groups(cs) == [('aa', 'top')] + [
        ('act%d' % b, 'lr%d' % b, 'units%d' % b, 'zz%d' % b) for b in range(3)]


def test_hp_groups_of_cfg3_space():
    cs = Domain(lambda x: 0.0, spaces.cfg3_space(hp)).space
    groups = tpe.hp_groups(cs)
    assert cs.labels[0] == 'ch0'                # (group 0 is the root all the same)
    assert groups[0] == ('top',) and len(groups) == 8
    for b, g in enumerate(groups[1:]):
        assert g == tuple(sorted(['ch%d' % b] + ['lr%d_%d' % (b, j) for j in range(3)] +
                                 ['un%d_%d' % (b, j) for j in range(3)]))


def test_hp_groups_of_a_nested_space_with_a_shared_label():
    cs = Domain(lambda x: 0.0, G.nested_space(hp)).space
    assert cs.by_label['shared'].conds() == (('top', 0), ('top', 1))
    assert tpe.hp_groups(cs) == NESTED_GROUPS
    # the oracle's partition is the same one, as indices
    hps = oracle_hps(cs)
    parts = G.partition([(lab, hps[lab]) for lab in cs.labels])
    assert [tuple(cs.labels[i] for i in g) for g in parts] == NESTED_GROUPS


def test_group_plan_host_checks(tmp_path):
    """The engine's partition and layout (tpe_group_plan.hpp) on hand-built
    condition tables: host-only, address and undefined-behaviour sanitizers,
    a stand-alone program."""
    if not os.path.exists(HIPCC):
        pytest.fail('hipcc not found at %s' % HIPCC)
    exe = str(tmp_path / 'group_plan_check')
    src = os.path.join(ROOT, 'tests', 'host', 'group_plan_check.cpp')
    cc = subprocess.run(
        [HIPCC, '-x', 'hip', '--cuda-host-only', '-std=c++17', '-O1', '-g', '-Wall',
         '-Xarch_host', '-fsanitize=address,undefined',
         '-Xarch_host', '-fno-sanitize-recover=undefined', src, '-o', exe],
        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert cc.returncode == 0, cc.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       universal_newlines=True)
    assert r.returncode == 0, r.stdout


# ---------------------------------------------------------------- the oracle
def _done(docs, losses):
    for d, l in zip(docs, losses):
        d['state'] = H.JOB_STATE_DONE
        d['result'] = {'status': 'ok', 'loss': float(l)}
    return trials_from_docs(docs)


def _rand_history(make, n, seed):
    dom = Domain(lambda x: 0.0, make(hp))
    docs = rand.suggest(list(range(n)), dom, Trials(), seed)
    _, losses, vals, active = tpe.build_history(
        dom, _done(docs, np.random.RandomState(seed + 100).rand(n)))
    h = oracle_hps(dom.space)
    return dom, [(lab, h[lab]) for lab in dom.space.labels], losses, vals, active


@pytest.fixture(scope='module')
def nested():
    dom, hps, losses, vals, active = _rand_history(G.nested_space, 80, 7)
    return dom, hps, losses, vals, active, G.GroupModel(hps, losses, vals, active, GAMMA,
                                                        PRIOR_WEIGHT)


def test_the_hps_of_a_group_are_active_together(nested):
    dom, hps, losses, vals, active, model = nested
    for g in model.groups:
        assert (active[g] == active[g[0]]).all()
    assert active[model.groups[0]].all()
    # and the oracle's activity of the history rows is the history's
    on = model.active(vals)
    for gi, g in enumerate(model.groups):
        np.testing.assert_array_equal(on[gi], active[g[0]] == 1)


def _marginal_sides(h, losses, col, act):
    tids = np.arange(losses.size)
    return O.split_observations(tids[act == 1], col[act == 1], tids, losses, GAMMA, kind='stable')


def test_group_components_are_the_marginal_mixtures(nested):
    """Per group, hp and side the multiset {(w, mu, sigma)} is the mixture
    the marginal fit of that hp gives on the rows it is active in."""
    dom, hps, losses, vals, active, model = nested
    for gi, g in enumerate(model.groups):
        for j, i in enumerate(g):
            h = hps[i][1]
            obs = _marginal_sides(h, losses, vals[i], active[i])
            for s in range(2):
                d = model.dims[gi][s][j]
                np.testing.assert_array_equal(vals[i][model.rows[gi][s]], obs[s])
                if d.cat:
                    continue
                fk, pm, ps, low, high, q, tr = O.posterior_spec(h['dist'], h['args'], PRIOR_WEIGHT)
                want = O.parzen_fit(O.transform_obs(obs[s], tr, low), PRIOR_WEIGHT, pm, ps,
                                    kind='stable')
                order = np.lexsort((np.concatenate([[-1], model.rows[gi][s]]), d.mu))
                for got, w in zip((d.w, d.mu, d.sigma), want):
                    np.testing.assert_array_equal(got[order], w)


@pytest.mark.parametrize('label,exact', [('shared', True), ('v', True), ('r', False),
                                         ('z', False)])
def test_one_hp_group_is_the_marginal_term(nested, label, exact):
    """J_below - J_above of a group of one hp is score_hp's llik_b - llik_a:
    exactly for log-continuous and categorical kinds, up to one constant per
    fit (the two truncation masses) for uniform and quniform."""
    dom, hps, losses, vals, active, model = nested
    i = dom.space.labels.index(label)
    gi = model.group_of[i]
    assert model.groups[gi] == [i]
    h = hps[i][1]
    cand = O.prior_sample(np.random.RandomState(3), h['dist'], h['args'], 64).astype(np.float64)
    d = [model.dims[gi][s][0] for s in range(2)]
    with np.errstate(all='ignore'):
        js = [O.lse_rows(np.log(model.w[gi][s])[None, :] + d[s].log_kernel(cand))
              for s in range(2)]
        bo, ao = _marginal_sides(h, losses, vals[i], active[i])
        r = O.score_hp(h['dist'], h['args'], bo, ao, PRIOR_WEIGHT, cand, kind='stable')
    diff = (js[0] - js[1]) - (r['llik_b'] - r['llik_a'])
    assert np.isfinite(diff).all()
    print('%s: max |diff| %.3g, spread %.3g' % (label, np.abs(diff).max(), np.ptp(diff)))
    if exact:
        assert np.abs(diff).max() <= 1e-12
    else:
        assert np.ptp(diff) <= 1e-12


def test_on_a_space_without_conditions_the_group_model_is_the_joint_model():
    dom, hps, losses, vals, active = _rand_history(spaces.many_dists_space, 60, 11)
    gm = G.GroupModel(hps, losses, vals, active, GAMMA, PRIOR_WEIGHT)
    jm = J.JointModel(hps, losses, vals, GAMMA, PRIOR_WEIGHT)
    assert gm.groups == [list(range(11))]
    gb, ga = gm.sides(vals)
    jb, ja = jm.sides(vals)
    np.testing.assert_array_equal(gb[0], jb)
    np.testing.assert_array_equal(ga[0], ja)
    np.testing.assert_array_equal(gm.total(vals), 0.0 + jm.joint(vals))


# ------------------------------------------------ the interaction in a branch
def conditional_checkerboard():
    """test_joint_host's checkerboard inside branch 0 of a two-branch choice,
    with 16 rows of the other branch (worse than every checkerboard row)
    interleaved: one after every two checkerboard rows."""
    _, cl, cv = TJ.checkerboard()
    u = dict(dist='uniform', args=(-1, 1))
    hps = [('top', dict(dist='randint', args=(2,), paths=[()])),
           ('x', dict(paths=[(('top', 0),)], **u)), ('y', dict(paths=[(('top', 0),)], **u)),
           ('z', dict(paths=[(('top', 1),)], **u))]
    cols, losses = [], []
    for j in range(32):
        cols.append((0.0, cv[0, j], cv[1, j], np.nan))
        losses.append(cl[j])
        if j % 2 == 1:
            cols.append((1.0, np.nan, np.nan, -0.9 + 0.1 * (j // 2)))
            losses.append(3.0 + j)
    vals = np.array(cols).T
    return hps, np.array(losses), vals, (~np.isnan(vals)).astype(np.uint8)


def test_conditional_checkerboard_is_visible_to_the_group_model_only():
    hps, losses, vals, active = conditional_checkerboard()
    assert vals.shape == (4, 48)
    cfg = np.array([[0.0, 0.0], [0.8, 0.8], [0.8, -0.8], [np.nan, np.nan]])   # on / off diagonal
    gm = G.GroupModel(hps, losses, vals, active, GAMMA, PRIOR_WEIGHT)
    assert gm.groups == [[0], [1, 2], [3]] and gm.rows[1][0].tolist() == [0, 1]
    assert gm.rows[1][1].size == 30 and gm.rows[2][1].size == 16
    total = gm.total(cfg)
    np.testing.assert_array_equal(gm.active(cfg), [[True, True], [True, True], [False, False]])
    # multivariate=True on this space: the root model over `top` plus marginal terms
    jm = J.JointModel(hps, losses, vals, GAMMA, PRIOR_WEIGHT)
    tids = np.arange(losses.size)
    marg = jm.joint(cfg)
    for i in (1, 2):
        bo, ao = O.split_observations(tids[active[i] == 1], vals[i][active[i] == 1], tids, losses,
                                      GAMMA, kind='stable')
        with np.errstate(all='ignore'):
            r = O.score_hp('uniform', (-1, 1), bo, ao, PRIOR_WEIGHT, cfg[i], kind='stable')
        marg = marg + (r['llik_b'] - r['llik_a'])
    print('groups on / off %s, root model + marginal terms on / off %s' % (total, marg))
    assert total[0] - total[1] > 1
    assert abs(marg[0] - marg[1]) < 1e-3


# ------------------------------------------------------------------- the ABI
def test_abi_additions():
    names = ('tpe_plan_group_info', 'tpe_plan_group_fit', 'tpe_plan_group_get_mixture',
             'tpe_plan_group_score_points', 'tpe_plan_group_sides',
             'tpe_plan_group_sample_points')
    hdr = os.path.join(ROOT, 'include', 'tpe_engine.h')
    declared = set(re.findall(r'\b(tpe_[a-z_]+)\s*\(', open(hdr).read()))
    for nm in names:
        assert nm in declared and nm in E.EXPORTS
    for meth in ('group_info', 'group_fit', 'group_mixture', 'group_score_points',
                 'group_score_points_device', 'group_sides', 'group_sample_points',
                 'group_sample_points_device'):
        assert callable(getattr(E.Plan, meth))
    if os.path.exists(E.LIB_PATH):
        lib = E.load_library()
        for nm in names:
            assert getattr(lib, nm).argtypes is not None


# -------------------------------------------------------------- the plumbing
class StubPlan(TJ.StubPlan):
    def group_fit(self):
        self.calls.append('group_fit')

    def group_score_points(self, vals, want_active=False, want_joint=False):
        self.calls.append('group_score_points')
        m = vals.shape[1]
        out = (-np.arange(m, dtype=float),) + \
            ((tpe.active_columns(self.cs, vals).astype(np.uint8),) if want_active else ()) + \
            ((np.full((4, m), 5.0),) if want_joint else ())
        return out[0] if len(out) == 1 else out

    def group_sample_points(self, seed, m, begin=0):
        self.calls.append(('group_sample_points', seed, m, begin))
        return np.full((self.P, m), 2.0), np.full(m, 2.0)


@pytest.fixture
def stub(monkeypatch):
    dom = Domain(lambda x: 0.0, spaces.cond_space(hp))
    plan = StubPlan(len(dom.space.labels))
    plan.cs = dom.space
    monkeypatch.setattr(tpe._State, 'plan_for', lambda self, domain, n, engine: plan)
    monkeypatch.setattr(E, 'default_engine', lambda *a: None)
    return dom, plan, TJ._history(dom, 6)


def test_groups_argument_reaches_the_group_calls(stub):
    dom, plan, trials = stub
    cs = dom.space
    hv, ha = TJ.trials_vals(cs, trials)
    pool = np.where(ha == 1, hv, np.nan)
    dicts = tpe.columns_to_configs(cs, pool, ~np.isnan(pool))
    ei, terms, active, joint = tpe.score_configs(pool, dom, trials, return_terms=True,
                                                 multivariate='groups')
    assert plan.calls == ['fit', 'group_fit', 'group_score_points']
    assert joint.shape == (4, pool.shape[1]) and (joint == 5.0).all()
    assert sorted(terms) == cs.labels and all((terms[lab] == 0.0).all() for lab in cs.labels)
    assert active['top'].all()
    assert np.array_equal(tpe.score_configs(pool, dom, trials, multivariate='groups'), ei)
    del plan.calls[:]
    vals, total = tpe.sample_configs(5, dom, trials, 1, begin=9, multivariate='groups')
    assert plan.calls == ['fit', 'group_fit',
                          ('group_sample_points', tpe.batch_seeds(1, 1)[0], 5, 9)]
    assert (vals == 2.0).all() and (total == 2.0).all()
    del plan.calls[:]
    docs = tpe.suggest_from_pool([10], dom, trials, 1, pool=dicts, n_startup_jobs=0,
                                 skip_seen=False, multivariate='groups')
    assert plan.calls == ['fit', 'group_fit', 'group_score_points']
    got = {lab: v[0] for lab, v in docs[0]['misc']['vals'].items() if v}
    assert got == tpe.columns_to_configs(cs, pool[:, :1], ~np.isnan(pool[:, :1]))[0]
    # True still takes the root model's calls
    del plan.calls[:]
    tpe.score_configs(pool, dom, trials, multivariate=True)
    tpe.sample_configs(5, dom, trials, 1, multivariate=True)
    assert [c if isinstance(c, str) else c[0] for c in plan.calls] == [
        'fit', 'joint_fit', 'joint_score_points', 'fit', 'joint_fit', 'joint_sample_points']


@pytest.mark.parametrize('bad', ['group', 2, 1, None, 'True'])
def test_other_values_of_multivariate_raise(stub, bad):
    dom, plan, trials = stub
    cs = dom.space
    hv, ha = TJ.trials_vals(cs, trials)
    pool = np.where(ha == 1, hv, np.nan)
    for call in (lambda: tpe.score_configs(pool, dom, trials, multivariate=bad),
                 lambda: tpe.sample_configs(5, dom, trials, 1, multivariate=bad),
                 lambda: tpe.suggest_from_pool([10], dom, trials, 1, pool=pool, n_startup_jobs=0,
                                               multivariate=bad),
                 lambda: tpe.suggest_joint([10], dom, trials, 1, n_startup_jobs=0,
                                           multivariate=bad)):
        with pytest.raises(ValueError, match='multivariate must be'):
            call()
    assert plan.calls == []


def test_groups_need_their_hps_active_together(stub):
    dom, plan, trials = stub
    st = tpe._state(dom)
    with st.lock:
        hist = st.history(dom, trials).sync(trials)
    labels = dom.space.labels
    a, l = labels.index('act1'), labels.index('lr1')
    rows = np.flatnonzero(np.asarray(hist.active)[l, :hist.n])
    assert rows.size, 'the stub history never takes branch 1'
    j = int(rows[-1])
    hist.active[a, j] = 0
    try:
        with pytest.raises(ValueError, match="row %d .*'act1'" % j):
            tpe._fit_for(st, dom, trials, hist, None, PRIOR_WEIGHT, GAMMA, multivariate='groups')
        assert 'group_fit' not in plan.calls
        tpe._fit_for(st, dom, trials, hist, None, PRIOR_WEIGHT, GAMMA, multivariate=True)
    finally:
        hist.active[a, j] = 1
    # a root missing in a row: the message multivariate=True gives
    i = labels.index('aa')
    hist.active[i, 2] = 0
    try:
        with pytest.raises(ValueError, match="row 2 .*'aa'"):
            tpe._fit_for(st, dom, trials, hist, None, PRIOR_WEIGHT, GAMMA, multivariate='groups')
    finally:
        hist.active[i, 2] = 1
    tpe._fit_for(st, dom, trials, hist, None, PRIOR_WEIGHT, GAMMA, multivariate='groups')
    assert plan.calls[-2:] == ['fit', 'group_fit']


def test_suggest_joint_startup_ignores_groups():
    dom = Domain(lambda x: 0.0, spaces.cond_space(hp))
    a = tpe.suggest_joint([0, 1], dom, Trials(), 5, multivariate='groups')
    b = tpe.suggest_joint([0, 1], dom, Trials(), 5)
    assert [d['misc']['vals'] for d in a] == [d['misc']['vals'] for d in b]
