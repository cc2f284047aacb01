"""Importances from the fitted models on the GPU against tests/importance_oracle.py
on the mixtures the plan holds, so only the kernel's arithmetic is under test.  Per lpdf the bar is
gpu_util.RTOL max(1, |lpdf|); D and mass lie within 3 B + 64 eps (tiles + 8) S of the oracle, B the
first-order change of D under that bar, S the sum of |f|.  The plain cases pass ghat = 0.25, where
the allowance covers the mass too: its change is at most sum w eps max(l, g), and (1 - ghat)^2
(l + g)^2 / q >= 0.56 max(l, g), a third of it at least."""
import functools

import numpy as np
import pytest

import hyperopt_amd as H
from hyperopt_amd import hp, rand, tpe, Trials, trials_from_docs
from hyperopt_amd import _engine as E
from hyperopt_amd.base import Domain

import importance_oracle as IO
import spaces
from gpu_util import RTOL

pytestmark = pytest.mark.gpu

GHAT, EPS = 0.25, np.finfo(np.float64).eps
KINDS = sorted(spaces.many_dists_space(hp))


def _space(name):
    if name == 'cond':
        return spaces.cond_space(hp)
    return {lab: spaces.many_dists_space(hp)[lab] for lab in name}


@functools.lru_cache(maxsize=None)
def _history(name, rows, constraints=False):
    dom = Domain(lambda x: 0.0, _space(name))
    docs = rand.suggest(list(range(rows)), dom, Trials(), 11)
    rng = np.random.RandomState(rows)
    losses, g = rng.rand(rows), rng.randn(rows)
    g[np.argmin(losses)] = -1.0                   # the best row is feasible: nb[0] stays plain
    for d, l, gi in zip(docs, losses, g):
        d['state'] = H.JOB_STATE_DONE
        d['result'] = {'status': 'ok', 'loss': float(l)}
        if constraints:
            d['result']['constraints'] = [float(gi), -1.0]       # the second never binds
    trials = trials_from_docs(docs)
    _, ls, vals, act = tpe.build_history(dom, trials, dom.space.labels)
    return dom, trials, np.asarray(ls), np.ascontiguousarray(vals), np.ascontiguousarray(act), g


def _new_plan(cs, losses, vals, active, fit=True):
    hps, conds, pprior = cs.engine_tables()
    plan = E.Plan(E.default_engine(), hps, conds, pprior, max_trials=losses.size)
    plan.set_history(losses, vals, active)
    if fit:
        plan.fit(gamma=0.25, prior_weight=1.0)
    return plan


@functools.lru_cache(maxsize=None)
def _plan(name, rows):
    dom, _, losses, vals, active, _ = _history(name, rows)
    return _new_plan(dom.space, losses, vals, active), dom.space


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check_layer(cs, get, ghat, G, D, mass, curves, msg):
    """One model against the oracle on get(i, side)'s mixtures; the worst allowance fraction."""
    worst = 0.0
    tiles = -(-G // IO.TILE)
    for i, lab in enumerate(cs.labels):
        h, cat = cs.by_label[lab], cs.by_label[lab].dist in ('randint', 'categorical')
        below, above = (get(i, side)[0] if cat else get(i, side) for side in (0, 1))
        x, w, _ = IO.nodes(h.dist, h.args, below, above, G)
        k = x.size
        lb, la = IO.lpdfs(h.dist, h.args, below, above, x)
        if curves is not None:
            gx, glb, gla = (c[i] for c in curves)
            assert (_bits(gx[:k]) == _bits(x)).all(), (msg, lab, 'nodes')
            assert all(np.isnan(c[k:]).all() for c in (gx, glb, gla)), (msg, lab, 'padding')
            for got, want in ((glb[:k], lb), (gla[:k], la)):
                fin = np.isfinite(want)
                np.testing.assert_array_equal(got[~fin], want[~fin], err_msg=str((msg, lab)))
                err = np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin]))
                assert (err <= RTOL).all(), (msg, lab, 'lpdf', err.max())
        r = IO.integrate(lb, la, w, ghat, RTOL)
        allow = 3 * r['B'] + 64 * EPS * (tiles + 8) * r['S']
        for got, want in ((D[i], r['D']), (mass[i], r['mass'])):
            assert abs(got - want) <= allow, (msg, lab, got, want, allow)
            worst = max(worst, abs(got - want) / allow if allow else 0.0)
    return worst


@pytest.mark.parametrize('G', [64, 320])
@pytest.mark.parametrize('rows', [1, 40, 300])
@pytest.mark.parametrize('name', KINDS + ['cond'])
def test_curves_d_and_mass_match_the_oracle(name, rows, G):
    plan, cs = _plan(name, rows)
    D, norm, mass, x, lb, la = plan.importance(G, [GHAT], want_curves=True)
    worst = _check_layer(cs, plan.mixture, GHAT, G, D[0], mass[0], (x[0], lb[0], la[0]),
                         (name, rows, G))
    print('%s rows %d G %d: worst fraction of the allowance %.3g' % (name, rows, G, worst))
    # node by node (l / q - 1)^2 <= (1 / ghat - 1)^2, whatever the nodes cover
    assert (D >= 0).all() and (D <= (1 / GHAT - 1) ** 2 * mass * (1 + 1e-12)).all()
    assert abs(norm.sum() - 1.0) < 1e-12 if D.sum() else norm.sum() == 0.0
    assert (_bits(plan.importance(G, [1.0])[0]) == 0).all()


def test_ctpe_layers_and_the_dead_constraint():
    dom, trials, losses, vals, active, g = _history('ac', 40, True)
    Gm = np.ascontiguousarray(np.stack([g, np.full(40, -1.0)]))
    nb, ghat = tpe.ctpe_counts(losses, Gm)
    assert ghat[2] == 1.0 and ghat[1] < 1.0 and nb[0] == 2
    plan = _new_plan(dom.space, losses, vals, active, fit=False)
    plan.ctpe_fit(Gm, nb, ghat)
    D, norm, mass = plan.importance(64)
    plain = _new_plan(dom.space, losses, vals, active).importance(64, [ghat[0]])
    assert (_bits(D[0]) == _bits(plain[0][0])).all()
    _check_layer(dom.space, functools.partial(plan.ctpe_mixture, 1), ghat[1], 64, D[1], mass[1],
                 None, 'ctpe layer 1')
    imp = tpe.importances(dom, trials, n_nodes=64, constraints=2, constraint_model='ctpe')
    assert list(imp) == ['objective', 'constraint 0', 'constraint 1']
    assert list(imp['constraint 1'].values()) == [0.0, 0.0]
    for m, name in enumerate(('objective', 'constraint 0')):
        assert (_bits(list(imp[name].values())) == _bits(norm[m])).all()
    raw = tpe.importances(dom, trials, n_nodes=64, normalize=False)
    assert list(raw) == dom.space.labels and (_bits(list(raw.values())) == _bits(D[0])).all()


def test_an_hp_scores_the_same_alone_and_among_others():
    dom, _, losses, vals, active, _ = _history('acg', 40)
    i = dom.space.labels.index('c')
    among = _new_plan(dom.space, losses, vals, active).importance(320, [GHAT])
    alone_cs = Domain(lambda x: 0.0, _space('c')).space
    alone = _new_plan(alone_cs, losses, vals[i:i + 1].copy(), active[i:i + 1].copy())
    D, _, mass = alone.importance(320, [GHAT])
    assert _bits(D[0, 0]) == _bits(among[0][0, i]) and _bits(mass[0, 0]) == _bits(among[2][0, i])


def test_refusals():
    dom, _, losses, vals, active, _ = _history('c', 40)
    with pytest.raises(ValueError):
        _new_plan(dom.space, losses, vals, active, fit=False).importance(64, [GHAT])
    plan, _ = _plan('c', 40)
    for bad, ghat in ((100, GHAT), (0, GHAT), (65536 + 64, GHAT), (64, 0.0)):
        with pytest.raises(ValueError):
            plan.importance(bad, [ghat])
