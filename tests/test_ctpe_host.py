"""c-TPE on the host: the Python layer's nb / ghat rule against the oracle's
row-by-row restatement, the argument errors, and one sense check of the rule."""
import numpy as np
import pytest

from hyperopt_amd import hp, tpe, Trials
from hyperopt_amd.base import Domain

import ctpe_oracle as CO
import spaces

INF, NAN = np.inf, np.nan
LOSS = np.arange(40.0)[::-1].copy()         # row 39 is the best, row 0 the worst


def _case(name):
    losses, G = LOSS.copy(), np.full((2, 40), 1.0)      # 'none_feasible' as it stands
    if name == 'all_feasible':
        G[:] = -1.0
    elif name == 'best_feasible_deep':      # the only fully feasible row is 30th in loss order
        G[:, 10], G[0, :25] = 0.0, -2.0
    elif name == 'nan_constraint':
        G[0, :30], G[0, 5], G[1, 7] = -1.0, NAN, NAN
    elif name == 'pending_rows':
        G[:], G[1, ::2], losses[[3, 4, 38]] = -1.0, 3.0, INF
    return losses, G


@pytest.mark.parametrize('name', ['none_feasible', 'all_feasible', 'best_feasible_deep',
                                  'nan_constraint', 'pending_rows'])
def test_counts_follow_the_rule(name):
    losses, G = _case(name)
    nb, ghat = tpe.ctpe_counts(losses, G, 0.25)
    want_nb, want_ghat, live = CO.counts(losses, G, 0.25)
    np.testing.assert_array_equal(nb, want_nb)
    assert nb.dtype == np.int32 and ghat.tobytes() == want_ghat.tobytes()
    # (the plain count is min(ceil(0.25 sqrt(40)), 25) = 2)
    want = {'none_feasible': ([2, 2, 2], [0, 1, 2]), 'all_feasible': ([2, 40, 40], [0]),
            'best_feasible_deep': ([30, 25, 2], [0, 1, 2]),
            'nan_constraint': ([2, 29, 2], [0, 1, 2]), 'pending_rows': ([2, 37, 19], [0, 2])}
    assert (nb.tolist(), live) == want[name]
    assert ghat.tolist() == [b / int(np.isfinite(losses).sum()) for b in nb]


def test_argument_errors():
    dom, tr = Domain(lambda x: 0.0, spaces.cond_space(hp)), Trials()
    with pytest.raises(ValueError, match='suggest_joint'):
        tpe.suggest([0], dom, tr, 1, constraints=2, constraint_model='ctpe')
    for kw in (dict(constraint_model='ctpe'),                       # no constraints
               dict(constraints=2, constraint_model='ctpe', multivariate=True),
               dict(constraints=2, constraint_model='ctpe', multivariate='groups'),
               dict(constraints=2, constraint_model='c-tpe')):
        for call in (lambda: tpe.score_configs([], dom, tr, **kw),
                     lambda: tpe.sample_configs(4, dom, tr, 1, **kw),
                     lambda: tpe.suggest_from_pool([0], dom, tr, 1, pool=[], **kw),
                     lambda: tpe.suggest_joint([0], dom, tr, 1, **kw)):
            with pytest.raises(ValueError, match='constraint_model|multivariate'):
                call()
    with pytest.raises(ValueError, match='multivariate|pending'):
        tpe.suggest_joint([0], dom, tr, 1, constraints=2, constraint_model='ctpe',
                          multivariate='groups', batch='pending')
    with pytest.raises(ValueError, match='complete'):
        tpe.ctpe_counts([INF, INF], [[0.0, 0.0]])


def test_constraint_model_moves_the_ranking_to_the_feasible_side():
    """x, y uniform on [0, 1], loss x^2 + y^2, feasible when x >= 0.5: the low-loss corner is
    infeasible.  The ranking pass's model alone (T_0, fitted without the constraint) prefers the
    unconstrained optimum to a feasible point at the boundary; c-TPE's acquisition the latter."""
    dom = Domain(lambda x: 0.0, {'x': hp.uniform('x', 0, 1), 'y': hp.uniform('y', 0, 1)})
    cs = dom.space
    rs = np.random.RandomState(0)
    hv = rs.uniform(0, 1, (2, 200))
    losses = (hv ** 2).sum(axis=0)
    G = (0.5 - hv[cs.labels.index('x')])[None, :]
    ha = np.ones((2, 200), dtype=np.uint8)
    pts = np.array([[0.05, 0.55], [0.05, 0.05]])            # [optimum, feasible]; rows x, y
    if cs.labels.index('x') != 0:
        pts = pts[::-1]
    nb, ghat = tpe.ctpe_counts(losses, G, 0.25)
    key = CO.keys(losses, G)
    T = []
    for m in range(2):
        lb, la = CO.model_lliks(cs, key[m], nb[m], hv, ha, pts, np.ones((2, 2), dtype=np.uint8))
        T.append((lb - la).sum(axis=0))
    acq = CO.acquisition(ghat, T)
    assert T[0][0] > T[0][1] and acq[1] > acq[0]
