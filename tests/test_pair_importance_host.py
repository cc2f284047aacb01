"""The pairwise importance rule in its numpy restatement alone: no device.

On the checkerboard (32 rows, the two best at (0.8, 0.8) and (-0.8, -0.8), the rest on the
anti-diagonal) at ghat = 2 / 32 and 64 nodes per dim: D_x = D_y = 0.1312, D_xy = 10.95, 83.4
times either marginal."""
import numpy as np

import group_oracle as G
import importance_oracle as IO
import pair_importance_oracle as PO
import test_joint_host as TJ
from hyperopt_amd import _engine as E, tpe

NODES = 64


def test_checkerboard_pair_outweighs_both_marginals():
    assert 'tpe_plan_group_importance_pairs' in E.EXPORTS and E.Plan.importance_pairs
    assert 'pairs' in tpe.importances.__code__.co_varnames
    hps, losses, vals = TJ.checkerboard()
    m = G.GroupModel(hps, losses, vals, np.ones_like(vals), 0.25, 1.0)
    ghat = m.rows[0][0].size / float(losses.size)
    assert ghat == 2 / 32.0
    a, b, w = PO.from_group_model(m, 0, 0, 1)
    _, wa, _, wb, L = PO.planes(a, b, w, NODES)
    r = PO.integrate(L, wa, wb, ghat)
    marg = [IO.importance('uniform', (-1, 1), m.dims[0][0][i].marginal, m.dims[0][1][i].marginal,
                          ghat, NODES)['D'] for i in range(2)]
    print('D_x = %.4g, D_y = %.4g, D_xy = %.4g, ratio %.3g' % (marg[0], marg[1], r['D'],
                                                               r['D'] / max(marg)))
    # (the kernels carry no truncation normaliser: part of each side's mass lies past [-1, 1]^2)
    assert 0.2 < r['Zb'] < 1 and 0.2 < r['Za'] < 1
    assert 0 < max(marg) * 10 < r['D'] <= 1 / ghat - 1


def test_prior_alone_on_both_sides_gives_zero():
    prior = [(np.array([0.0]), np.array([2.0]))] * 2
    cat = [(np.array([-1.0]), np.array([0.5]))] * 2
    a, b = ('uniform', (-1, 1), prior), ('randint', (3,), cat)
    _, wa, _, wb, L = PO.planes(a, b, [np.ones(1), np.ones(1)], 16)
    assert L[0].shape == (16, 3) and PO.integrate(L, wa, wb, 0.25)['D'] == 0.0
