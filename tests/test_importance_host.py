"""The importance rule in its numpy restatement alone: no device."""
import numpy as np
import pytest

import importance_oracle as IO
from hyperopt_amd import _engine as E, tpe
from oracle import tpe_oracle as O

# gamma = 1: 8 of 60 rows on the good side.  At the default 0.25 the good side is 2 rows, and
# two points say as much about where an irrelevant hp's good trials lie as about a relevant
# one's (the ratio below has median 2.2 over seeds 0..299, against 9.2 here)
GAMMA = 1.0
UNIFORM, NORMAL = ('uniform', (0.0, 1.0)), ('normal', (0.0, 1.0))


def _fit(dist, args, vals, losses):
    """(below, above) mixtures of one hp over a complete history, and ghat."""
    tids = np.arange(losses.size)
    bo, ao = O.split_observations(tids, vals, tids, losses, GAMMA, kind='stable')
    _, pm, ps = O.posterior_spec(dist, args, 1.0)[:3]
    return (O.parzen_fit(bo, 1.0, pm, ps, kind='stable'),
            O.parzen_fit(ao, 1.0, pm, ps, kind='stable'), bo.size / float(losses.size))


def test_the_hp_the_loss_depends_on_outweighs_the_other():
    assert tpe.importances and E.Plan.importance       # the feature this file restates
    rng = np.random.RandomState(2)
    x, y = rng.uniform(0, 1, 60), rng.uniform(0, 1, 60)
    D = [IO.importance(*UNIFORM, *_fit(*UNIFORM, v, x * x))['D'] for v in (x, y)]
    print('D[x] = %.4g, D[y] = %.4g' % tuple(D))
    assert D[0] > 10 * D[1] > 0


@pytest.mark.parametrize('dist, args', [UNIFORM, NORMAL])
def test_mass_is_one_and_ghat_one_gives_zero(dist, args):
    # 20 rows: the midpoint rule misses a bounded hp's mass by h^2 / 24 (q'(high) - q'(low)),
    # 4e-8 times a slope difference that grows as the components narrow with the history
    rng = np.random.RandomState(5)
    v = rng.uniform(0, 1, 20) if dist == 'uniform' else rng.normal(0, 1, 20)
    below, above, ghat = _fit(dist, args, v, rng.rand(20))
    r = IO.importance(dist, args, below, above, ghat)
    assert abs(r['mass'] - 1.0) < 1e-6 and 0 < r['D'] <= 1 / ghat - 1
    assert IO.importance(dist, args, below, above, 1.0)['D'] == 0.0
    assert IO.importance(dist, args, above, above, ghat)['D'] == 0.0      # l == g


def test_lattice_stride():
    mix = O.parzen_fit(np.array([10.0, 500.0]), 1.0, 500.0, 1000.0)
    x, w, s = IO.nodes('quniform', (0, 1000, 1), mix, mix, 64)
    assert s == 16 and x.size == 63 and (w == 16).all()          # 1001 values
    np.testing.assert_array_equal(x, 16.0 * np.arange(63))
    assert IO.nodes('quniform', (0, 10, 3), mix, mix, 64)[0].tolist() == [0.0, 3.0, 6.0, 9.0]
