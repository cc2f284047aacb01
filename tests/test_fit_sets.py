"""The numpy emulation of the table path (tools/table_error.py)
away from the default fit: every named set of fit parameters (FIT_SETS: gamma,
gamma_cap, prior_weight, lf) on the history of test_gpu_table.py (N = 6000),
for both bounded hps.

Per (set, hp): the split and mixture sizes the set names; both tables exist
with every panel certified (prior_weight 0 leaves a -inf coefficient on the
widest component; one observation or none below leaves a below table of one or
two panels); and on 2^18 draws of the below mixture (RandomState 7) the
prefilter prunes no wave tile whose best score reaches k_tie_gather's
threshold, the pruning draw drops none, and it keeps some wave tiles but not
all.  tests/test_gpu_fit_params.py runs the same sets on the device.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import table_error as TE  # noqa: E402
from oracle import tpe_oracle as O  # noqa: E402

DRAWS = 1 << 18
N = 6000
# panels of the below table (the above table has 50 throughout)
BELOW_PANELS = {'default': 11, 'wide-below': 40, 'huge-below': 50, 'over-cap': 50, 'few-below': 2,
                'prior-only': 1, 'pw-small': 11, 'pw-big': 11, 'pw-zero': 11, 'lf-off': 11,
                'lf-long': 40}


def test_the_sets_are_the_eleven():
    assert sorted(TE.FIT_SETS) == sorted(BELOW_PANELS)
    for name, s in TE.FIT_SETS.items():
        assert s['n_below'] == O.n_below_count(N, s['gamma'], s['gamma_cap']), name
        assert s['K_below'] == s['n_below'] + 1 and s['K_above'] == N - s['n_below'] + 1, name
    K = {n: (s['n_below'], s['K_below'], s['K_above']) for n, s in TE.FIT_SETS.items()}
    assert K == {'default': (20, 21, 5981), 'wide-below': (78, 79, 5923),
                 'huge-below': (1240, 1241, 4761), 'over-cap': (2479, 2480, 3522),
                 'few-below': (2, 3, 5999), 'prior-only': (0, 1, 6001), 'pw-small': (20, 21, 5981),
                 'pw-big': (20, 21, 5981), 'pw-zero': (20, 21, 5981), 'lf-off': (20, 21, 5981),
                 'lf-long': (78, 79, 5923)}


@pytest.mark.parametrize('lab', ['u', 'lu'])
@pytest.mark.parametrize('name', sorted(BELOW_PANELS))
def test_fit_set_emulation(name, lab):
    s = TE.FIT_SETS[name]
    fit = TE.fit_params(name)
    losses, cols, specs = TE.test_shape(N)
    dist, args = specs[lab]
    (mb, ma), _ = TE.mixtures(losses, cols, lab, dist, args, **fit)
    assert (mb[0].size, ma[0].size) == (s['K_below'], s['K_above'])
    assert mb[0].size + ma[0].size == N + 2
    if s['prior_weight'] == 0.0:       # the -inf coefficient is there, once per side
        assert (mb[0] == 0.0).sum() == 1 and (ma[0] == 0.0).sum() == 1
    pair = TE.certified_pair(losses, cols, lab, dist, args, **fit)
    assert pair is not None, 'a table is missing or a panel not certified'
    tb, ta, (w, mu, sg), (low, high, pm) = pair
    assert tb['ok'].all() and ta['ok'].all()
    assert (tb['P'], ta['P']) == (BELOW_PANELS[name], 50)
    worst = max(float((t['log2_err'] - t['log2_glb']).max()) for t in (tb, ta))
    assert worst <= TE.BAR
    y = TE.draw_below(w, mu, sg, low, high, pm, DRAWS, np.random.RandomState(7))
    with np.errstate(all='ignore'):
        r = TE.draw_prune(tb, ta, y)       # (prefilter()'s result and the draw's on top)
    assert np.isfinite(r['wmax']).all() and np.isfinite(r['U']).all()
    hot = ~(r['wmax'] < r['thr'])
    missed = int((r['pruned'] & hot).sum())
    print('%s %s: K %d / %d, panels %d / %d, worst log2 err - glb %.1f, wave tiles passing %.4f, '
          'kept %.4f, hot %d, missed %d, dropped %d'
          % (name, lab, mb[0].size, ma[0].size, tb['P'], ta['P'], worst, (~r['pruned']).mean(),
             r['kept'].mean(), int(hot.sum()), missed, r['dropped_hot']))
    assert hot.any() and missed == 0
    assert r['dropped_hot'] == 0
    assert 0.0 < r['kept'].mean() < 1.0
