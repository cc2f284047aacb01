"""The lean gather between the table pass and the direct pass (DESIGN 5.10;
k_tie_gather_lean: each wave counts the hot entries of its own span of whole
64-entry rows, one scan over the 16 totals, a second sweep writes the list)
against k_tie_gather, which the same library keeps behind TPE_TABLE_LEAN=0 (a
child interpreter: the switch is read once per process).

Compared: Plan.tie_list entry for entry, the tie counts, every tab_wmax word
(tab_max is their maximum, a NaN first: derived here, and the list is checked
against the gather's predicate on it) and the records.  Shape:
test_gpu_table.py's, 2120 list entries per slot of which 2113 hold candidates
-- 33 rows of 64 and one of 8, over 16 waves: spans of 3 rows, the twelfth
wave's ending in the partial row and the last four waves with none.

Cases: the shape; TPE_TABLE_TIE_LOG2=2000 (every tile hot: the list is 0 ..
2112 in order); TPE_TABLE_TIE_LOG2=-1074 (the single best wave, or little
more); TPE_DRAW_PRUNE=0 (no dropped tiles: tab_pref 1); the --gap history
(u takes the every-tile branch, unchanged); the conditional space (inactive
hps).
"""
import numpy as np
import pytest

import test_gpu_table_build_lean as B
import test_gpu_tie_gather as G

pytestmark = pytest.mark.gpu

CASES = [('plain', 'shape', B.LABELS), ('wide', 'shape', B.LABELS), ('narrow', 'shape', B.LABELS),
         ('noprune', 'shape', B.LABELS), ('plain', 'gap', B.LABELS),
         ('plain', 'cond', ('u', 'a', 'b'))]
TIE = {'plain': 2.0 ** -16, 'noprune': 2.0 ** -16, 'narrow': 2.0 ** -1074}


def _expected(w, tie, dropped):
    """k_tie_gather's list of a certified slot from its wave scores."""
    rec = w[:B.NWT]
    tm = np.nan if np.isnan(rec).any() else rec.max()
    with np.errstate(invalid='ignore', over='ignore'):
        thr = tm - tie * max(1.0, abs(tm))
        hot = ~(w < thr)
    if dropped:
        hot[:B.NWT] &= rec != -np.inf
    return np.flatnonzero(hot)


@pytest.mark.parametrize('env,case,labels', CASES, ids=['%s-%s' % c[:2] for c in CASES])
def test_gather_lists(env, case, labels):
    on, off = B.pair(env)
    on, off = on[case], off[case]
    assert on['labels'] == off['labels']
    assert on['hex'] == off['hex']
    assert on['counts'] == off['counts']
    cnt = np.asarray(on['counts'])
    n_sug = cnt.shape[0]
    for lab in labels:
        col = on['labels'].index(lab)
        assert on['wmax_' + lab] == off['wmax_' + lab]
        wm = B.unhex(on['wmax_' + lab], np.float64).reshape(n_sug, -1)
        for s in range(n_sug):
            a = B.unhex(on['list_' + lab][s], np.int32)
            b = B.unhex(off['list_' + lab][s], np.int32)
            np.testing.assert_array_equal(a, b)
            assert a.size == max(0, cnt[s, col])
            certified = not (case == 'gap' and lab == 'u') and case != 'cond'
            if env == 'wide' and certified:
                np.testing.assert_array_equal(a, np.arange(G.WAVE_TILES))
            elif certified:
                # the slot's waves past the candidates hold NaN: hot, as in the kernel
                w = wm[s, :G.WAVE_TILES]
                np.testing.assert_array_equal(a, _expected(w, TIE[env], env != 'noprune'))
        print(env, case, lab, 'list lengths:', cnt[:, col].tolist())
    if env == 'narrow':
        assert (cnt[:, [on['labels'].index(l) for l in labels]] <= 4 + G.WAVE_TILES - B.NWT).all()
    if case == 'gap':
        assert (cnt[:, on['labels'].index('u')] == G.WAVE_TILES).all()
    if case == 'cond':
        assert (cnt == 0).any() and (cnt > 0).any()
