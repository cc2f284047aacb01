"""The lean map behind the pruning draw (k_table_map_dp_lean: the
block's live wave tiles through one list in LDS, dealt round-robin to the eight
waves, each wave loading its next tile's candidates ahead) against
k_table_map_dp, which the same library keeps behind TPE_TABLE_LEAN=0 (a child
interpreter: the switch is read once per process).

Every entry of Plan.tab_wmax is compared as a 64-bit word -- -inf (a dropped
or prefiltered tile), NaN (a tile past the candidates) and scores alike -- and
with it the records and the tie counts.  Shape: test_gpu_table.py's N = 6000 and
2^18 + 8192 + 37 candidates on u, lu: 2113 wave tiles, so four full 512-tile
blocks and one of 65 per slot, the last tile partial.

Cases: the shape as it is (measured: 43 to 49 live tiles per slot, up to a few
dozen in a block and none in the last, partial one of some slots); the same
with TPE_TABLE_TIE_LOG2=2000 in both processes (nothing is pruned: every tile of
every block is live, a wave's share of the list is 64); the low-edge history
(the hot interval sits on a bound); the conditional space of
test_gpu_tie_gather.py (inactive hps: the block-uniform return ahead of the
barriers); the census on (the same pairs credited).
"""
import numpy as np
import pytest

import test_gpu_table_build_lean as B

pytestmark = pytest.mark.gpu

NEG_INF = np.array([-np.inf]).view(np.uint64)[0]
CASES = [('plain', 'shape', B.LABELS), ('wide', 'shape', B.LABELS), ('plain', 'low_edge', ('e',)),
         ('plain', 'cond', ('u', 'a', 'b')), ('plain', 'census', B.LABELS)]


@pytest.mark.parametrize('env,case,labels', CASES, ids=['%s-%s' % c[:2] for c in CASES])
def test_map_bytes(env, case, labels):
    on, off = B.pair(env)
    on, off = on[case], off[case]
    assert on['labels'] == off['labels'] and on['width'] == off['width'] >= B.NWT
    assert on['hex'] == off['hex']
    assert on['counts'] == off['counts']
    n_sug = len(on['counts'])
    for lab in labels:
        a = B.unhex(on['wmax_' + lab], np.uint64).reshape(n_sug, -1)
        b = B.unhex(off['wmax_' + lab], np.uint64).reshape(n_sug, -1)
        live = a[:, :B.NWT] != NEG_INF
        blocks = np.stack([live[:, i:i + 512].sum(axis=1) for i in range(0, B.NWT, 512)], axis=1)
        print(env, case, lab, 'entries differing:', int((a != b).sum()), 'of', a.size,
              'live tiles per 512-tile block, first suggestion:', blocks[0].tolist())
        np.testing.assert_array_equal(a, b)
        if case in ('shape', 'census', 'low_edge'):
            # the tables are in play, and the map has work of the intended kind
            if env == 'wide':
                assert live.all()                      # every block full, the last one 65
            else:
                assert live.any() and not live.all()
                assert (blocks.max(axis=1) < 512).all()   # no block is all live
    if case == 'census':
        assert on['census'] == off['census'] and on['census'][3] > 0
    if case == 'cond':
        cnt = np.asarray(on['counts'])
        assert (cnt == 0).any() and (cnt > 0).any()    # inactive and active slots
