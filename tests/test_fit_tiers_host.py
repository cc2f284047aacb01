"""Where test_gpu_fit_tiers.py's cases sit among k_fit's tiers, from the
oracle's split alone (no engine): if the space, an N or a cap of
fit_tier_cases.py changes, this shows which tier dropped out."""
import numpy as np

from oracle import tpe_oracle as O
import fit_tier_cases as FC

BINS = (('[1, 64]', 1, 64), ('(64, 1024]', 65, FC.K_MERGE_MAX),
        ('(1024, 4096]', FC.K_MERGE_MAX + 1, FC.K_MIX_M),
        ('(4096, 10000]', FC.K_MIX_M + 1, FC.K_SORT_CAP), ('> 10000', FC.K_SORT_CAP + 1, 1 << 30))


def _sides():
    """(case, label, side, m) of every (hp, side) of every case."""
    out = []
    for c in FC.CASES:
        for lab, ms in FC.side_sizes(c).items():
            out += [(c, lab, side, m) for side, m in enumerate(ms)]
    return out


def _show(sides, k=2):
    return [(FC.case_id(c), lab, ('below', 'above')[side], m) for c, lab, side, m in sides[:k]]


def test_the_cases_sit_on_the_edges():
    hps, labels = FC.specs()
    assert set(FC.ROOT) == {lab for lab in labels if not hps[lab]['conds']}
    sides = _sides()
    upper = {lab: (int(h['args'][0]) if h['dist'] == 'randint' else len(h['args'][0]))
             for lab, h in hps.items() if h['dist'] in ('randint', 'categorical')}
    assert sorted(upper) == ['act0', 'act1', 'act2', 'pk', 'r300', 'top']

    # every tier of m; the three large ones behind a chunked gather (N > kPreN)
    # on a sparse side
    for name, lo, hi in BINS:
        hit = [s for s in sides if lo <= s[3] <= hi]
        print('m in %s: %d (hp, side) pairs, e.g. %s' % (name, len(hit), _show(hit)))
        assert hit, name
        if lo > FC.K_MERGE_MAX:
            far = [s for s in hit if s[0][0] > FC.K_PRE_N and s[1] not in FC.ROOT]
            print('  of them on a branch hp with N > %d: %d, e.g. %s'
                  % (FC.K_PRE_N, len(far), _show(far)))
            assert far, name

    # the mixture's LDS edge (K = m + 1 <= kMixLds) on a root below side, and
    # every N edge as a pair
    root_below = {(c[0], m) for c, lab, side, m in sides if lab == 'aa' and side == 0}
    for m in (FC.K_MIX_M, FC.K_MIX_M + 1):
        assert any(mm == m and n > FC.K_PRE_N for n, mm in root_below), m
        assert any(mm == m and FC.K_SORT_CAP < n <= FC.K_PRE_N for n, mm in root_below), m
    ns = {c[0] for c in FC.CASES}
    for edge in (FC.K_MERGE_MAX, FC.K_SORT_CAP, FC.K_PRE_N):
        assert {edge, edge + 1} <= ns, edge
    assert {b for _, b in FC.GROWTH} <= ns and FC.LAUNCH_N in ns
    for a, b in FC.GROWTH:
        assert a < b - 1 and any(a <= e < b for e in (FC.K_MERGE_MAX, FC.K_SORT_CAP, FC.K_PRE_N))

    # the categorical paths: counted (upper <= 64, kMergeMax < m <= kSortCap),
    # sorted in global memory (upper > 64, m > kSortCap)
    counted = [(FC.case_id(c), lab, m) for c, lab, _, m in sides
               if lab in upper and upper[lab] <= 64 and FC.K_MERGE_MAX < m <= FC.K_SORT_CAP]
    wide = [(FC.case_id(c), lab, m) for c, lab, _, m in sides
            if lab in upper and upper[lab] > 64 and m > FC.K_SORT_CAP]
    print('counted categoricals: %d, e.g. %s; sorted past kSortCap: %d, e.g. %s'
          % (len(counted), counted[:2], len(wide), wide[:2]))
    assert counted and wide
    # (and a few-bin categorical just past the counting path: sorted)
    assert any(lab == 'top' and m == FC.K_SORT_CAP + 1 for c, lab, _, m in sides)

    # every tied column: trials on both sides carry the threshold loss
    tied = [c for c in FC.CASES if c[5] == 'tied']
    assert len(tied) >= 14
    for c in tied:
        l, below = FC.case_losses(c), FC.below_mask(c)
        nb = O.n_below_count(c[0], c[1], c[2])
        assert below.sum() == nb
        thr = np.sort(l)[nb - 1]
        at = l == thr
        assert np.isinf(l).sum() == 5 and np.isnan(l).sum() == 2
        assert (at & below).sum() >= 1 and (at & ~below).sum() >= 1, FC.case_id(c)
        assert at.sum() >= FC.N_TIED
        # (by position: the below ones come first)
        assert np.flatnonzero(at & below).max() < np.flatnonzero(at & ~below).min()
        # tied trials in the first and the last 1024 rows and in every chunk
        rows = np.flatnonzero(at)
        assert (rows < 1024).any() and (rows >= c[0] - 1024).any()
        for a in range(0, c[0], FC.K_PRE_N):
            assert ((rows >= a) & (rows < a + FC.K_PRE_N)).any(), (FC.case_id(c), a)
    # the case without a threshold: every trial below
    full = [c for c in FC.CASES if O.n_below_count(*c[:3]) >= c[0]]
    assert [c[:3] for c in full] == [(10001, 100.0, 10001)] and FC.below_mask(full[0]).all()


def test_the_history_is_a_prior_sample():
    """The columns are what the issue of the tiers asks for: branch hps active
    in about a third of the rows, values inside their priors' supports, the
    quantized ones heavily tied."""
    hps, labels = FC.specs()
    vals, active, _ = FC.history(31000)
    top = vals[labels.index('top')]
    for i, lab in enumerate(labels):
        on = active[i] == 1
        if lab in FC.ROOT:
            assert on.all()
        else:
            np.testing.assert_array_equal(on, top == hps[lab]['conds'][0][1])
            assert 0.3 < on.mean() < 0.37
        assert np.isfinite(vals[i]).all()
    assert np.unique(vals[labels.index('qu')]).size == 101
    assert np.unique(vals[labels.index('r300')]).size == 300
    assert set(np.unique(vals[labels.index('pk')])) == {0.0, 1.0, 2.0}
