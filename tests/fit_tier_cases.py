"""Histories and cases of the plan-level fit tests across the history-size
tiers of tpe_fit.hip (test_gpu_fit_tiers.py on the device, test_fit_tiers_host.py
for where the cases sit).  Numpy and the oracle only: importable without the
engine.

k_fit picks its code from N, the history length (kMergeMax = 1024: the
all-LDS kernel; kSortCap = 10000: the split's loss keys in LDS or in global
memory; kPreN = 12288: one prefetched gather or a loop of chunks), and from m,
the observations of one hp on one side (64, kMergeMax, kMixLds - 1 = 4096,
kSortCap: the sorts and where the mixture lives).

The space is spaces.fit_tiers_space.  The columns are built directly: ``top``
from RandomState(N), then every other hp's prior draws in label order from the
same stream; a branch hp is active where ``top`` picks its branch (about a
third of the rows: the sparse sides), a root hp everywhere.
"""
import functools

import numpy as np

from oracle import tpe_oracle as O
import spaces

K_MERGE_MAX, K_MIX_M, K_SORT_CAP, K_PRE_N = 1024, 4096, 10000, 12288
DEFAULT = (0.25, 25, 1.0, 25)          # gamma, gamma_cap, prior_weight, lf
N_TIED = 40                            # rows given the threshold loss
EDGE_NS = (1024, 1025, 10000, 10001, 12288, 12289, 31000)
ROOT = ('aa', 'pk', 'qn', 'qu', 'r300', 'top')


def _cases():
    out = []
    for n in EDGE_NS:
        for col in ('distinct', 'tied'):
            out.append((n,) + DEFAULT + (col,))
    for n in (10001, 31000):
        for cap in (1100, 4096, 4097, 10001):
            # (10001 trials, cap 10001: n_below = N, every trial is below and
            # no loss is a threshold -- the distinct losses)
            out.append((n, 100.0, cap, 1.0, 25, 'tied' if cap < n else 'distinct'))
    out.append((12289, 0.25, 25, 0.5, 100, 'tied'))
    return tuple(out)


# (N, gamma, gamma_cap, prior_weight, lf, loss column)
CASES = _cases()
TABLE_CASES = ((31000,) + DEFAULT + ('distinct',), (31000, 100.0, 10001, 1.0, 25, 'tied'))
GROWTH = ((1023, 1025), (9999, 10001), (12287, 12289))
LAUNCH_N = 12289


def case_id(c):
    return 'N%d-g%g-cap%d-pw%g-lf%d-%s' % c


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def specs():
    """label -> dict(dist, args, conds) of the space, and the sorted labels."""
    hps = spaces.describe(spaces.fit_tiers_space(spaces.RecordingHP()))
    return hps, tuple(sorted(hps))


def columns(n, seed):
    """(vals[P, n], active[P, n] uint8) of n prior configurations."""
    hps, labels = specs()
    rs = np.random.RandomState(seed)
    top = rs.randint(3, size=n)
    vals = np.zeros((len(labels), n))
    active = np.ones((len(labels), n), dtype=np.uint8)
    for i, lab in enumerate(labels):
        h = hps[lab]
        if lab == 'top':
            vals[i] = top
            continue
        vals[i] = O.prior_sample(rs, h['dist'], h['args'], n)
        for parent, b in h['conds']:
            assert parent == 'top'
            active[i] = top == b
    return vals, active


@functools.lru_cache(maxsize=None)
def history(n):
    """(vals[P, n], active[P, n], distinct losses[n]) of the n-trial history."""
    vals, active = columns(n, n)
    return _frozen(vals, active, np.random.RandomState(n + 1).rand(n))


@functools.lru_cache(maxsize=None)
def losses(n, col, n_below):
    """The loss column of a case.  ``tied``: rounded to three digits, five
    rows +inf and two NaN (pending and failed trials), and N_TIED rows above
    the threshold given the loss of rank n_below -- some in the first and the
    last 1024 rows and in every 12288-row chunk -- so that trials on both
    sides of the split carry the threshold loss and the position decides."""
    if col == 'distinct':
        return history(n)[2]
    assert col == 'tied' and 0 < n_below < n
    rs = np.random.RandomState(n + 2)
    l = np.round(rs.rand(n), 3)
    l[rs.randint(n, size=5)] = np.inf
    l[rs.randint(n, size=2)] = np.nan
    thr = np.sort(l)[n_below - 1]
    assert np.isfinite(thr)
    free = np.isfinite(l) & (l > thr)          # (raising no rank under n_below)
    spans = [(0, min(n, 1024)), (max(0, n - 1024), n)]
    spans += [(a, min(n, a + K_PRE_N)) for a in range(0, n, K_PRE_N)]
    rows = set()
    for a, b in spans:
        cand = a + np.flatnonzero(free[a:b])
        assert cand.size, (n, a, b)            # (N = 12289: the last chunk is one row)
        rows.update(rs.choice(cand, min(6, cand.size), replace=False).tolist())
    rest = np.setdiff1d(np.flatnonzero(free), sorted(rows))
    rows.update(rs.choice(rest, N_TIED - len(rows), replace=False).tolist())
    l[sorted(rows)] = thr
    return _frozen(l)[0]


def case_losses(c):
    n, gamma, cap = c[:3]
    return losses(n, c[5], O.n_below_count(n, gamma, cap))


@functools.lru_cache(maxsize=None)
def below_mask(c):
    """bool[N]: the oracle's below trials of a case (stable ties)."""
    n, gamma, cap = c[:3]
    good, _ = O.below_tids(np.arange(n), case_losses(c), gamma, cap, kind='stable')
    mask = np.zeros(n, dtype=bool)
    mask[sorted(good)] = True
    return _frozen(mask)[0]


def side_sizes(c):
    """label -> (m below, m above) from the oracle's split alone."""
    _, labels = specs()
    _, active, _ = history(c[0])
    below = below_mask(c)
    return {lab: (int((active[i] == 1)[below].sum()), int((active[i] == 1)[~below].sum()))
            for i, lab in enumerate(labels)}
