"""The plan's fit (k_fit: split, gather in tid order, sort, Parzen or
categorical fit, scoring tables) across its history-size tiers, against the
oracle -- histories of up to 31 000 trials with a real split behind every side.

k_fit picks its code from N (kMergeMax = 1024: the all-LDS kernel; kSortCap =
10000: the split's loss keys in LDS or in global memory, where the observation
keys overwrite them afterwards; kPreN = 12288: one prefetched gather or a loop
of 12288-row chunks whose count accumulates) and from m, the observations of
one hp on one side (64, kMergeMax, 4096 = kMixLds - 1, kSortCap).  The
operator-level fits (test_gpu_ops.py) have N == m, no split and full ballots;
here the branch hps of spaces.fit_tiers_space are active in a third of the
rows, and the `tied` loss columns put trials with the threshold loss on both
sides of every split.  fit_tier_cases.py builds the histories and lists the
cases; test_fit_tiers_host.py shows, without a device, which tier each covers.

Per case, for every hp and both sides: K and the mixture (w, mu, sigma)
against the oracle's fit of the oracle's split, bit for bit (the log families
through fit_oracle.assert_mixture_bit_exact); the categorical posteriors bit
for bit.  The scoring tables of the same kernel through score_points within
the project's 1e-6 term bound.  Histories grown across an N edge by a deferred
update equal fresh plans byte for byte, and fit_suggest equals fit + suggest
past kPreN.

Measured on an MI355X: every case passes -- no fault found in tpe_fit.hip; the
table terms reach 0.054 of their bound; the module takes 4.7 s, its slowest
test (the table oracle at K = 31 000) 1.3 s.
"""
import functools

import numpy as np
import pytest

from hyperopt_amd import hp, _engine as E
from hyperopt_amd.base import Domain

from oracle import tpe_oracle as O
from fit_oracle import assert_mixture_bit_exact
import fit_tier_cases as FC
import spaces
import test_gpu_points as P

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _dom():
    dom = Domain(lambda x: 0.0, spaces.fit_tiers_space(hp))
    assert dom.space.labels == list(FC.specs()[1])
    return dom


def _new_plan(n_max, losses, vals, active):
    hps, conds, pprior = _dom().space.engine_tables()
    plan = E.Plan(E.default_engine(), hps, conds, pprior, max_trials=n_max)
    plan.set_history(np.ascontiguousarray(losses), np.ascontiguousarray(vals),
                     np.ascontiguousarray(active))
    return plan


def _fitted(c):
    n, gamma, cap, pw, lf, _ = c
    vals, active, _ = FC.history(n)
    plan = _new_plan(n, FC.case_losses(c), vals, active)
    plan.fit(gamma=gamma, prior_weight=pw, lf=lf, gamma_cap=cap)
    return plan


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_mixtures(a, b, msg):
    for i in range(a.n_hp):
        for side in (0, 1):
            for x, y, what in zip(a.mixture(i, side), b.mixture(i, side), ('w', 'mu', 'sigma')):
                np.testing.assert_array_equal(_bits(x), _bits(y),
                                              err_msg='%s hp %d side %d %s' % (msg, i, side, what))


@pytest.mark.parametrize('c', FC.CASES, ids=FC.case_id)
def test_fit_matches_oracle(c):
    n, gamma, cap, pw, lf, _ = c
    hps, labels = FC.specs()
    vals, active, _ = FC.history(n)
    losses = FC.case_losses(c)
    plan = _fitted(c)
    tids = np.arange(n)
    sizes = FC.side_sizes(c)
    for i, lab in enumerate(labels):
        h = hps[lab]
        on = active[i] == 1
        sides = O.split_observations(tids[on], vals[i][on], tids, losses, gamma, cap,
                                     kind='stable')
        assert (sides[0].size, sides[1].size) == sizes[lab]
        for side, obs in enumerate(sides):
            msg = '%s %s side %d (m = %d) ' % (FC.case_id(c), lab, side, obs.size)
            w, mu, sg = plan.mixture(i, side)
            if h['dist'] in ('randint', 'categorical'):
                pp = None if h['dist'] == 'randint' else np.asarray(h['args'][0])
                upper = int(h['args'][0]) if pp is None else pp.size
                assert w.size == upper, msg
                np.testing.assert_array_equal(
                    w, O.categorical_posterior(obs, upper, pw, pp, lf=lf), err_msg=msg)
                continue
            assert w.size == obs.size + 1, msg + 'K = %d' % w.size
            with np.errstate(all='ignore'):
                fk, pm, ps, low, high, q, tr = O.posterior_spec(h['dist'], h['args'], pw)
                tobs = O.transform_obs(obs, tr, low)
            assert_mixture_bit_exact((w, mu, sg), tobs, pw, pm, ps, lf, fk == 'lgmm', msg)


@pytest.mark.parametrize('c', FC.TABLE_CASES, ids=FC.case_id)
def test_scoring_tables_match_oracle(c):
    """The tables prep_slot / store_table write at the end of the same kernel:
    256 prior configurations (branch values included) scored through
    score_points, every term within test_gpu_points' bound of the oracle's."""
    n, gamma, cap, pw, lf, _ = c
    assert (pw, lf) == (P.PRIOR_WEIGHT, O.DEFAULT_LF)
    cs = _dom().space
    vals, active, _ = FC.history(n)
    pts, pact = FC.columns(256, 77)
    assert all(pact[i].any() and pact[i].sum() < 256 for i, lab in enumerate(cs.labels)
               if lab not in FC.ROOT)
    lb, la = P._oracle_lliks(cs, FC.case_losses(c), vals, active, pts, pact, gamma=gamma,
                             gamma_cap=cap)
    total, terms, act = _fitted(c).score_points(pts, want_terms=True, want_active=True)
    P._check_against_oracle(total, terms, act, lb, la, pact, FC.case_id(c))


@pytest.mark.parametrize('a,b', FC.GROWTH)
def test_growth_across_an_edge(a, b):
    """A plan fitted on the first a trials (the kernel or tier under the edge),
    then given the last two rows as a deferred update (k_fit writes them
    itself) and fitted again: every mixture byte for byte that of a fresh plan
    given all b trials at once."""
    c = (b,) + FC.DEFAULT + ('tied',)
    vals, active, _ = FC.history(b)
    losses = FC.case_losses(c)
    part = _new_plan(b, losses[:a], vals[:, :a], active[:, :a])
    part.fit()
    assert part.mixture(_dom().space.labels.index('aa'), 1)[0].size \
        == a - O.n_below_count(a, 0.25) + 1
    part.update_history(b, a, vals, active, b, a, losses)
    part.fit()
    _same_mixtures(part, _fitted(c), '%d -> %d' % (a, b))


def test_fit_suggest_equals_fit_then_suggest_past_the_prefetch():
    """fit_suggest (the engine's one-call launch shape) at N = 12289 > kPreN
    against fit() + suggest() on a second plan, byte for byte."""
    c = (FC.LAUNCH_N,) + FC.DEFAULT + ('tied',)
    vals, active, _ = FC.history(FC.LAUNCH_N)
    one = _new_plan(FC.LAUNCH_N, FC.case_losses(c), vals, active)
    got = one.fit_suggest([11, 12], 4096)
    two = _fitted(c)
    want = two.suggest([11, 12], 4096)
    assert got['active'].any() and np.isfinite(got['value'][got['active'] == 1]).all()
    np.testing.assert_array_equal(got.view(np.uint8), want.view(np.uint8))
    _same_mixtures(one, two, 'fit_suggest')
