"""Host side of the pending batch's edge tests (no GPU): the proof
that ``test_gpu_batch_edges.py`` can fail.  On ``batch_edge_cases``' fixtures
the closed-form sigma is ``parzen_fit``'s bit for bit, the crafted picks reach
every edge of the sigma search, and each wrong rule of the update -- a mutant
of ``batch_edge_cases.replay`` -- moves some trace entry by more than 4x the
bound the GPU test holds the device to (the factor of
``test_batch_host.test_every_gpu_round_is_decided``)."""
import numpy as np
import pytest

from hyperopt_amd import _engine as E

import batch_edge_cases as X
import batch_oracle as B

FACTOR = 4.0
ONE_HP = [(kind, n) for kind in X.KINDS for n in X.SIZES]
# the upper clip cannot act on a bounded quantized kind: every value the kernel
# accepts lies in [low, high], the prior's mu is their midpoint and prior_sigma
# their distance, so no gap exceeds prior_sigma
# (test_the_upper_clip_is_out_of_reach_of_a_bounded_quantized_kind)
OUT_OF_REACH = {('ceiling', 'quniform'), ('ceiling', 'qloguniform'),
                ('no upper clip', 'quniform'), ('no upper clip', 'qloguniform')}
CLASSES = ('lo=0', 'lo=K', 'tie', 'floor 2+K', 'floor 100', 'ceiling', 'K=1')


# ------------------------------------------------------------- the fixtures
@pytest.mark.parametrize('kind', list(X.KINDS))
def test_the_above_mixtures_span_the_tiers_of_the_sigma_floor(kind):
    """K = 1 (the prior alone), K = 2, one K with divisor 2 + K and one with
    the divisor capped at 100."""
    Ks = [X.model(kind, n).w[0][1].size for n in X.SIZES]
    print(kind, 'K =', Ks)
    assert Ks[0] == 1 and Ks[1] == 2 and 3 <= Ks[2] <= 97 and Ks[3] >= 98
    if kind not in X.CATEGORICAL:
        assert [X.above_mus(kind, n).size for n in X.SIZES] == Ks


@pytest.mark.parametrize('kind, n', ONE_HP)
def test_case_layout(kind, n):
    """The picks lead and are alone eligible; the audience repeats them and
    holds two values the kind rejects, NaN in every round."""
    c = X.case(kind, n)
    p = np.array(X.picks(kind, n))
    assert c.k == p.size <= X.MAX_LATTICE and c.k <= E.BATCH_MAX
    assert c.eligible[:c.k].all() and not c.eligible[c.k:].any()
    np.testing.assert_array_equal(c.vals[0, :c.k], p)
    np.testing.assert_array_equal(c.vals[0, c.k:2 * c.k], p)
    res = X.oracle_run(c)
    assert sorted(res.picks.tolist()) == list(range(c.k))
    nan = np.isnan(res.scores)
    assert (nan == nan[0]).all()            # (a score never turns NaN in a later round)
    if kind in X.LOG_KINDS or kind in X.CATEGORICAL:
        assert nan[0, -2:].all()
    if kind in ('qlognormal', 'qloguniform'):
        assert 0.0 in p                     # the observation transform's floor
    if kind in X.QUANTIZED:
        q = X.spec(kind)[5]
        np.testing.assert_array_equal(np.round(p / q) * q, p)


def test_two_branch_picks_alternate_branches():
    c = X.two_branch_case()
    assert c.model.groups == [[0], [1], [2]] and c.vals.shape == (3, 6 + X.TWO_BRANCH_AUDIENCE)
    t = c.vals[0]
    assert list(t[:6]) == [0, 1, 0, 1, 0, 1]
    res = X.oracle_run(c)
    assert (np.diff(t[res.picks]) != 0).all(), t[res.picks]
    assert (res.ratio > FACTOR).all()


def test_every_many_dists_round_is_decided():
    """``test_batch_host.test_every_gpu_round_is_decided``'s criterion."""
    c = X.many_dists_case()
    assert len(c.model.groups) == 1 and len(c.model.groups[0]) == 11
    res = X.oracle_run(c)
    print('many_dists m=%d k=%d: min margin / bound = %.3g' % (X.MANY_M, X.MANY_K, res.ratio.min()))
    assert np.isfinite(res.scores[np.arange(c.k), res.picks]).all()
    assert (res.ratio > FACTOR).all(), res.ratio
    assert len(set(res.picks.tolist())) == c.k


def test_the_launch_shape_cases():
    """More than 256 blocks with the best eligible configuration in the last
    one and every round decided; BATCH_MAX distinct configurations."""
    c = X.slot_case()
    assert (X.SLOT_M + X.BLOCK - 1) // X.BLOCK > X.BLOCK and X.SLOT_BEST // X.BLOCK == 257
    blocks = np.flatnonzero(c.eligible) // X.BLOCK
    assert [int((blocks == b).sum()) for b in (0, 256, 257)] == [2, 5, 5]
    res = X.oracle_run(c)
    assert res.picks[0] == X.SLOT_BEST and (res.ratio > FACTOR).all()
    c = X.kmax_case(E.BATCH_MAX)
    assert np.unique(c.vals[0]).size == X.KMAX_M > E.BATCH_MAX == c.k


# ----------------------------------------------------------- the closed form
@pytest.mark.parametrize('kind, n', [(k, n) for k, n in ONE_HP if k not in X.CATEGORICAL])
def test_closed_form_sigma_of_every_crafted_pick(kind, n):
    d = X.model(kind, n).dims[0][1][0]
    _, pm, ps = X.spec(kind)[:3]
    mus = X.above_mus(kind, n)
    for v, mu in zip(X.picks(kind, n), X.transform(kind, X.picks(kind, n))):
        want = B.pending_sigma(d.obs, mu, X.PRIOR_WEIGHT, pm, ps)
        assert B.pending_sigma_closed(mus, mu, ps) == want, (kind, n, v)
        assert X.rule_sigma(mus, mu, ps) == want, (kind, n, v)


@pytest.mark.parametrize('kind', X.CONTINUOUS + X.QUANTIZED)
def test_crafted_picks_reach_every_edge_of_the_sigma_search(kind):
    ps = X.spec(kind)[2]
    count = dict.fromkeys(CLASSES, 0)
    for n in X.SIZES:
        for mu in X.transform(kind, X.picks(kind, n)):
            for cls in X.sigma_class(X.above_mus(kind, n), mu, ps):
                count[cls] += 1
    print(kind, count)
    for cls in CLASSES:
        assert (count[cls] == 0) == ((cls, kind) in OUT_OF_REACH), (kind, cls, count)


@pytest.mark.parametrize('kind', ['quniform', 'qloguniform'])
def test_the_upper_clip_is_out_of_reach_of_a_bounded_quantized_kind(kind):
    """Why OUT_OF_REACH holds: the transformed values span [low, high], the
    prior's mu -- always in the mixture -- is their midpoint and prior_sigma is
    high - low, so a one-sided gap is at most prior_sigma / 2 and a two-sided
    one below prior_sigma.  A value off that range has no kernel at all."""
    _, pm, ps, low, high, q, _ = X.spec(kind)
    assert ps == high - low and pm == 0.5 * (low + high)
    lattice = np.arange(0.0, np.exp(high) if kind in X.LOG_KINDS else high, q / 8)
    mu = X.transform(kind, lattice)
    assert mu.min() >= low and mu.max() <= high
    for n in X.SIZES:
        mus = X.above_mus(kind, n)
        assert pm in mus and mus.min() >= low and mus.max() <= high
        for v in mu:
            assert 'ceiling' not in X.sigma_class(mus, v, ps)
    # outside: log(cdf(ub) - cdf(lb)) of ub <= lb
    d = X.model(kind, 40).dims[0][1][0]
    top = np.round((np.exp(high) if kind in X.LOG_KINDS else high) / q) * q
    with np.errstate(all='ignore'):
        assert not np.isfinite(d.log_kernel(np.array([top + 2 * q]))).any()


# --------------------------------------------------------------- the mutants
def _moved(case, rules):
    """max over (round, configuration) of |mutant - oracle| / bound, the
    mutant replayed on the oracle's picks."""
    base = X.oracle_run(case)
    got = X.replay(case.model, case.vals, base.picks, rules=X.Rules(**rules))
    with np.errstate(all='ignore'):
        r = np.abs(got.scores - base.scores) / base.bound
        r = np.where(np.isnan(got.scores) != np.isnan(base.scores), np.inf, r)
    return float(np.max(np.where(np.isnan(r), 0.0, r)))


REPLAYED = {'uniform n=40': lambda: X.case('uniform', 40),
            'qlognormal n=140': lambda: X.case('qlognormal', 140),
            'pchoice n=2': lambda: X.case('pchoice', 2), 'two_branch': X.two_branch_case,
            'many_dists': X.many_dists_case, 'slots': X.slot_case,
            'kmax': lambda: X.kmax_case(E.BATCH_MAX)}


@pytest.mark.parametrize('name', list(REPLAYED))
def test_the_replay_under_the_models_rules_is_the_oracle(name):
    case = REPLAYED[name]()
    base = X.oracle_run(case)
    got = X.replay(case.model, case.vals, base.picks)
    np.testing.assert_array_equal(got.scores.view(np.uint64), base.scores.view(np.uint64))


@pytest.mark.parametrize('kind', X.CONTINUOUS + X.QUANTIZED)
@pytest.mark.parametrize('mutant', X.SIGMA_MUTANTS)
def test_a_wrong_sigma_rule_is_caught_on_every_kind(mutant, kind):
    r = [_moved(X.case(kind, n), X.MUTANTS[mutant]) for n in X.SIZES]
    print('%s, %s: worst |d| / bound at n = 1, 2, 40, 140: %s' % (
        mutant, kind, ' '.join('%.3g' % v for v in r)))
    if (mutant, kind) in OUT_OF_REACH:
        assert max(r) == 0.0                # (the rule never acts: nothing to catch)
    else:
        assert max(r) > FACTOR, (mutant, kind, r)


def _applies(mutant):
    one = {'W without n_g': list(X.KINDS), 'categorical hit and miss swapped': X.CATEGORICAL,
           'quantized bounds not clipped': ('quniform', 'qloguniform'),
           'no - log x': ('loguniform', 'lognormal'), 'inactive group updated': ()}[mutant]
    cases = [X.case(kind, n) for kind in one for n in X.SIZES]
    if mutant in ('W without n_g', 'inactive group updated'):
        cases.append(X.two_branch_case())
    return cases


@pytest.mark.parametrize('mutant', [m for m in X.MUTANTS if m not in X.SIGMA_MUTANTS])
def test_a_wrong_update_rule_is_caught(mutant):
    """On every one-hp fixture the rule applies to and on two_branch, not only
    on one of them.  many_dists is printed, not asserted: in its 11-hp group a
    pending component is negligible away from the pick, which is why the
    one-hp fixtures exist."""
    for case in _applies(mutant):
        r = _moved(case, X.MUTANTS[mutant])
        print('%s, %s: worst |d| / bound = %.3g' % (mutant, case.name, r))
        assert r > FACTOR, (mutant, case.name, r)
    if mutant != 'inactive group updated':
        print('%s, many_dists: worst |d| / bound = %.3g' % (
            mutant, _moved(X.many_dists_case(), X.MUTANTS[mutant])))


def test_a_two_percent_sigma_error_is_caught():
    """The bar is tight enough for the kernel's sigma: 1.02 sigma moves some
    entry of every continuous and quantized fixture far past the bound."""
    worst = np.inf
    for kind in X.CONTINUOUS + X.QUANTIZED:
        for n in X.SIZES:
            case = X.case(kind, n)
            base = X.oracle_run(case)
            orig = X.rule_sigma
            try:
                X.rule_sigma = lambda *a, **kw: 1.02 * orig(*a, **kw)
                got = X.replay(case.model, case.vals, base.picks)
            finally:
                X.rule_sigma = orig
            with np.errstate(all='ignore'):
                r = float(np.nanmax(np.abs(got.scores - base.scores) / base.bound))
            worst = min(worst, r)
            assert r > FACTOR, (kind, n, r)
    print('1.02 sigma: smallest worst |d| / bound over the fixtures = %.3g' % worst)


@pytest.mark.parametrize('kind', X.EXACT_MU)
def test_the_tight_allowance_is_far_below_the_bound(kind):
    """The GPU test's second bar, on the oracle's own sides: its median is
    under 1e-6 of the first (it grows with |lk|, which the first does not see),
    and a relative error of 1e-9 in the pending sigma is past it on every
    fixture."""
    for n in X.SIZES:
        case = X.case(kind, n)
        base = X.oracle_run(case)
        jb, ja = B.sides(case.model, case.vals)
        rep = X.replay(case.model, case.vals, base.picks, sides=(jb, ja))
        np.testing.assert_array_equal(rep.scores, base.scores)
        allow = X.tight_allowance(jb[0], rep)
        assert np.median(allow / base.bound) < 1e-6
        orig = X.rule_sigma
        try:
            X.rule_sigma = lambda *a, **kw: (1 + 1e-9) * orig(*a, **kw)
            off = X.replay(case.model, case.vals, base.picks, sides=(jb, ja))
        finally:
            X.rule_sigma = orig
        r = float(np.max(np.abs(off.scores - base.scores) / allow))
        print('%s: (1 + 1e-9) sigma moves an entry by %.3g allowances' % (case.name, r))
        assert r > FACTOR, (case.name, r)
