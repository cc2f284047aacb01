"""Host side of the greedy batch with a pending-trial penalty (no GPU;
DESIGN 5.16): the near-duplicate top-k that motivates it, the pending kernel's
closed-form sigma against ``parzen_fit``, the recursive update against an
explicitly rebuilt above mixture, the selection rule, the argument checks of
``suggest_joint(batch=)``, and the proof that every round of the GPU test's
fixtures is decided under the oracle."""
import numpy as np
import pytest

from hyperopt_amd import hp, rand, tpe, Trials
from hyperopt_amd import _engine as E
from hyperopt_amd.base import Domain

from oracle import tpe_oracle as O
from oracle_algo import oracle_hps
import batch_cases as C
import batch_oracle as B
import group_oracle as G
import spaces


# ------------------------------------------------------------ the motivation
def _xy_space(hp_):
    return {'x': hp_.uniform('x', -1, 1), 'y': hp_.uniform('y', -1, 1),
            'c': hp_.choice('c', [0, 1, 2])}


def _mean_nn(pts):
    d = np.sqrt(((pts[:, None, :] - pts[None, :, :]) ** 2).sum(axis=2))
    np.fill_diagonal(d, np.inf)
    return float(d.min(axis=1).mean())


def test_a_pending_batch_spreads_where_the_top_k_repeats_one_point():
    """x, y ~ uniform(-1, 1) and a 3-way choice, 200 prior trials with loss
    (x - 0.6)^2 + (y - 0.6)^2 + 0.1 c, one 'groups' model, 4096 numpy draws
    from its below side, k = 8.  Measured: the top 8 have EI 8.832 .. 8.830
    and a mean nearest-neighbour distance in (x, y) of 0.0139; the greedy
    batch over the same draw has 0.1663, its picks' original EI running from
    8.832 down to 8.383."""
    dom = Domain(lambda c: 0.0, _xy_space(hp))
    docs = rand.suggest(list(range(200)), dom, Trials(), 3)
    cfgs = [{lab: v[0] for lab, v in d['misc']['vals'].items() if v} for d in docs]
    losses = [(c['x'] - 0.6) ** 2 + (c['y'] - 0.6) ** 2 + 0.1 * c['c'] for c in cfgs]
    _, ls, vals, active = tpe.build_history(dom, C.done(docs, losses))
    h = oracle_hps(dom.space)
    hps = [(lab, h[lab]) for lab in dom.space.labels]
    model = G.GroupModel(hps, ls, vals, active, C.GAMMA, C.PRIOR_WEIGHT)
    draw = B.draw_below(model, hps, 4096, 5)
    ix, iy = dom.space.labels.index('x'), dom.space.labels.index('y')
    res = B.run(model, draw, 8)
    ei = res.scores[0]
    top = tpe.rank_pool(ei, np.ones(4096, dtype=bool), 8)
    assert res.picks[0] == top[0]
    nn_top = _mean_nn(draw[[ix, iy]][:, top].T)
    nn_batch = _mean_nn(draw[[ix, iy]][:, res.picks].T)
    print('top-k: EI %.3f .. %.3f, mean nn %.4f; batch: EI %.3f .. %.3f, mean nn %.4f' % (
        ei[top[0]], ei[top[-1]], nn_top, ei[res.picks].max(), ei[res.picks].min(), nn_batch))
    assert nn_top < 0.05 < nn_batch
    assert nn_batch > 5 * nn_top
    # the gains fall: every pick lowers the EI around itself
    assert (np.diff(res.gains) < 0).all()


# ------------------------------------------------------- the pending kernel
PM, PS = 0.5, 2.0


def _mixture_mus(obs):
    return O.parzen_fit(np.asarray(obs, dtype=np.float64), 1.0, PM, PS, kind='stable')[1]


@pytest.mark.parametrize('obs, mu', [
    ([], 0.3),                              # the prior alone
    ([], PM),
    ([1.0], 0.2), ([1.0], 1.0), ([1.0], 3.0), ([1.0], PM),
    ([0.1, 0.9, 1.4, 2.0], -3.0),           # below all mus
    ([0.1, 0.9, 1.4, 2.0], 7.0),            # above all mus
    ([0.1, 0.9, 1.4, 2.0], 0.9),            # equal to an existing mu
    ([0.1, 0.9, 0.9, 2.0], 0.9),            # ... that is held twice
    ([0.1, 0.9, 1.4, 2.0], PM),             # equal to the prior's mu
    ([PM, PM, 1.4], PM),                    # ... with observations on it
    ([0.1, 0.9, 1.4, 2.0], 1.0),
    ([0.1, 0.9, 1.4, 2.0], 0.1000001),      # the floor of the clip
    ([2.0, 0.1, 1.4, 0.9], 1.5),            # (observation order does not matter)
])
def test_closed_form_sigma_is_parzen_fits(obs, mu):
    want = B.pending_sigma(obs, mu, 1.0, PM, PS)
    got = B.pending_sigma_closed(_mixture_mus(obs), mu, PS)
    assert got == want, (obs, mu, got, want)


@pytest.mark.parametrize('n', [24, 25, 26, 40, 97, 98, 99, 150])
def test_closed_form_sigma_on_long_sides(n):
    """Across the linear-forgetting length and the 100 in the sigma floor."""
    rng = np.random.RandomState(n)
    obs = rng.normal(PM, PS, n)
    mus = _mixture_mus(obs)
    for mu in list(rng.normal(PM, 2 * PS, 20)) + [obs[3], obs.min() - 1, obs.max() + 1, PM]:
        assert B.pending_sigma_closed(mus, mu, PS) == B.pending_sigma(obs, mu, 1.0, PM, PS)


@pytest.mark.parametrize('label', ['qu0', 'lu1', 'u2'])
def test_closed_form_sigma_of_fixture_hps(label):
    """A quantized hp (its observations repeat), a log-scale one and a
    uniform one of cfg2's above side, at values on and between observations."""
    dom, _, vals, _ = C.history('cfg2')
    i = dom.space.labels.index(label)
    d = C.model('cfg2').dims[0][1][C.model('cfg2').groups[0].index(i)]
    fk, pm, ps, low, high, q, tr = O.posterior_spec(d.h['dist'], d.h['args'], C.PRIOR_WEIGHT)
    raw = list(vals[i][:12]) + list(C.configs('cfg2')[i][:12])
    for v in raw:
        mu = float(O.transform_obs(np.array([v]), tr, low)[0])
        got = B.pending_sigma_closed(d.marginal[1], mu, ps)
        assert got == B.pending_dim(d, v).sigma[0], (label, v)
    assert np.unique(d.marginal[1]).size < d.marginal[1].size or label != 'qu0'


def test_round_scores_are_those_of_the_rebuilt_above_mixture():
    """The recursion of the pending components is the log-density of the
    above mixture with them appended and the weights renormalised."""
    for name, picks in (('nested', [3, 17, 17 + 1, 40, 5, 60]), ('cond', [0, 9, 30, 31, 2])):
        model = C.model(name)
        vals = np.ascontiguousarray(C.configs(name)[:, :64])
        res = B.run(model, vals, len(picks), forced=picks)
        on = model.active(vals)
        jb, _ = B.sides(model, vals)
        shared = 0
        for t in range(len(picks)):
            ja = B.rebuilt_above(model, vals, picks[:t])
            with np.errstate(all='ignore'):
                want = G.ordered_sum(np.where(on, jb - ja, 0.0))
            np.testing.assert_allclose(res.scores[t], want, rtol=1e-11, atol=1e-11,
                                       err_msg='%s round %d' % (name, t))
            if t:
                shared += int((res.scores[t] != res.scores[t - 1]).sum())
        assert shared > len(picks)          # (the picks do reach other configurations)
        # a pick is pushed down hardest at itself
        drop = res.scores[0] - res.scores[-1]
        assert (drop[picks[:-1]] > 0).all()


# ------------------------------------------------------- the selection rule
def test_k_1_is_rank_pools_first():
    for name in C.NAMES:
        res = C.oracle_run(name, C.M, 1)
        total = C.model(name).total(np.ascontiguousarray(C.configs(name)))
        np.testing.assert_array_equal(res.scores[0], total)
        assert res.picks[0] == tpe.rank_pool(total, np.ones(C.M, dtype=bool), 1)[0]
        assert res.gains[0] == total[res.picks[0]]


def test_duplicates_sink_nan_is_last_and_eligible_holds():
    model = C.model('cond')
    base = np.ascontiguousarray(C.configs('cond')[:, :6])
    labels = C.history('cond')[0].space.labels
    # columns: 0..5 distinct, 6 = 0 again, 7 = 1 again, 8 = a bad value (NaN score)
    vals = np.concatenate([base, base[:, [0, 1]], base[:, [2]]], axis=1)
    vals[labels.index('aa'), 8] = np.nan
    res = B.run(model, vals, 9)
    assert np.isnan(res.scores[0][8]) and np.isfinite(res.scores[0][:8]).all()
    assert sorted(res.picks[:6]) == [0, 1, 2, 3, 4, 5]      # every non-duplicate first
    assert res.picks[6] == 8                                # ... the NaN one last of them
    assert sorted(res.picks[7:]) == [6, 7]                  # then the duplicates
    np.testing.assert_array_equal(B.apply_rule(res.scores, B.config_keys(model, vals)), res.picks)
    # equal scores: the lower index wins
    first = tpe.rank_pool(res.scores[0], np.ones(9, dtype=bool), 9)
    assert list(first).index(0) < list(first).index(6)
    # the mask
    el = np.ones(9, dtype=bool)
    el[[res.picks[0], 3]] = False
    masked = B.run(model, vals, 7, eligible=el)
    assert not set(masked.picks) & {int(res.picks[0]), 3}
    with pytest.raises(ValueError):
        B.run(model, vals, 8, eligible=el)
    assert list(B.apply_rule(np.tile(res.scores[0], (8, 1)), B.config_keys(model, vals),
                             el))[-1] == -1


# ------------------------------------------------------------- the plumbing
def test_suggest_joint_batch_argument_is_checked_before_startup():
    dom = Domain(lambda c: 0.0, spaces.cond_space(hp))
    for mv in (False, True):
        with pytest.raises(ValueError, match="multivariate='groups'"):
            tpe.suggest_joint([0], dom, Trials(), 1, batch='pending', multivariate=mv)
    with pytest.raises(ValueError, match='bogus'):
        tpe.suggest_joint([0], dom, Trials(), 1, batch='bogus', multivariate='groups')
    # the startup branch itself is untouched
    docs = tpe.suggest_joint([0, 1], dom, Trials(), 1, batch='pending', multivariate='groups')
    want = rand.suggest([0, 1], dom, Trials(), 1, rng_stream='numpy')
    assert [d['misc']['vals'] for d in docs] == [d['misc']['vals'] for d in want]


def test_abi_declares_the_batch_call():
    assert 'tpe_plan_group_batch_points' in E.EXPORTS
    assert E.BATCH_MAX == 1024
    assert hasattr(E.Plan, 'group_batch_points') and hasattr(E.Plan, 'group_batch_points_device')


# --------------------------------------------------- the GPU test's fixtures
def _cases():
    out = [(name, C.M, C.K) for name in C.NAMES]
    return out + [('cond', m, k) for m, k in C.SHAPES if (m, k) != (C.M, C.K)]


@pytest.mark.parametrize('name, m, k', _cases())
def test_every_gpu_round_is_decided(name, m, k):
    """Decided: the pick's score exceeds every other selectable score of its
    tier by more than 4x the GPU test's bound on a score (the larger of the
    two).  The cap on undecided rounds is zero."""
    res = C.oracle_run(name, m, k)
    print('%s m=%d k=%d: min margin / bound = %.3g' % (name, m, k, res.ratio.min()))
    assert np.isfinite(res.scores[np.arange(k), res.picks]).all()
    assert (res.ratio > 4.0).all(), res.ratio
    assert len(set(res.picks.tolist())) == k
