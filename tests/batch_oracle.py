"""Numpy restatement of the greedy batch with a pending-trial penalty
(tpe_plan_group_batch_points) -- TEST INFRASTRUCTURE ONLY, built
on ``group_oracle.GroupModel``.

Round t scores every configuration, score_t(c) = the ordered float64 sum of
J_g,below(c) - Ja_g(c) over the groups active in c, and picks the first
selectable one in ``tpe.rank_pool``'s order, configurations equal to a taken
one last.  The pick joins the above side of each of its active groups as one
pending component of unnormalised weight 1:
  Ja_g(c) <- logaddexp(Ja_g(c) + log(W_g + n_g), sum_d log kappa_d(c_d; p_d))
             - log(W_g + n_g + 1),      W_g = S_g,above + prior_weight,
with the kernel ``oracle.parzen_fit`` gives the pick's value appended to the
hp's above observations."""
import copy

import numpy as np

from hyperopt_amd import tpe

from oracle import tpe_oracle as O
from gpu_util import RTOL
import group_oracle as G
import joint_oracle as J


def pending_sigma(obs, mu, prior_weight, prior_mu, prior_sigma, lf=O.DEFAULT_LF):
    """The sigma ``parzen_fit`` (stable) assigns to ``mu`` appended to the
    transformed observations ``obs``."""
    allobs = np.append(np.asarray(obs, dtype=np.float64), mu)
    _, _, sig, order, pos = O.parzen_fit(allobs, prior_weight, prior_mu, prior_sigma, lf=lf,
                                         kind='stable', return_order=True)
    n = allobs.size
    if n == 1:
        return sig[1 - pos]
    rank = int(np.flatnonzero(order == n - 1)[0])
    return sig[rank + (rank >= pos)]


def pending_sigma_closed(mus, mu, prior_sigma):
    """The same from the hp's sorted above mixture ``mus`` (the prior in it,
    K of them), as the device finds it: the left neighbour is the last
    mu_k <= mu, the right one the first mu_k > mu."""
    mus = np.asarray(mus, dtype=np.float64)
    K = mus.size
    if K == 1:
        return 0.5 * prior_sigma
    lo = int(np.searchsorted(mus, mu, side='right'))
    gaps = ([mu - mus[lo - 1]] if lo > 0 else []) + ([mus[lo] - mu] if lo < K else [])
    return min(max(max(gaps), prior_sigma / min(100.0, 2.0 + K)), prior_sigma)


def pending_dim(d, value, prior_weight=1.0, lf=O.DEFAULT_LF):
    """A one-component ``DimFit`` of the pending kernel of the above-side dim
    ``d`` for a pick's raw ``value``: ``.log_kernel(x)[:, 0]``."""
    p = copy.copy(d)
    if d.cat:
        ok = 0 <= value < d.pi.size and float(value).is_integer()
        p.kappa = J.kappa([int(value) if ok else -1], d.a, d.pi)[1:2]
        return p
    fk, pm, ps, low, high, q, tr = O.posterior_spec(d.h['dist'], d.h['args'], prior_weight)
    mu = float(O.transform_obs(np.array([value], dtype=np.float64), tr, low)[0])
    p.mu = np.array([mu])
    p.sigma = np.array([pending_sigma(d.obs, mu, prior_weight, pm, ps, lf)])
    return p


class Result(object):
    """picks[k], gains[k], scores[k, M] (every configuration's score per
    round), bound[k, M] (the GPU tolerance on each of them) and ratio[k] -- per round
    the smallest (score of the pick - score of another selectable
    configuration of its tier) / (the larger of the two bounds); inf when the
    pick is alone in its tier."""

    def __init__(self, picks, gains, scores, bound, ratio):
        self.picks, self.gains, self.scores = picks, gains, scores
        self.bound, self.ratio = bound, ratio


def score_bound(on, jb, ja):
    """The GPU test's bound on a score: RTOL max(1, |value|) on each of
    J_below and Ja per active group, summed."""
    with np.errstate(all='ignore'):
        per = RTOL * (np.maximum(1.0, np.abs(jb)) + np.maximum(1.0, np.abs(ja)))
    return np.where(on, per, 0.0).sum(axis=0)


def sides(model, vals):
    """``GroupModel.sides``, also where a group is active in no configuration
    (the quantized kernels of ``DimFit`` do not take an empty array)."""
    on = model.active(vals)
    out = []
    with np.errstate(all='ignore'):
        for s in range(2):
            js = np.full(on.shape, np.nan)
            for g, hp_ids in enumerate(model.groups):
                sel = on[g]
                if not sel.any():
                    continue
                a = np.log(model.w[g][s])[None, :] + np.zeros((int(sel.sum()), 1))
                for i, d in zip(hp_ids, model.dims[g][s]):
                    a = a + d.log_kernel(vals[i][sel])
                js[g, sel] = O.lse_rows(a)
            out.append(js)
    return out[0], out[1]


def config_keys(model, vals):
    """``tpe._row_keys`` of configurations under the model's activity."""
    vals = np.asarray(vals, dtype=np.float64)
    on = model.active(vals)
    hp_on = np.zeros(vals.shape, dtype=bool)
    for g, hp_ids in enumerate(model.groups):
        hp_on[hp_ids] = on[g]
    return tpe._row_keys(vals, hp_on)


def apply_rule(scores, keys, eligible=None):
    """The picks the rule makes from given per-round scores[k, M]: per round
    the first selectable configuration in ``rank_pool``'s order, those whose
    key equals a taken one's after all others; -1 from the first round
    without one."""
    M = scores.shape[1]
    eligible = np.ones(M, dtype=bool) if eligible is None else np.asarray(eligible, dtype=bool)
    taken, dup = np.zeros(M, dtype=bool), np.zeros(M, dtype=bool)
    picks = []
    for score in scores:
        sel = eligible & ~taken
        tier = sel & ~dup if (sel & ~dup).any() else sel
        if not tier.any():
            return np.array(picks + [-1] * (len(scores) - len(picks)))
        p = int(tpe.rank_pool(score, tier, 1)[0])
        picks.append(p)
        taken[p] = True
        dup |= keys == keys[p]
    return np.array(picks)


def run(model, vals, k, eligible=None, forced=None, prior_weight=1.0, lf=O.DEFAULT_LF):
    """The greedy batch of ``k`` over configurations ``vals[P, M]`` under the
    ``GroupModel``; ``forced``: take these picks instead of the rule's (the
    scores are then those of the forced sequence).  ValueError when a round
    has no selectable configuration."""
    vals = np.asarray(vals, dtype=np.float64)
    M = vals.shape[1]
    on = model.active(vals)
    jb, ja = sides(model, vals)
    keys = config_keys(model, vals)
    eligible = np.ones(M, dtype=bool) if eligible is None else np.asarray(eligible, dtype=bool)
    taken, dup = np.zeros(M, dtype=bool), np.zeros(M, dtype=bool)
    n_g = [0] * len(model.groups)
    picks, gains, scores, ratios, bounds = [], [], [], [], []
    for t in range(k):
        with np.errstate(all='ignore'):
            score = G.ordered_sum(np.where(on, jb - ja, 0.0))
        bound = score_bound(on, jb, ja)
        bounds.append(bound)
        sel = eligible & ~taken
        tier = sel & ~dup if (sel & ~dup).any() else sel
        if not tier.any():
            raise ValueError('round %d: no selectable configuration' % t)
        p = int(tpe.rank_pool(score, tier, 1)[0]) if forced is None else int(forced[t])
        others = tier.copy()
        others[p] = False
        with np.errstate(all='ignore'):
            r = (score[p] - score[others]) / np.maximum(bound[p], bound[others])
        ratios.append(np.inf if not others.any() or not tier[p] else
                      float(np.min(np.where(np.isnan(score[others]), np.inf, r))))
        picks.append(p)
        gains.append(score[p])
        scores.append(score)
        taken[p] = True
        dup |= keys == keys[p]
        for g, hp_ids in enumerate(model.groups):
            if not on[g][p]:
                continue
            c = on[g]                               # (p itself is in it)
            lk = np.zeros(int(c.sum()))
            with np.errstate(all='ignore'):
                for i, d in zip(hp_ids, model.dims[g][1]):
                    lk = lk + pending_dim(d, vals[i][p], prior_weight, lf).log_kernel(
                        vals[i][c])[:, 0]
                W = model.S[g][1] + prior_weight + n_g[g]
                ja[g][c] = np.logaddexp(ja[g][c] + np.log(W), lk) - np.log(W + 1.0)
            n_g[g] += 1
    return Result(np.array(picks), np.array(gains), np.array(scores), np.array(bounds),
                  np.array(ratios))


def rebuilt_above(model, vals, pending, prior_weight=1.0, lf=O.DEFAULT_LF):
    """Ja[G, M] under explicitly rebuilt above mixtures: per group the fitted
    components with their unnormalised weights and one component of weight 1
    per configuration of ``pending`` (indices into ``vals``) that activates
    the group, the weights renormalised; NaN where the group is inactive."""
    vals = np.asarray(vals, dtype=np.float64)
    on = model.active(vals)
    out = np.full(on.shape, np.nan)
    for g, hp_ids in enumerate(model.groups):
        c = on[g]
        if not c.any():
            continue
        mine = [p for p in pending if on[g][p]]
        W = model.S[g][1] + prior_weight
        w = np.concatenate([model.w[g][1] * W, np.ones(len(mine))]) / (W + len(mine))
        with np.errstate(all='ignore'):
            a = np.log(w)[None, :] + np.zeros((int(c.sum()), 1))
            for i, d in zip(hp_ids, model.dims[g][1]):
                cols = [d.log_kernel(vals[i][c])]
                cols += [pending_dim(d, vals[i][p], prior_weight, lf).log_kernel(vals[i][c])
                         for p in mine]
                a = a + np.concatenate(cols, axis=1)
            out[g, c] = O.lse_rows(a)
    return out


def draw_below(model, hps, n, seed):
    """``n`` configurations [P, n] drawn from the group models' below sides in
    numpy: every active group picks a component and draws its hps from it
    (a bounded continuous hp by rejection; unbounded, log-scale and quantized
    kinds are not needed by the host tests and not handled)."""
    rng = np.random.RandomState(seed)
    P = len(hps)
    vals = np.full((P, n), np.nan)
    for j in range(n):
        done = set()
        while True:
            on = model.active(vals[:, j:j + 1])[:, 0]
            todo = [g for g in range(len(model.groups)) if on[g] and g not in done]
            if not todo:
                break
            g = todo[0]
            done.add(g)
            comp = rng.choice(model.w[g][0].size, p=model.w[g][0])
            for i, d in zip(model.groups[g], model.dims[g][0]):
                if d.cat:
                    vals[i, j] = rng.choice(d.pi.size, p=d.kappa[comp])
                    continue
                assert d.q is None and d.fk == 'gmm' and d.low is not None and d.high is not None
                while True:
                    x = rng.normal(d.mu[comp], d.sigma[comp])
                    if d.low <= x < d.high:
                        vals[i, j] = x
                        break
    return vals
