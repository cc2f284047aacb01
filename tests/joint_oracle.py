"""Numpy restatement of the multivariate (joint Parzen) TPE model over the
unconditional hps -- TEST INFRASTRUCTURE ONLY, composed from
``oracle.tpe_oracle``: the stable split, ``parzen_fit(return_order=True)``,
``lf_weights``, the cdf / lpdf helpers and ``lse_rows``.

Side s of the split holds n_s rows in row order and K_s = n_s + 1 components:
component 0 is the prior, component k the side's k-th row.  Per root hp a
component carries the kernel the hp's marginal fit gave that row's
observation, so per hp the multiset of (w, mu, sigma) is the marginal
mixture; J_s(c) = logsumexp_k [log w_k + sum_d log kappa_dk(c_d)] and
joint(c) = J_below(c) - J_above(c)."""
import numpy as np

from oracle import tpe_oracle as O

EPS = O.EPS


def is_root(h):
    """An hp description (``spaces.describe`` or ``oracle_algo.oracle_hps``)
    without a condition."""
    if 'paths' in h:
        return any(len(p) == 0 for p in h['paths'])
    return len(h['conds']) == 0


def side_rows(losses, gamma, gamma_cap=O.DEFAULT_LF):
    """(below rows, above rows), each ascending: the stable split."""
    tids = np.arange(len(losses))
    good, bad = O.below_tids(tids, losses, gamma, gamma_cap, kind='stable')
    return np.array(sorted(good), dtype=np.int64), np.array(sorted(bad), dtype=np.int64)


def side_weights(n_s, prior_weight, lf=O.DEFAULT_LF):
    """(w[K], S): w_0 the prior's weight, w_k the k-th row's (lf = 0: no
    forgetting, as ``parzen_fit`` reads it)."""
    lw = O.lf_weights(n_s, lf) if lf and lf < n_s else np.ones(n_s)
    S = lw.sum() if n_s else 0.0
    return np.concatenate([[prior_weight], lw]) / (S + prior_weight), S


def cat_prior(h):
    if h['dist'] == 'randint':
        upper = int(h['args'][0])
        return np.full(upper, 1.0 / upper)
    return np.asarray(h['args'][0], dtype=np.float64)


def cat_a(upper, S, prior_weight):
    return prior_weight * (upper - 1) / (S + prior_weight)


def kappa(obs, a, pi):
    """kappa[k, c] of a categorical hp: row 0 the prior, row k >= 1 the
    component observing obs[k - 1] (the model's operation order)."""
    c = np.arange(pi.size)
    rows = ((c[None, :] == np.asarray(obs)[:, None]).astype(np.float64) + a * pi[None, :]) / (1 + a)
    return np.concatenate([pi[None, :], rows], axis=0)


class DimFit(object):
    """One root hp on one side, in component order."""

    def __init__(self, h, obs_raw, S, prior_weight, lf):
        self.h = h
        self.cat = h['dist'] in ('randint', 'categorical')
        n = len(obs_raw)
        if self.cat:
            self.pi = cat_prior(h)
            self.a = cat_a(self.pi.size, S, prior_weight)
            self.obs = np.asarray(obs_raw).astype(np.int64)
            self.kappa = kappa(self.obs, self.a, self.pi)
            return
        self.fk, pm, ps, self.low, self.high, self.q, tr = O.posterior_spec(
            h['dist'], h['args'], prior_weight)
        obs = O.transform_obs(obs_raw, tr, self.low)
        w, mus, sig, order, pos = O.parzen_fit(obs, prior_weight, pm, ps, lf=lf, kind='stable',
                                               return_order=True)
        if n == 0:
            place = np.zeros(0, dtype=np.int64)
        elif n == 1:
            place = np.array([1 - pos])
        else:
            rank = np.empty(n, dtype=np.int64)
            rank[order] = np.arange(n)
            place = rank + (rank >= pos)
        place = np.concatenate([[pos], place]).astype(np.int64)
        self.place = place                     # component k -> index in the marginal mixture
        self.marginal = (w, mus, sig)
        self.w, self.mu, self.sigma = w[place], mus[place], sig[place]
        self.obs = obs

    def log_kernel(self, x):
        """log kappa_k(x_m) as [M, K]."""
        x = np.asarray(x, dtype=np.float64)
        with np.errstate(all='ignore'):
            if self.cat:
                ok = (x >= 0) & (x < self.pi.size) & (np.floor(x) == x)
                c = np.where(ok, x, 0).astype(np.int64)
                out = np.log(self.kappa[:, c]).T
                out[~ok] = np.nan
                return out
            mu, sg = self.mu[None, :], self.sigma[None, :]
            xs = x[:, None]
            lg = self.fk == 'lgmm'
            if self.q is None:
                if lg:
                    return O.lognormal_lpdf(xs, mu, sg)
                return -0.5 * ((xs - mu) / np.maximum(sg, EPS)) ** 2 - np.log(
                    np.sqrt(2 * np.pi * sg ** 2))
            q, low, high = self.q, self.low, self.high
            if lg:
                ub = xs + q / 2.0 if high is None else np.minimum(xs + q / 2.0, np.exp(high))
                lb = xs - q / 2.0 if low is None else np.maximum(xs - q / 2.0, np.exp(low))
                lb = np.maximum(0, lb)
                ub = np.where(ub < 0, np.nan, ub)
                return np.log(O.lognormal_cdf(ub, mu, sg) - O.lognormal_cdf(lb, mu, sg))
            ub = xs + q / 2.0 if high is None else np.minimum(xs + q / 2.0, high)
            lb = xs - q / 2.0 if low is None else np.maximum(xs - q / 2.0, low)
            return np.log(O.normal_cdf(ub, mu, sg) - O.normal_cdf(lb, mu, sg))


class JointModel(object):
    """hps: [(label, description)] in hp index order; vals[P, n] the history
    columns (root hps active in every row)."""

    def __init__(self, hps, losses, vals, gamma=0.25, prior_weight=1.0, lf=O.DEFAULT_LF,
                 gamma_cap=O.DEFAULT_LF):
        losses = np.asarray(losses, dtype=np.float64)
        self.roots = [i for i, (_, h) in enumerate(hps) if is_root(h)]
        self.rows = side_rows(losses, gamma, gamma_cap)
        self.w, self.S, self.dims = [], [], []
        for s in range(2):
            r = self.rows[s]
            w, S = side_weights(r.size, prior_weight, lf)
            self.w.append(w)
            self.S.append(S)
            self.dims.append([DimFit(hps[i][1], np.asarray(vals)[i][r], S, prior_weight, lf)
                              for i in self.roots])

    def sides(self, vals):
        """(J_below[M], J_above[M]) of configurations vals[P, M]."""
        vals = np.asarray(vals, dtype=np.float64)
        out = []
        with np.errstate(all='ignore'):
            for s in range(2):
                a = np.log(self.w[s])[None, :] + np.zeros((vals.shape[1], 1))
                for i, d in zip(self.roots, self.dims[s]):
                    a = a + d.log_kernel(vals[i])
                out.append(O.lse_rows(a))
        return out[0], out[1]

    def joint(self, vals):
        jb, ja = self.sides(vals)
        with np.errstate(all='ignore'):
            return jb - ja
