"""Pairwise importances under the group models (include/tpe_engine.h states the
rule) in plain float64 numpy.  A dim is (dist, args, [below, above]) with a side (mu[K], sigma[K])
in component order as ``Plan.group_mixture`` and ``joint_oracle.DimFit`` hold them (categorical:
the observed option, -1 for the prior, and the smoothing a); a side's weights are w[K]."""
import numpy as np
from scipy.special import erf, erfc

from oracle import tpe_oracle as O
import importance_oracle as IO
import joint_oracle as J

EPS, TILE = O.EPS, 64


def _cat(dist):
    return dist in ('randint', 'categorical')


def dim_nodes(dist, args, sides, G):
    """(x, w) of one dim: ``importance_oracle.nodes`` on what the rule reads of the mixtures."""
    if _cat(dist):
        pi = J.cat_prior(dict(dist=dist, args=args))
        return IO.nodes(dist, args, pi, pi, G)[:2]
    srt = [(None, np.sort(mu), None) for mu, _ in sides]
    return IO.nodes(dist, args, srt[0], srt[1], G)[:2]


def _cell(zu, zl):
    """Phi(zu) - Phi(zl) in erf arguments, in the complement of the nearer tail."""
    up, lo = zl >= 0, zu <= 0
    return 0.5 * np.where(up, erfc(zl) - erfc(zu),
                          np.where(lo, erfc(-zu) - erfc(-zl), erf(zu) - erf(zl)))


def factors(dist, args, mu, sigma, x):
    """kappa[K, n]: every component's kernel at the nodes, in the linear domain."""
    mu, sg, xs = np.asarray(mu)[:, None], np.asarray(sigma)[:, None], np.asarray(x)[None, :]
    with np.errstate(all='ignore'):
        if _cat(dist):
            pi = J.cat_prior(dict(dist=dist, args=args))[xs.astype(np.int64)]
            return np.where(np.arange(mu.size)[:, None] == 0, pi, ((mu == xs) + sg * pi) / (1 + sg))
        fk, _, _, low, high, q, _ = O.posterior_spec(dist, args, 1.0)
        lg = fk == 'lgmm'
        if q is None:
            s = np.maximum(sg, EPS)
            z = ((np.log(xs) if lg else xs) - mu) / s
            return np.exp(-0.5 * (z * z)) / (np.sqrt(2 * np.pi) * (s * xs if lg else sg))
        ub, lb = xs + q / 2.0, xs - q / 2.0
        if high is not None:
            ub = np.minimum(ub, np.exp(high) if lg else high)
        if low is not None:
            lb = np.maximum(lb, np.exp(low) if lg else low)
        if lg:
            ub, lb = np.log(np.maximum(ub, EPS)), np.log(np.maximum(np.maximum(0, lb), EPS))
        d = np.maximum(np.sqrt(2) * sg, EPS)
        return _cell((ub - mu) / d, (lb - mu) / d)


def planes(dim_a, dim_b, weights, G):
    """(x_a, w_a, x_b, w_b, [L_below, L_above]) of one pair."""
    xa, wa = dim_nodes(*dim_a, G)
    xb, wb = dim_nodes(*dim_b, G)
    L = [(factors(*dim_a[:2], *dim_a[2][s], xa) * np.asarray(weights[s])[:, None]).T
         @ factors(*dim_b[:2], *dim_b[2][s], xb) for s in range(2)]
    return xa, wa, xb, wb, L


def integrate(L, wa, wb, ghat, rtol=0.0):
    """dict(D, Zb, Za, S = sum |f|, B): the pair's divergence and covered masses; B bounds
    the change of D when L_below and L_above move by rtol max(1, |log L|) each."""
    W = np.outer(wa, wb)
    with np.errstate(all='ignore'):
        Z = [float((W * Ls).sum()) for Ls in L]
        l, g = L[0] / Z[0], L[1] / Z[1]
        q = ghat * l + (1.0 - ghat) * g
        on = q > 0
        den = np.where(on, q, 1.0)
        f = np.where(on, W * (l - g) ** 2 / den, 0.0)
        mag = [np.maximum(1.0, np.abs(np.where(Ls > 0, np.log(Ls), 0.0))) for Ls in L]
        b = np.where(on, rtol * (mag[0] + mag[1]) * W * (l + g) ** 2 / den, 0.0)
    c = (1.0 - ghat) * (1.0 - ghat)
    return dict(D=0.0 if ghat == 1.0 else c * float(f.sum()), Zb=Z[0], Za=Z[1],
                S=float(np.abs(f).sum()), B=c * float(b.sum()))


def from_group_model(model, g, ia, ib):
    """(dim_a, dim_b, weights) of hps ia < ib of group g of a ``group_oracle.GroupModel``."""
    dims = []
    for i in (ia, ib):
        d = [model.dims[g][s][model.groups[g].index(i)] for s in range(2)]
        h = d[0].h
        if d[0].cat:
            sides = [(np.concatenate([[-1.0], f.obs]), np.full(f.obs.size + 1, f.a)) for f in d]
        else:
            sides = [(f.mu, f.sigma) for f in d]
        dims.append((h['dist'], h['args'], sides))
    return dims[0], dims[1], model.w[g]
