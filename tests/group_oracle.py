"""Numpy restatement of multivariate TPE with one joint Parzen model per group
of hps that are always active together -- TEST INFRASTRUCTURE
ONLY, composed from ``joint_oracle``: ``side_rows``, ``side_weights`` and
``DimFit`` do the per-side and per-dimension work.

A group is a maximal set of hps with the same set of immediate
(parent, branch) alternatives; group 0 holds the unconditional hps, the others
follow in ascending order of their smallest hp index.  Group g's side s holds
the rows of the split side in which the group is active, in row order;
J_gs(c) = logsumexp_k [log w_k + sum_{d in g} log kappa_dk(c_d)],
joint_g = J_g,below - J_g,above, and EI(c) is the sum of joint_g(c) over the
groups active in c, in group order."""
import numpy as np

from oracle import tpe_oracle as O
import joint_oracle as J


def nested_space(hp):
    """Nested choices and a label shared by two branches: the groups are
    {top}, {inner, w}, {p, q}, {r}, {shared}, {v}, {z}."""
    shared = hp.loguniform('shared', -2, 0)
    inner = hp.choice('inner', [{'p': hp.uniform('p', 0, 1), 'q': hp.normal('q', 0, 1)},
                                {'r': hp.quniform('r', 0, 10, 1)}])
    return hp.choice('top', [{'inner': inner, 'w': hp.lognormal('w', 0, 1), 's': shared},
                             {'v': hp.randint('v', 5), 's': shared},
                             {'z': hp.uniform('z', -1, 1)}])


def immediate(h):
    """The set of immediate (parent label, branch) alternatives of an hp
    description (``spaces.describe`` or ``oracle_algo.oracle_hps``)."""
    paths = h['paths'] if 'paths' in h else [h['conds']]
    if any(len(p) == 0 for p in paths):
        return frozenset()
    return frozenset(tuple(p[-1]) for p in paths)


def partition(hps):
    """[[hp index, ...], ...]: group 0 the unconditional hps."""
    groups, where = [[]], {frozenset(): 0}
    for i, (_, h) in enumerate(hps):
        key = immediate(h)
        if key not in where:
            where[key] = len(groups)
            groups.append([])
        groups[where[key]].append(i)
    return groups


class GroupModel(object):
    """hps: [(label, description)] in hp index order; vals[P, n] and
    active[P, n] the history columns (the hps of a group active in the same
    rows, the unconditional ones in all)."""

    def __init__(self, hps, losses, vals, active, gamma=0.25, prior_weight=1.0, lf=O.DEFAULT_LF,
                 gamma_cap=O.DEFAULT_LF):
        losses = np.asarray(losses, dtype=np.float64)
        vals, active = np.asarray(vals), np.asarray(active) != 0
        self.labels = [lab for lab, _ in hps]
        self.groups = partition(hps)
        index = {lab: i for i, lab in enumerate(self.labels)}
        self.alts = [sorted((index[lab], int(b)) for lab, b in immediate(hps[g[0]][1])) if g else []
                     for g in self.groups]
        self.group_of = {i: gi for gi, g in enumerate(self.groups) for i in g}
        split = J.side_rows(losses, gamma, gamma_cap)
        self.rows, self.w, self.S, self.dims = [], [], [], []
        for g in self.groups:
            rows, ws, Ss, dims = [], [], [], []
            for s in range(2):
                r = split[s] if not g else split[s][active[g[0]][split[s]]]
                w, S = J.side_weights(r.size, prior_weight, lf)
                rows.append(r)
                ws.append(w)
                Ss.append(S)
                dims.append([J.DimFit(hps[i][1], vals[i][r], S, prior_weight, lf) for i in g])
            self.rows.append(rows)
            self.w.append(ws)
            self.S.append(Ss)
            self.dims.append(dims)

    def active(self, vals):
        """on[G, M]: some alternative holds with the parent's group active."""
        vals = np.asarray(vals, dtype=np.float64)
        M = vals.shape[1]
        on = [None] * len(self.groups)

        def visit(g):
            if on[g] is None:
                on[g] = np.ones(M, dtype=bool) if g == 0 else np.zeros(M, dtype=bool)
                for par, br in self.alts[g]:
                    on[g] |= visit(self.group_of[par]) & (vals[par] == float(br))
            return on[g]

        return np.stack([visit(g) for g in range(len(self.groups))])

    def sides(self, vals):
        """(J_below[G, M], J_above[G, M]), NaN where the group is inactive."""
        vals = np.asarray(vals, dtype=np.float64)
        on = self.active(vals)
        out = []
        with np.errstate(all='ignore'):
            for s in range(2):
                js = np.full(on.shape, np.nan)
                for g, hp_ids in enumerate(self.groups):
                    sel = on[g]
                    a = np.log(self.w[g][s])[None, :] + np.zeros((int(sel.sum()), 1))
                    for i, d in zip(hp_ids, self.dims[g][s]):
                        a = a + d.log_kernel(vals[i][sel])
                    js[g, sel] = O.lse_rows(a) if a.shape[0] else np.zeros(0)
                out.append(js)
        return out[0], out[1]

    def joint(self, vals):
        """joint[G, M], 0.0 where the group is inactive."""
        jb, ja = self.sides(vals)
        with np.errstate(all='ignore'):
            return np.where(self.active(vals), jb - ja, 0.0)

    def total(self, vals):
        return ordered_sum(self.joint(vals))


def ordered_sum(joint):
    """The float64 sum of joint[G, M] over the groups, in group order from 0.0."""
    acc = np.zeros(joint.shape[1])
    with np.errstate(all='ignore'):
        for row in joint:
            acc = acc + row
    return acc
