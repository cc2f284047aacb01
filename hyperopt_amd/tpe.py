"""TPE suggestion on the MI355X engine -- ``tpe.suggest`` drop-in.

Same call as the reference (hyperopt/tpe.py:804-897)::

    suggest(new_ids, domain, trials, seed, prior_weight=1.0, n_startup_jobs=20,
            n_EI_candidates=24, gamma=0.25, linear_forgetting=25)

Host side (this module): the trial history is a columnar mirror of the
Trials (``history.TrialHistory``: tpe.py:820-848 semantics, synced
incrementally and copied to the device row by row), the startup fallback to
``rand.suggest`` and the write-back of the winning values (tpe.py:887-897).
Device side (libtpe_engine.so, one plan per Domain): the good/bad split,
every hyperparameter's two Parzen fits, candidate draws, below/above lpdf
and the EI argmax, level by level through conditional choices.  There is no
CPU fallback: without the engine this raises.

``new_ids`` may hold several ids (the reference accepts exactly one,
tpe.py:812): the suggestions are served by ONE batched engine call on the
same history, suggestion s drawing its candidates with ``batch_seeds(seed,
S)[s]`` (s = 0 uses ``seed`` itself, so a single suggestion is unchanged).

``rng_stream='numpy'`` replays the reference's RandomState candidate stream
(hyperopt draws in its interpreter order): the fit and the scoring stay on the
GPU, the draws are made on the host with the reference's numpy calls, so the
suggestions equal the reference's (up to 1e-6 EI ties).  The default
``'philox'`` draws candidates on the device (counter-based Philox keyed by
seed, hp and candidate index).
"""
from __future__ import annotations

import logging
import math
import threading
import weakref

import numpy as np

from . import _engine as E
from . import rand, rstream
from .history import TrialHistory, check_objectives, check_hypervolume, HV_N_SAMPLES

logger = logging.getLogger(__name__)

EPS = 1e-12
DEFAULT_LF = 25

_default_prior_weight = 1.0
_default_n_EI_candidates = 24
_default_gamma = 0.25
_default_n_startup_jobs = 20
_default_linear_forgetting = DEFAULT_LF


def build_history(domain, trials, labels=None):
    """(tids, losses[N], vals[P, N], active[P, N]) of ``trials`` in tid
    order -- the reference's history assembly (tpe.py:820-848), from a
    fresh columnar mirror.  ``labels`` must be the domain's (sorted) labels."""
    h = TrialHistory(domain)
    if labels is not None and list(labels) != h.labels:
        raise ValueError('labels must be the domain space labels')
    return h.sync(trials).columns()


def batch_seeds(seed, n):
    """Per-suggestion Philox keys of a batch: ``seed`` first, then splitmix64
    steps of it (independent streams; deterministic in (seed, position))."""
    out = [int(seed) & (2 ** 64 - 1)]
    z = out[0]
    for _ in range(1, n):
        z = (z + 0x9E3779B97F4A7C15) & (2 ** 64 - 1)
        x = z
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & (2 ** 64 - 1)
        out.append(x ^ (x >> 31))
    return out


# --------------------------------------------------------------------------
# per-Domain device state: the plan, and one history mirror per Trials
# --------------------------------------------------------------------------
class _State(object):
    def __init__(self):
        self.plan = None
        self.lock = threading.Lock()
        self.histories = weakref.WeakKeyDictionary()

    def history(self, domain, trials):
        h = self.histories.get(trials)
        if h is None:
            h = self.histories[trials] = TrialHistory(domain)
        return h

    def plan_for(self, domain, n, engine):
        p = self.plan
        if p is None or p.max_trials < n or p.engine is not engine:
            cap = max(64, 1 << max(0, int(math.ceil(math.log2(max(n, 1))))))
            hps, conds, pprior = domain.space.engine_tables()
            self.plan = p = E.Plan(engine, hps, conds, pprior, cap)
        return p


def _state(domain):
    st = domain.__dict__.get('_tpe_state')
    if st is None:
        st = domain.__dict__.setdefault('_tpe_state', _State())
    return st


def _domain_plan(domain, n_trials, engine):
    """The domain's plan, sized for ``n_trials`` (tools / tests)."""
    st = _state(domain)
    st.plan_for(domain, n_trials, engine)
    return st


def _fmt(h, v):
    return int(round(v)) if h.is_categorical else float(v)


def _new_doc(domain, trials, cs, new_id, chosen):
    """The returned document (tpe.py:887-897): misc idxs / vals of the one
    new id -- what miscs_update_idxs_vals(idxs_map={fake_ids[0]: new_id})
    leaves in it, built directly (one misc, every label present)."""
    misc = dict(tid=new_id, cmd=domain.cmd, workdir=domain.workdir,
                idxs={lab: ([new_id] if lab in chosen else []) for lab in cs.labels},
                vals={lab: ([chosen[lab]] if lab in chosen else []) for lab in cs.labels})
    return trials.new_trial_docs([new_id], [None], [domain.new_result()], [misc])[0]


def _picks(cs, res):
    """{label: value} of every suggestion's active winners, from the engine's
    [S][P] records (one conversion to Python lists, no per-field numpy
    scalar access)."""
    S = res.shape[0]
    act = res['active'].tolist()
    idx = res['index'].tolist()
    val = res['value'].tolist()
    out = []
    for s in range(S):
        a, i, v = act[s], idx[s], val[s]
        out.append({lab: (int(round(v[j])) if cat else v[j])
                    for lab, j, cat in cs.pick_order if a[j] and i[j] >= 0})
    return out


def suggest(new_ids, domain, trials, seed,
            prior_weight=_default_prior_weight,
            n_startup_jobs=_default_n_startup_jobs,
            n_EI_candidates=_default_n_EI_candidates,
            gamma=_default_gamma,
            linear_forgetting=_default_linear_forgetting,
            rng_stream='philox', startup_stream='numpy', engine=None, objectives=None,
            hypervolume=False):
    """hyperopt/tpe.py:804-897 on the GPU, one document per id in
    ``new_ids``.  ``linear_forgetting`` is accepted and, as in the reference
    (tpe.py:809), not used: LF is fixed at 25.  The first ``n_startup_jobs``
    trials come from ``rand.suggest`` with ``startup_stream``: 'numpy' (the
    reference's RandomState stream, default) or 'philox' (device prior
    draws, tpe_plan_sample_prior).

    ``objectives=M`` (multi-objective TPE): the model reads
    ``result['objectives']``, a sequence of M numbers to minimise, from every
    ok trial -- an ok trial without it, or with another length, is a
    ValueError naming the tid -- and the good / bad split ranks the history by
    Pareto dominance (``pareto_ranks``) instead of by ``result['loss']``,
    which ``fmin`` still needs for its own bookkeeping.  Everything behind
    the split is unchanged; with M = 1 and ``objectives = [loss]`` the
    suggestions are those of ``objectives=None``.  Calls with different
    ``objectives`` may alternate on one domain and one trials object.

    ``hypervolume`` (with ``objectives``): the order inside the
    Pareto front, which decides the good side once the front is larger than
    the split, becomes a greedy hypervolume subset selection -- the front
    trial that adds the most hypervolume against a reference point first,
    then the one that adds the most given the first, ... (``hv_picks``), as in
    MOTPE.  ``True``: the default reference point, per objective ``hi + 0.1
    (hi - lo)`` over the finite values of complete trials (``hi + 1`` when
    they are all equal); a sequence of M finite floats: that reference point;
    ``False`` (default): the order of DESIGN 5.17.  Anything else, or
    ``hypervolume`` without ``objectives``, is a ValueError.  With M = 1 the
    setting is ignored."""
    objectives = check_objectives(objectives)
    hypervolume = check_hypervolume(hypervolume, objectives)
    new_ids = list(new_ids)
    if not new_ids:
        return []
    if rng_stream not in ('philox', 'numpy'):
        raise ValueError('rng_stream must be "philox" or "numpy"')
    cs = domain.space
    st = _state(domain)
    with st.lock:
        hist = st.history(domain, trials).sync(trials, objectives, hypervolume)
        startup = hist.n < n_startup_jobs
    if startup:
        # the reference's RandomState prior stream (numpy), or device prior
        # draws with the Philox stream (tpe_plan_sample_prior)
        return rand.suggest(new_ids, domain, trials, seed, rng_stream=startup_stream)
    with st.lock:
        engine = engine or E.default_engine()
        if hist.M != objectives or hist.hv != hypervolume:    # (another thread's call in between)
            hist.sync(trials, objectives, hypervolume)
        plan = st.plan_for(domain, hist.n, engine)
        hist.push(plan)
        seeds = batch_seeds(seed, len(new_ids))
        n_ei = int(n_EI_candidates)
        if rng_stream == 'philox':
            # fit + sample + score + argmax of every suggestion in one call
            res = plan.fit_suggest(seeds, n_ei, gamma=gamma, prior_weight=prior_weight,
                                   lf=DEFAULT_LF)
            picks = _picks(cs, res)
        else:
            plan.fit(gamma=gamma, prior_weight=prior_weight, lf=DEFAULT_LF)
            picks = [_suggest_numpy_stream(cs, plan, sd, n_ei) for sd in seeds]
    return [_new_doc(domain, trials, cs, i, c) for i, c in zip(new_ids, picks)]


def _suggest_numpy_stream(cs, plan, seed, n_ei):
    """Reference RandomState candidate stream; fit + scoring on the GPU."""
    rng = np.random.RandomState(seed)
    chosen = {}
    for lab in cs.draw_order:
        if not cs.is_active(lab, chosen):
            continue
        h = cs.by_label[lab]
        if h.is_categorical:
            p = plan.mixture(h.index, 0)[0]
            cand = rstream.multinomial_draw(rng, p, n_ei).astype(np.float64)
        else:
            t = cs.engine_tables()[0][h.index]
            lg = t.family == E.LGMM
            low = t.low if t.flags & E.HAS_LOW else None
            high = t.high if t.flags & E.HAS_HIGH else None
            q = t.q if t.flags & E.HAS_Q else None
            cand = rstream.posterior_draw(rng, lg, plan.mixture(h.index, 0), low, high, q, n_ei)
        if n_ei == 0:
            continue
        _, _, best, _ = plan.score_candidates(h.index, cand)
        chosen[lab] = _fmt(h, cand[best])
    return chosen


# --------------------------------------------------------------------------
# whole configurations under the fitted model: score_configs / suggest_from_pool
# --------------------------------------------------------------------------
def config_columns(cs, configs):
    """``configs`` as the history's columns: (vals[P, M] float64 in
    ``cs.labels`` order with NaN for absent, present[P, M] bool).  Accepts a
    sequence of ``{label: value}`` dicts (choices as option indices: what fmin
    returns and space_eval takes; absent labels are inactive) or a float array
    [P, M] with NaN for absent."""
    P = len(cs.labels)
    if isinstance(configs, np.ndarray):
        vals = np.ascontiguousarray(configs, dtype=np.float64)
        if vals.ndim != 2 or vals.shape[0] != P:
            raise ValueError('a configuration array must be [%d, M] in domain.space.labels '
                             'order' % P)
        return vals, ~np.isnan(vals)
    configs = list(configs)
    vals = np.full((P, len(configs)), np.nan)
    index = {lab: i for i, lab in enumerate(cs.labels)}
    for j, cfg in enumerate(configs):
        for lab, v in cfg.items():
            i = index.get(lab)
            if i is None:
                raise ValueError('configuration %d: unknown label %r' % (j, lab))
            vals[i, j] = float(v)
    return vals, ~np.isnan(vals)


def columns_to_configs(cs, vals, active):
    """The ``{label: value}`` dicts of the columns' configurations (active
    labels only; categorical values as ints)."""
    vals, active = np.asarray(vals), np.asarray(active).astype(bool)
    vl, al = vals.T.tolist(), active.T.tolist()
    return [{lab: (int(round(v[i])) if cat else v[i]) for lab, i, cat in cs.pick_order if a[i]}
            for v, a in zip(vl, al)]


def active_columns(cs, vals):
    """active[P, M] implied by the configurations' own values, as
    ``CompiledSpace.is_active`` states it: an hp is active iff it has no
    condition, or some condition has its parent active with value == branch
    (vectorised over the configurations; what the engine derives on the
    device)."""
    hps, conds, _ = cs.engine_tables()
    P, M = vals.shape
    act = np.zeros((P, M), dtype=bool)
    done = [False] * P

    def visit(i):
        if done[i]:
            return
        done[i] = True          # (conditions are acyclic: plan_build checks)
        t = hps[i]
        if t.cond_count == 0:
            act[i] = True
            return
        for par, br in conds[t.cond_begin:t.cond_begin + t.cond_count]:
            visit(par)
            act[i] |= act[par] & (vals[par] == float(br))

    for i in range(P):
        visit(i)
    return act


def _check_consistent(cs, present, active):
    """A dict's labels must be exactly the hps its own choices activate."""
    bad = np.argwhere(present != np.asarray(active).astype(bool))
    if len(bad):
        i, j = (int(x) for x in bad[0])
        raise ValueError('configuration %d: label %r is %s, but its choices make it %s'
                         % (j, cs.labels[i], 'present' if present[i, j] else 'missing',
                            'inactive' if present[i, j] else 'active'))


def root_indices(cs):
    """The unconditional hps of a space -- the dimensions of the multivariate
    model -- as indices into ``cs.labels``."""
    return [i for i, h in enumerate(cs.hps) if len(h.conds()) == 0]


def hp_groups(cs):
    """The hps of a space in groups that are always active together -- the
    joint models of ``multivariate='groups'`` -- as a list of label tuples: a
    group is a maximal set of hps with the same set of immediate
    (parent, branch) alternatives (``conds()`` as a set); group 0 holds the
    unconditional hps, the others follow in ascending order of their smallest
    hp index, labels in hp index order.  A label shared by two branches has
    both alternatives and is a group of its own."""
    groups, where = [[]], {frozenset(): 0}
    for h in cs.hps:
        key = frozenset(h.conds())
        if key not in where:
            where[key] = len(groups)
            groups.append([])
        groups[where[key]].append(h.label)
    return [tuple(g) for g in groups]


def _mode(multivariate):
    """``multivariate=`` checked: False (marginal), True (joint over the
    unconditional hps) or 'groups' (one joint model per ``hp_groups`` group)."""
    if isinstance(multivariate, (bool, np.bool_)):
        return bool(multivariate)
    if isinstance(multivariate, str) and multivariate == 'groups':
        return 'groups'
    raise ValueError("multivariate must be False, True or 'groups', got %r" % (multivariate,))


def _fit_for(st, domain, trials, hist, engine, prior_weight, gamma, multivariate=False):
    """Push the history and fit, exactly as ``suggest`` does (st.lock held).
    ``multivariate``: also the joint model over the unconditional hps, which
    every history row must hold (ValueError otherwise); 'groups': the joint
    model of every ``hp_groups`` group, whose hps must be active in exactly
    the same history rows (ValueError otherwise)."""
    multivariate = _mode(multivariate)
    engine = engine or E.default_engine()
    plan = st.plan_for(domain, hist.n, engine)
    hist.push(plan)
    plan.fit(gamma=gamma, prior_weight=prior_weight, lf=DEFAULT_LF)
    if multivariate == 'groups':
        cs = domain.space
        index = {lab: i for i, lab in enumerate(cs.labels)}
        act = np.asarray(hist.active)[:, :hist.n] != 0
        for g, labs in enumerate(hp_groups(cs)):
            if not labs:
                continue
            rows = [index[lab] for lab in labs]
            # the roots against all rows, every other group against its first hp
            want = np.ones(hist.n, dtype=bool) if g == 0 else act[rows[0]]
            bad = np.argwhere((act[rows] != want).T)       # (row, hp) in row order
            if len(bad):
                j, i = (int(x) for x in bad[0])
                if g == 0:
                    raise ValueError('multivariate TPE: history row %d has no value for the '
                                     'unconditional hp %r' % (j, labs[i]))
                raise ValueError('multivariate TPE: in history row %d the hps %r and %r of one '
                                 'group are not active together' % (j, labs[0], labs[i]))
        plan.group_fit()
    elif multivariate:
        roots = root_indices(domain.space)
        act = np.asarray(hist.active)[roots, :hist.n]
        if not act.all():
            i, j = (int(x) for x in np.argwhere(act == 0)[0])
            raise ValueError('multivariate TPE: history row %d has no value for the '
                             'unconditional hp %r' % (j, domain.space.labels[roots[i]]))
        plan.joint_fit()
    return plan


def score_configs(configs, domain, trials, prior_weight=_default_prior_weight,
                  gamma=_default_gamma, engine=None, return_terms=False, multivariate=False,
                  objectives=None, hypervolume=False):
    """What the fitted TPE model thinks of configurations the caller holds.

    The history of ``trials`` is synced, pushed and fitted as ``suggest``
    does; every configuration c is then scored on the device as
    ``EI(c) = sum over its active hps of below_llik(v) - above_llik(v)`` --
    per hp the score the reference's broadcast_best ranks (tpe.py:749-759),
    added in float64 in ``domain.space.labels`` order.  ``configs``: a
    sequence of ``{label: value}`` dicts (absent labels inactive) or a float
    array [P, M] (NaN for absent).  Returns EI[M]; with ``return_terms`` also
    ``{label: term[M]}`` and ``{label: active[M]}``.  Non-finite lpdfs
    propagate (nothing is clamped); an active categorical value that is not
    an option index scores NaN.  ValueError: an empty history, or a dict whose
    labels contradict the activity its own choices imply.

    ``multivariate``: the unconditional hps are scored together under the
    joint Parzen model (one mixture over whole history rows per side, as
    Optuna's ``multivariate=True``), which sees interactions
    between them: ``EI(c) = joint(c) + the conditional hps' terms``.  With
    ``return_terms`` the result is (EI, terms, active, joint[M]); the terms of
    unconditional labels are 0.0.

    ``multivariate='groups'``: every ``hp_groups`` group -- the unconditional
    hps, and the hps of each branch -- is scored under a joint model of its
    own, fitted on the history rows in which the group is active (Optuna's
    ``group=True``), so interactions inside a branch are seen
    too: ``EI(c) = the sum of joint_g(c) over the groups active in c``.  With
    ``return_terms`` the result is (EI, terms, active, joint[G, M]) with
    ``joint`` in ``hp_groups`` order (0.0 where a group is inactive); all
    terms are 0.0.  Any other value of ``multivariate`` is a ValueError.

    ``objectives=M``: the model is fitted on the Pareto ranking of the
    trials' ``result['objectives']`` (``suggest``); ``hypervolume``: with the
    hypervolume order inside the front (``suggest``)."""
    multivariate = _mode(multivariate)
    objectives = check_objectives(objectives)
    hypervolume = check_hypervolume(hypervolume, objectives)
    cs = domain.space
    as_dicts = not isinstance(configs, np.ndarray)
    vals, present = config_columns(cs, configs)
    st = _state(domain)
    with st.lock:
        hist = st.history(domain, trials).sync(trials, objectives, hypervolume)
        if hist.n == 0:
            raise ValueError('score_configs needs a history: trials holds no usable trial')
        plan = _fit_for(st, domain, trials, hist, engine, prior_weight, gamma, multivariate)
        joint = None
        if multivariate == 'groups':
            total, active, joint = plan.group_score_points(vals, want_active=True,
                                                           want_joint=True)
            terms = np.zeros(vals.shape)
        elif multivariate:
            total, terms, active, joint = plan.joint_score_points(
                vals, want_terms=True, want_active=True, want_joint=True)
        else:
            total, terms, active = plan.score_points(vals, want_terms=True, want_active=True)
    if as_dicts:
        _check_consistent(cs, present, active)
    if not return_terms:
        return total
    out = (total, {lab: terms[i] for i, lab in enumerate(cs.labels)},
           {lab: active[i].astype(bool) for i, lab in enumerate(cs.labels)})
    return out + (joint,) if multivariate else out


class _Pool(object):
    """A candidate pool as columns, with its host-derived activity."""

    def __init__(self, cs, pool):
        self.source = pool          # (keeps an array pool alive: the cache key is its identity)
        self.vals, present = config_columns(cs, pool)
        self.active = active_columns(cs, self.vals)
        if not isinstance(pool, np.ndarray):
            _check_consistent(cs, present, self.active)
        self.m = self.vals.shape[1]
        self._dev = None            # (engine, values, totals) device buffers of an array pool

    def totals(self, plan, multivariate=False):
        """EI of every pool configuration under ``plan``'s fit."""
        groups = multivariate == 'groups'
        if not isinstance(self.source, np.ndarray) or self.m == 0:
            return (plan.group_score_points if groups else plan.joint_score_points
                    if multivariate else plan.score_points)(self.vals)
        # an array pool lives on the device: uploaded once, scored in place
        eng = plan.engine
        if self._dev is None or self._dev[0] is not eng:
            self._dev = (eng, E.DeviceBuffer(eng, self.vals.nbytes).upload(self.vals),
                         E.DeviceBuffer(eng, 8 * self.m))
        _, v, out = self._dev
        score = (plan.group_score_points_device if groups else plan.joint_score_points_device
                 if multivariate else plan.score_points_device)
        score(v.ptr, self.m, self.m, out.ptr)
        return out.download(np.empty(self.m))


def _pool_for(st, cs, pool):
    if not isinstance(pool, np.ndarray):
        return _Pool(cs, pool)
    p = getattr(st, 'pool', None)
    if p is None or p.source is not pool:
        p = st.pool = _Pool(cs, pool)
    return p


def _row_keys(vals, active):
    """One opaque key per configuration: its activity and active values
    (inactive slots and the sign of zero do not count)."""
    canon = np.where(active, vals, 0.0) + 0.0
    rows = np.ascontiguousarray(np.concatenate([canon.T, active.T.astype(np.float64)], axis=1))
    return rows.view(np.dtype((np.void, rows.dtype.itemsize * rows.shape[1]))).ravel()


def seen_in_history(pool_vals, pool_active, hist_vals, hist_active):
    """seen[M]: pool configurations whose active values equal those of some
    history row (vectorised over the columns)."""
    if hist_vals.shape[1] == 0 or pool_vals.shape[1] == 0:
        return np.zeros(pool_vals.shape[1], dtype=bool)
    return np.isin(_row_keys(pool_vals, pool_active),
                   _row_keys(hist_vals, np.asarray(hist_active).astype(bool)))


def rank_pool(total, eligible, k):
    """The k eligible pool indices of highest EI: ties to the lower index,
    NaN totals last."""
    idx = np.flatnonzero(eligible)
    t = total[idx]
    nan = np.isnan(t)
    order = np.lexsort((idx, -np.where(nan, 0.0, t), nan))
    return idx[order[:k]]


def suggest_from_pool(new_ids, domain, trials, seed, pool=None,
                      prior_weight=_default_prior_weight,
                      n_startup_jobs=_default_n_startup_jobs,
                      gamma=_default_gamma, skip_seen=True, engine=None, multivariate=False,
                      objectives=None, hypervolume=False):
    """``algo=`` for a constrained or discrete search: the next trials are the
    ``len(new_ids)`` configurations of ``pool`` the fitted model scores
    highest (``score_configs``' EI), distinct, ties to the lower pool index,
    NaN scores last.  Use as ``functools.partial(tpe.suggest_from_pool,
    pool=...)``.  ``pool`` takes ``score_configs``' two formats; an array is
    converted and uploaded once per domain (cached on the array's identity).
    ``skip_seen`` drops pool configurations whose active values equal those of
    a trial already in the history.  While the history has fewer than
    ``n_startup_jobs`` trials the picks are ``np.random.RandomState(seed)
    .choice(M, k, replace=False)`` over the whole pool.  ValueError when fewer
    than ``len(new_ids)`` eligible configurations remain.  ``multivariate``
    (True or 'groups'): the pool is ranked by ``score_configs`` with that
    argument.  ``objectives=M``: the model is fitted on the Pareto ranking of
    the trials' ``result['objectives']`` (``suggest``); ``hypervolume``: with
    the hypervolume order inside the front (``suggest``)."""
    multivariate = _mode(multivariate)
    objectives = check_objectives(objectives)
    hypervolume = check_hypervolume(hypervolume, objectives)
    new_ids = list(new_ids)
    if not new_ids:
        return []
    if pool is None:
        raise TypeError('suggest_from_pool needs pool=')
    cs = domain.space
    st = _state(domain)
    k = len(new_ids)
    with st.lock:
        pl = _pool_for(st, cs, pool)
        hist = st.history(domain, trials).sync(trials, objectives, hypervolume)
        if hist.n < n_startup_jobs:
            if pl.m < k:
                raise ValueError('the pool holds %d configurations, %d asked for' % (pl.m, k))
            picks = np.random.RandomState(seed).choice(pl.m, k, replace=False)
        else:
            eligible = np.ones(pl.m, dtype=bool)
            if skip_seen:
                eligible &= ~seen_in_history(pl.vals, pl.active, hist.vals[:, :hist.n],
                                             hist.active[:, :hist.n])
            if int(eligible.sum()) < k:
                raise ValueError('%d eligible pool configurations remain, %d asked for'
                                 % (int(eligible.sum()), k))
            plan = _fit_for(st, domain, trials, hist, engine, prior_weight, gamma, multivariate)
            picks = rank_pool(pl.totals(plan, multivariate), eligible, k)
    chosen = columns_to_configs(cs, pl.vals[:, picks], pl.active[:, picks])
    return [_new_doc(domain, trials, cs, i, c) for i, c in zip(new_ids, chosen)]


# --------------------------------------------------------------------------
# whole configurations drawn from the fitted model: sample_configs / suggest_joint
# --------------------------------------------------------------------------
_default_n_configs = 4096
TOPK_MAX = 4096             # tpe_plan_topk_points' largest k
STARTUP_ROUNDS = 100        # suggest_joint's prior rounds under a predicate


def sample_configs(n, domain, trials, seed, prior_weight=_default_prior_weight,
                   gamma=_default_gamma, engine=None, begin=0, as_dicts=False,
                   multivariate=False, objectives=None, hypervolume=False):
    """``n`` whole configurations drawn from the fitted model's *below*
    mixtures, each with its joint EI (``score_configs``' total of it).

    The history is synced, pushed and fitted as ``suggest`` does; the device
    then draws every configuration parents first -- a conditional hp only
    under the branch drawn for its parent -- and scores it
    (tpe_plan_sample_points).  Configuration j is draw ``begin + j`` of the
    Philox key ``batch_seeds(seed, 1)[0]``, so calls that split a range give
    the numbers of one call.  Returns (vals[P, n] in ``domain.space.labels``
    order with NaN for inactive -- a pool array -- , ei[n]); with ``as_dicts``
    the configurations as ``{label: value}`` dicts instead.  ValueError on an
    empty history.

    ``multivariate``: every configuration picks one component of the joint
    below model -- the prior or one good trial -- and draws all its
    unconditional hps from that component's kernels, so they keep the good
    trials' correlations; the EI is ``score_configs(..., multivariate=True)``'s
    (tpe_plan_joint_sample_points).  ``multivariate='groups'``: every group
    the configuration activates picks a component of its own below model and
    draws the group's hps from it, parents first; the EI is
    ``score_configs(..., multivariate='groups')``'s
    (tpe_plan_group_sample_points).  ``objectives=M``: the model is fitted on
    the Pareto ranking of the trials' ``result['objectives']`` (``suggest``);
    ``hypervolume``: with the hypervolume order inside the front (``suggest``)."""
    multivariate = _mode(multivariate)
    objectives = check_objectives(objectives)
    hypervolume = check_hypervolume(hypervolume, objectives)
    cs = domain.space
    st = _state(domain)
    with st.lock:
        hist = st.history(domain, trials).sync(trials, objectives, hypervolume)
        if hist.n == 0:
            raise ValueError('sample_configs needs a history: trials holds no usable trial')
        plan = _fit_for(st, domain, trials, hist, engine, prior_weight, gamma, multivariate)
        draw = (plan.group_sample_points if multivariate == 'groups' else
                plan.joint_sample_points if multivariate else plan.sample_points)
        vals, total = draw(batch_seeds(seed, 1)[0], int(n), begin=int(begin))
    if as_dicts:
        return columns_to_configs(cs, vals, ~np.isnan(vals)), total
    return vals, total


def _joint_walk(keys, seen, k, complete):
    """suggest_joint's selection over configurations in rank order: ``keys``
    their row keys, ``seen`` those equal to a history row.  Accept a
    configuration unless it is seen or equals an accepted one, until ``k``
    are accepted; when the walk ends short, fill from the rejected duplicates
    of accepted ones in rank order.  Returns the picked positions; None when
    short and the walk was over a prefix only (``complete`` False); ValueError
    when short over all of them."""
    picks, dups, taken = [], [], set()
    for j in range(len(keys)):
        if seen[j]:
            continue
        kb = keys[j].tobytes()
        if kb in taken:
            dups.append(j)
            continue
        taken.add(kb)
        picks.append(j)
        if len(picks) == k:
            return picks
    if not complete:
        return None
    picks += dups[:k - len(picks)]
    if len(picks) < k:
        raise ValueError('the draw holds %d selectable configurations, %d asked for'
                         % (len(picks), k))
    return picks


def joint_select(total, eligible, vals, hist_vals, hist_active, k, skip_seen=True):
    """The indices ``suggest_joint`` picks from drawn configurations
    ``vals[P, n]`` (NaN for inactive) with EI ``total[n]``: the eligible ones
    walked in ``rank_pool`` order under ``_joint_walk``'s rule, equality
    being ``_row_keys``' (active values; the sign of zero does not count)."""
    n = vals.shape[1]
    eligible = np.ones(n, dtype=bool) if eligible is None else np.asarray(eligible, dtype=bool)
    order = rank_pool(np.asarray(total), eligible, n)
    v = vals[:, order]
    act = ~np.isnan(v)
    seen = (seen_in_history(v, act, hist_vals, hist_active) if skip_seen
            else np.zeros(order.size, dtype=bool))
    return order[_joint_walk(_row_keys(v, act), seen, k, True)]


def _feasible_mask(feasible, cs, vals):
    """``feasible({label: column[n]})`` checked: a bool array [n]."""
    n = vals.shape[1]
    r = feasible({lab: vals[i] for i, lab in enumerate(cs.labels)})
    r = np.asarray(r)
    if r.dtype != np.bool_ or r.shape != (n,):
        raise ValueError('feasible must return a bool array of shape (%d,), got %s %s'
                         % (n, r.dtype, r.shape))
    return r


def _joint_startup(new_ids, domain, trials, seed, feasible, startup_stream):
    """Prior rounds of len(new_ids) draws until enough satisfy ``feasible``."""
    cs = domain.space
    k = len(new_ids)
    kept = []
    for r in range(STARTUP_ROUNDS):
        sd = batch_seeds(seed, r + 1)[r]
        if startup_stream == 'numpy' and r > 0:
            sd %= 2 ** 32       # (RandomState takes 32 bits; round 0 is ``seed`` as given)
        docs = rand.suggest(new_ids, domain, trials, sd, rng_stream=startup_stream)
        cfgs = [{lab: v[0] for lab, v in d['misc']['vals'].items() if v} for d in docs]
        ok = _feasible_mask(feasible, cs, config_columns(cs, cfgs)[0])
        kept += [c for c, good in zip(cfgs, ok) if good]
        if len(kept) >= k:
            return [_new_doc(domain, trials, cs, i, c) for i, c in zip(new_ids, kept)]
    raise ValueError('%d prior rounds gave %d feasible configurations, %d asked for'
                     % (STARTUP_ROUNDS, len(kept), k))


def _joint_buffers(st, engine, P, n):
    """The device arrays of a joint draw, kept per domain: values [P, n],
    totals [n], mask [n], picks [TOPK_MAX] and their columns [P, TOPK_MAX]."""
    b = getattr(st, 'joint', None)
    if b is None or b[0] is not engine or b[1] != (P, n):
        mk = lambda nbytes: E.DeviceBuffer(engine, nbytes)   # noqa: E731
        b = st.joint = (engine, (P, n), mk(8 * P * n), mk(8 * n), mk(n), mk(4 * TOPK_MAX),
                        mk(8 * P * TOPK_MAX))
    return b[2:]


PENDING_RERUNS = 3          # suggest_joint(batch='pending'): reruns before the full host mask


def _pending_batch(plan, k, bufs, shape, vals, eligible, hv, ha, skip_seen):
    """suggest_joint's ``batch='pending'`` selection over the draw in
    ``bufs``: the columns [P, k] of the greedy picks.  ``skip_seen`` means the
    greedy selection over the configurations that are not history rows: the
    picks of a run are checked against the history on the host, the ones that
    are history rows masked and the selection rerun -- a round's argmax over a
    superset that lies in the subset is the subset's argmax, so a run without
    a history row among its picks is the selection over the subset -- and
    after ``PENDING_RERUNS`` reruns every history row of the draw is masked."""
    d_vals, d_mask, d_idx, d_cols = bufs
    P, n = shape
    mask = None if eligible is None else np.array(eligible, dtype=bool)
    for run in range(PENDING_RERUNS + 2):
        if run == PENDING_RERUNS + 1:
            # the full host mask: every configuration of the draw that is a history row
            if vals is None:
                vals = d_vals.download(np.empty((P, n)))
            mask = (np.ones(n, dtype=bool) if mask is None else mask) & \
                ~seen_in_history(vals, ~np.isnan(vals), hv, ha)
        if mask is not None:
            d_mask.upload(mask.astype(np.uint8))
        plan.group_batch_points_device(d_vals.ptr, n, n, k, d_idx.ptr,
                                       eligible_ptr=0 if mask is None else d_mask.ptr)
        plan.gather_points(d_vals.ptr, d_idx.ptr, k=k, ld=n, out=d_cols.ptr)
        cols = d_cols.download(np.empty((P, k)))
        if not skip_seen:
            return cols
        seen = seen_in_history(cols, ~np.isnan(cols), hv, ha)
        if not seen.any():
            return cols
        picks = d_idx.download(np.empty(k, dtype=np.int32))
        if mask is None:
            mask = np.ones(n, dtype=bool)
        mask[picks[seen]] = False
    raise AssertionError('a history row was picked under the full mask')


def suggest_joint(new_ids, domain, trials, seed, n_configs=_default_n_configs, feasible=None,
                  skip_seen=True, prior_weight=_default_prior_weight,
                  n_startup_jobs=_default_n_startup_jobs, gamma=_default_gamma,
                  startup_stream='numpy', engine=None, multivariate=False, batch='topk',
                  objectives=None, hypervolume=False):
    """``algo=`` that ranks whole configurations: one fit, one draw of
    ``n_configs`` configurations from the fitted model (``sample_configs``)
    and the ``len(new_ids)`` distinct ones of highest joint EI -- a branch is
    ranked together with the children it activates, a batch is the k best of
    one draw.  Use as ``functools.partial(tpe.suggest_joint, ...)``.

    ``feasible``: a predicate over the whole draw, called once as
    ``feasible({label: column[n_configs]})`` (NaN where inactive); it must
    return a bool array [n_configs], and only configurations it accepts are
    picked.  Selection: the eligible configurations in ``rank_pool`` order
    (highest EI first, ties to the lower draw index, NaN last); one is taken
    unless its active values equal those of one already taken or, with
    ``skip_seen``, of a history row; when fewer than k remain, duplicates of
    taken ones fill the rest in rank order; ValueError when that is short
    too.  The ranking and the gather run on the device (tpe_plan_topk_points,
    tpe_plan_gather_points) over a few multiples of k, with the full host
    ranking behind them when duplicates exhaust those.

    While the history has fewer than ``n_startup_jobs`` trials the documents
    come from ``rand.suggest`` as in ``suggest``; under ``feasible``, from
    rounds of it with seeds ``batch_seeds(seed, r + 1)[r]`` (the 'numpy'
    stream takes their low 32 bits from round 1 on: RandomState holds no
    more), the feasible draws kept in order (at most 100 rounds, else
    ValueError).

    ``multivariate``: the draw and its ranking are
    ``sample_configs``' with that argument (True or 'groups'); everything
    else is as above.

    ``batch='pending'`` (with ``multivariate='groups'``) spreads a
    batch for parallel workers: the k best of one draw are near-duplicates of
    each other, so the picks are made greedily instead -- each pick counts as
    a bad trial that is out for evaluation (the constant liar), joins the
    above model of every group it activates as a pending component, and the
    draw is rescored before the next pick (tpe_plan_group_batch_points).  The
    first pick is ``batch='topk'``'s first.  Configurations equal to a taken
    one rank below all others instead of being dropped, and with
    ``skip_seen`` the selection runs over the configurations that are not
    history rows; ValueError when fewer than k selectable ones remain, for
    k > 1024, for any other ``multivariate`` (the marginal terms of False and
    True hold no per-configuration above density a pending component could
    join; without conditions 'groups' is True's model bit for bit) and for an
    unknown ``batch``.

    ``objectives=M``: the model is fitted on the Pareto ranking of the
    trials' ``result['objectives']`` (``suggest``); ``hypervolume``: with the
    hypervolume order inside the front (``suggest``)."""
    multivariate = _mode(multivariate)
    objectives = check_objectives(objectives)
    hypervolume = check_hypervolume(hypervolume, objectives)
    if batch not in ('topk', 'pending'):
        raise ValueError("batch must be 'topk' or 'pending', got %r" % (batch,))
    if batch == 'pending' and multivariate != 'groups':
        raise ValueError("batch='pending' needs multivariate='groups': only the group models "
                         "hold an above density per configuration that a pending trial can "
                         "join, got multivariate=%r" % (multivariate,))
    new_ids = list(new_ids)
    if not new_ids:
        return []
    cs = domain.space
    st = _state(domain)
    k = len(new_ids)
    n = int(n_configs)
    with st.lock:
        hist = st.history(domain, trials).sync(trials, objectives, hypervolume)
        startup = hist.n < n_startup_jobs
    if startup:
        if feasible is None:
            return rand.suggest(new_ids, domain, trials, seed, rng_stream=startup_stream)
        return _joint_startup(new_ids, domain, trials, seed, feasible, startup_stream)
    if n < k:
        raise ValueError('n_configs = %d configurations drawn, %d asked for' % (n, k))
    P = len(cs.labels)
    with st.lock:
        if hist.M != objectives or hist.hv != hypervolume:    # (another thread's call in between)
            hist.sync(trials, objectives, hypervolume)
        plan = _fit_for(st, domain, trials, hist, engine, prior_weight, gamma, multivariate)
        d_vals, d_total, d_mask, d_idx, d_cols = _joint_buffers(st, plan.engine, P, n)
        draw = (plan.group_sample_points_device if multivariate == 'groups' else
                plan.joint_sample_points_device if multivariate else plan.sample_points_device)
        draw(batch_seeds(seed, 1)[0], 0, n, n, d_vals.ptr, d_total.ptr)
        vals = eligible = None
        n_el = n
        if feasible is not None:
            vals = d_vals.download(np.empty((P, n)))
            eligible = _feasible_mask(feasible, cs, vals)
            d_mask.upload(eligible.astype(np.uint8))
            n_el = int(eligible.sum())
        hv, ha = hist.vals[:, :hist.n], hist.active[:, :hist.n]
        chosen = None
        kk = min(n_el, TOPK_MAX, max(4 * k, 64))
        if batch == 'pending':
            chosen = _pending_batch(plan, k, (d_vals, d_mask, d_idx, d_cols), (P, n), vals,
                                    eligible, hv, ha, skip_seen)
        elif k <= kk:
            plan.topk_points(d_total.ptr, kk, eligible=None if eligible is None else d_mask.ptr,
                             m=n, out=d_idx.ptr)
            plan.gather_points(d_vals.ptr, d_idx.ptr, k=kk, ld=n, out=d_cols.ptr)
            cols = d_cols.download(np.empty((P, kk)))
            act = ~np.isnan(cols)
            seen = (seen_in_history(cols, act, hv, ha) if skip_seen
                    else np.zeros(kk, dtype=bool))
            pos = _joint_walk(_row_keys(cols, act), seen, k, kk == n_el)
            if pos is not None:
                chosen = cols[:, pos]
        if chosen is None:
            # duplicates exhausted the device's picks: the rule over the whole draw
            if vals is None:
                vals = d_vals.download(np.empty((P, n)))
            total = d_total.download(np.empty(n))
            chosen = vals[:, joint_select(total, eligible, vals, hv, ha, k, skip_seen)]
    cfgs = columns_to_configs(cs, chosen, ~np.isnan(chosen))
    return [_new_doc(domain, trials, cs, i, c) for i, c in zip(new_ids, cfgs)]


# --------------------------------------------------------------------------
# multi-objective TPE: the Pareto ranking the split reads
# --------------------------------------------------------------------------
def _pareto(domain, trials, objectives, engine, hypervolume=False, want_hv=False):
    """(docs, tids, dominated_by, dominates, surrogate) of the synced history,
    ranked on the device; ``want_hv``: and ``Plan.hv_get``'s tuple."""
    objectives = check_objectives(objectives)
    if objectives is None:
        raise ValueError('the Pareto ranking needs objectives=M')
    hypervolume = check_hypervolume(hypervolume, objectives)
    st = _state(domain)
    none = (np.zeros(0, dtype=np.int32), np.zeros(0), np.zeros(0, dtype=np.int32), 0)
    with st.lock:
        hist = st.history(domain, trials).sync(trials, objectives, hypervolume)
        if hist.n == 0:
            out = [], [], np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0)
            return out + (none,) if want_hv else out
        plan = st.plan_for(domain, hist.n, engine or E.default_engine())
        hist.push(plan)
        out = (list(hist.docs), list(hist.tids)) + plan.pareto_get(hist.n)
        return out + (plan.hv_get(),) if want_hv else out


def pareto_ranks(domain, trials, objectives, engine=None, hypervolume=False):
    """(tids, dominated_by, dominates, surrogate) of the history of
    ``trials`` under ``objectives=M``, read back from the device
    (tpe_plan_pareto_get): per trial in tid order the number of complete
    trials that dominate it (0: on the Pareto front), the number it
    dominates, and the surrogate loss ``dominated_by (n + 1) + (n -
    dominates)`` the split ranks by; a trial that is not ok, or has a NaN or
    +inf objective, is pending: counts 0 and surrogate +inf.  With
    ``hypervolume`` the surrogate of a front trial is its place in the
    hypervolume subset selection (``suggest``, ``hv_picks``); the selection's
    sample seed is fixed, so the ranks are a function of the history alone."""
    return _pareto(domain, trials, objectives, engine, hypervolume)[1:]


def pareto_front(domain, trials, objectives, engine=None, hypervolume=False):
    """The trial documents on the Pareto front of ``result['objectives']``
    -- complete trials no complete trial dominates -- in tid order
    (``hypervolume`` orders the front's rows in the split and leaves the front
    as it is)."""
    docs, _, by, _, s = _pareto(domain, trials, objectives, engine, hypervolume)
    return [docs[r] for r in np.flatnonzero((by == 0) & np.isfinite(s))]


def hv_picks(domain, trials, objectives, hypervolume=True, engine=None):
    """(tids, gains, alive) of the hypervolume subset selection inside the
    Pareto front of ``trials`` (tpe_plan_hv_get), in pick order:
    the tids picked, what each added to the hypervolume given the picks
    before it -- the exact area with two objectives, the Monte-Carlo estimate
    ``vol * alive / S`` with more -- and its alive samples (-1: exact).  At most
    32 picks; fewer when the front inside the reference point is smaller;
    none with ``objectives=1``, ``hypervolume=False`` or no complete trial."""
    _, tids, _, _, _, (picks, keys, counts, R) = _pareto(domain, trials, objectives, engine,
                                                       hypervolume, want_hv=True)
    picks, keys, counts = picks[:R], keys[:R].copy(), counts[:R]
    mc = counts >= 0
    keys[mc] = keys[mc] / float(HV_N_SAMPLES)
    return [tids[int(r)] for r in picks], keys, counts


# --------------------------------------------------------------------------
# operator-level drop-ins for the reference's scope functions (GPU-backed)
# --------------------------------------------------------------------------
def _eng():
    return E.default_engine()


def ap_filter_trials(o_idxs, o_vals, l_idxs, l_vals, gamma, gamma_cap=DEFAULT_LF):
    """tpe.py:613-641; ties in the loss ranking broken by position."""
    l_idxs = np.asarray(l_idxs)
    mask = _eng().split(np.asarray(l_vals, dtype=np.float64), gamma, gamma_cap)
    good = set(l_idxs[mask].tolist())
    bad = set(l_idxs[~mask].tolist())
    below = [v for i, v in zip(o_idxs, o_vals) if i in good]
    above = [v for i, v in zip(o_idxs, o_vals) if i in bad]
    return np.asarray(below), np.asarray(above)


def linear_forgetting_weights(N, LF):
    """tpe.py:381-394 (host: trivial)."""
    assert N >= 0 and LF > 0
    if N == 0:
        return np.asarray([])
    if N < LF:
        return np.ones(N)
    return np.concatenate([np.linspace(1.0 / N, 1.0, num=N - LF), np.ones(LF)], axis=0)


def adaptive_parzen_normal(mus, prior_weight, prior_mu, prior_sigma, LF=DEFAULT_LF):
    """tpe.py:398-475 on the GPU (stable sort for tied observations)."""
    mus = np.asarray(mus, dtype=np.float64)
    if mus.ndim != 1:
        raise TypeError('mus must be vector', mus)
    return _eng().parzen_fit(mus, prior_weight, prior_mu, prior_sigma, LF)


def _opt(v):
    return None if v is None else float(v)


def GMM1_lpdf(samples, weights, mus, sigmas, low=None, high=None, q=None):
    """tpe.py:104-166 on the GPU."""
    w, m, s = (np.asarray(a, dtype=np.float64) for a in (weights, mus, sigmas))
    for a, nm in ((w, 'weights'), (m, 'mus'), (s, 'sigmas')):
        if a.ndim != 1:
            raise TypeError('need vector of %s' % nm, a.shape)
    x = np.asarray(samples, dtype=np.float64)
    if x.size == 0:
        return np.asarray([])
    return _eng().lpdf(E.GMM, x, w, m, s, _opt(low), _opt(high), _opt(q))


def LGMM1_lpdf(samples, weights, mus, sigmas, low=None, high=None, q=None):
    """tpe.py:259-301 on the GPU."""
    w, m, s = (np.asarray(a, dtype=np.float64) for a in (weights, mus, sigmas))
    x = np.asarray(samples, dtype=np.float64)
    if x.size == 0:
        return np.asarray([]).reshape(x.shape)
    return _eng().lpdf(E.LGMM, x, w, m, s, _opt(low), _opt(high), _opt(q))


def categorical_lpdf(sample, p, upper=None):
    """tpe.py:50-57 on the GPU."""
    sample = np.asarray(sample)
    if sample.size == 0:
        return np.asarray([])
    p = np.asarray(p, dtype=np.float64)
    return _eng().lpdf(E.CAT, sample.astype(np.float64), p)


def broadcast_best(samples, below_llik, above_llik):
    """tpe.py:749-759 (argmax with numpy semantics)."""
    if len(samples):
        score = np.asarray(below_llik) - np.asarray(above_llik)
        if len(samples) != len(score):
            raise ValueError()
        best = int(np.argmax(score))
        return [samples[best]] * len(samples)
    return []


def GMM1(weights, mus, sigmas, low=None, high=None, q=None, rng=None, size=()):
    """tpe.py:62-93: Philox draws on the GPU, seeded from ``rng``."""
    return _draw(E.GMM, weights, mus, sigmas, low, high, q, rng, size)


def LGMM1(weights, mus, sigmas, low=None, high=None, q=None, rng=None, size=()):
    """tpe.py:216-250: Philox draws on the GPU, seeded from ``rng``."""
    return _draw(E.LGMM, weights, mus, sigmas, low, high, q, rng, size)


def _draw(family, weights, mus, sigmas, low, high, q, rng, size):
    n = int(np.prod(size)) if size != () else 1
    seed = int(rng.randint(2 ** 31 - 1)) if rng is not None else int(np.random.randint(2 ** 31 - 1))
    if (low is None) != (high is None):
        raise TypeError('one-sided truncation is not supported (tpe.py:76)')
    out = _eng().sample(family, weights, mus, sigmas, _opt(low), _opt(high), _opt(q), seed=seed,
                        n=n)
    return out.reshape(size) if size != () else out[0]
