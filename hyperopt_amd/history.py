"""Columnar trial history of one (Domain, Trials) pair, synced incrementally
to the engine.

The reference re-assembles the history from every trial document on every
``tpe.suggest`` (tpe.py:820-848 plus ``miscs_to_idxs_vals``, base.py:187-202)
and hands it to numpy.  Here the history is kept as columns -- per-trial
losses, per-hyperparameter values and activity -- that are extended as
trials arrive: a sync reads only the documents appended to the visible list
and the ones the store's change journal names, and ``push`` copies only the
changed rows to the plan's device-resident history
(``tpe_plan_update_history``).

Semantics are the reference's: the loss of a trial is ``domain.loss(result,
spec)`` with None -> +inf; documents sharing a tid (``misc.from_tid``) keep
the one of lowest loss (the later one on ties); a tid whose first document
has a NaN loss is dropped; rows are in tid order; an observation counts for
a trial when its misc idxs entry equals the trial's (from_tid-aware) tid.
A history that is a plain extension (new integer tids in increasing order,
no from_tid) takes the incremental path; anything else rebuilds the columns
from cached per-document rows.

With ``objectives=M`` (multi-objective TPE) an objective store ``Y[M][cap]``
is kept beside the losses, from ``result['objectives']`` of the ok trials, and
``push`` has the device rank the history by Pareto dominance
(``tpe_plan_set_objectives``) instead of sending the losses.  With
``hypervolume=`` the nondominated rows are ordered by a greedy hypervolume
subset selection against a reference point (``tpe_plan_set_hv``).
"""
from __future__ import annotations

import math
import numbers
import weakref

import numpy as np

from .status import STATUS_OK

MAX_OBJ = 8                     # include/tpe_engine.h TPE_MAX_OBJ


def _loss_of(domain, doc):
    v = domain.loss(doc['result'], doc['spec'])
    return math.inf if v is None else float(v)


def check_objectives(objectives):
    """``objectives=`` checked: None (the scalar loss) or the number M >= 1 of
    objectives every ok trial reports in ``result['objectives']``."""
    if objectives is None:
        return None
    if isinstance(objectives, bool) or not isinstance(objectives, numbers.Integral) \
            or not 1 <= objectives <= MAX_OBJ:
        raise ValueError('objectives must be None or an int in [1, %d], got %r'
                         % (MAX_OBJ, objectives))
    return int(objectives)


def check_hypervolume(hypervolume, objectives):
    """``hypervolume=`` checked against the checked ``objectives``: False (off,
    the default), True (the default reference point, ``default_reference``) or
    a tuple of M finite floats, the reference point of the hypervolume subset
    selection inside the Pareto front."""
    if hypervolume is False:
        return False
    if objectives is None:
        raise ValueError('hypervolume needs objectives=M')
    if hypervolume is True:
        return True
    if isinstance(hypervolume, (str, bytes)):
        raise ValueError('hypervolume must be False, True or a sequence of %d finite numbers, '
                         'got %r' % (objectives, hypervolume))
    try:
        ref = tuple(hypervolume)
        ok = len(ref) == objectives and all(
            isinstance(v, numbers.Real) and not isinstance(v, bool) and math.isfinite(v)
            for v in ref)
    except TypeError:
        ok = False
    if not ok:
        raise ValueError('hypervolume must be False, True or a sequence of %d finite numbers, '
                         'got %r' % (objectives, hypervolume))
    return tuple(float(v) for v in ref)


def default_reference(Y):
    """The default reference point of ``Y[M, n]``: per objective, over the
    finite values of complete rows (no NaN, no +inf), ``hi + 0.1 (hi - lo)``, or
    ``hi + 1`` when ``hi == lo``.  None without a complete row."""
    Y = np.asarray(Y, dtype=np.float64)
    ok = ~(np.isnan(Y) | (Y == np.inf)).any(axis=0)
    if not ok.any():
        return None
    ref = []
    for m in range(Y.shape[0]):
        v = Y[m, ok]
        v = v[np.isfinite(v)]
        if len(v) == 0:                 # (every complete row holds -inf here)
            ref.append(1.0)
            continue
        hi, lo = float(v.max()), float(v.min())
        ref.append(hi + 1.0 if hi == lo else hi + 0.1 * (hi - lo))
    return tuple(ref)


# tpe_plan_set_hv's defaults (include/tpe_engine.h)
HV_N_PICK, HV_N_SAMPLES, HV_SEED, HV_METHOD = 32, 1024, 0, 0


def _objectives_of(doc, M, tid):
    """The M objectives of a row's document: those of an ok trial, NaN (a
    pending row) for any other."""
    res = doc['result']
    if res.get('status') != STATUS_OK:
        return np.full(M, np.nan)
    y = res.get('objectives')
    try:
        ok = y is not None and len(y) == M
    except TypeError:
        ok = False
    if not ok:
        raise ValueError("trial %r: result['objectives'] must be a sequence of %d numbers, got %r"
                         % (tid, M, y))
    return np.array([float(v) for v in y])


def _is_int_tid(t):
    return isinstance(t, numbers.Integral) and not isinstance(t, bool)


class TrialHistory(object):
    """losses[n], vals[P][n], active[P][n] in tid order (host columns with a
    row capacity; ``self.vals[:, :self.n]`` etc. are the live part)."""

    def __init__(self, domain):
        self.domain = domain
        self.labels = list(domain.space.labels)
        self.P = len(self.labels)
        self._cache = {}        # id(doc) -> (doc, tid, vals row, active row)
        self.M = None           # objectives of the last sync (None: the scalar loss)
        self.Y = None           # [M][cap] objective store beside losses (NaN: pending)
        self.hv = False         # hypervolume= of the last sync: False, True or the reference point
        self._alloc(64)
        self._forget()

    # -- storage -------------------------------------------------------------
    def _alloc(self, cap):
        self.cap = cap
        self.losses = np.zeros(cap)
        self.vals = np.zeros((self.P, cap))
        self.active = np.zeros((self.P, cap), dtype=np.uint8)

    def _grow(self, need):
        if need <= self.cap:
            return
        cap = self.cap
        while cap < need:
            cap *= 2
        l, v, a = self.losses, self.vals, self.active
        self._alloc(cap)
        self.losses[:self.n] = l[:self.n]
        self.vals[:, :self.n] = v[:, :self.n]
        self.active[:, :self.n] = a[:, :self.n]
        if self.Y is not None:
            y = self.Y
            self.Y = np.full((y.shape[0], cap), np.nan)
            self.Y[:, :self.n] = y[:, :self.n]

    def _forget(self):
        """Drop all rows: the next sync rebuilds from the documents."""
        self.n = 0
        self.tids = []
        self.docs = []          # the document of each row
        self._row = {}          # id(doc) -> row (incremental mode)
        self._dropped = {}      # id(doc) -> (doc, its loss then): visible documents without a row
        self._pending = set()   # rows with loss +inf (new / running / failed)
        self._owner = None      # weakref to the Trials synced
        self._epoch = None
        self._jgen = None
        self._jpos = 0
        self._seen = 0          # visible documents consumed
        self._vals_dirty = 0    # rows >= this differ from the device copy
        self._loss_dirty = 0
        self._obj_ok = False    # Y holds the objectives of every row not in _touched
        self._touched = set()   # rows whose document was (re)read since Y was
        self._obj_dirty = 0     # rows of Y >= this differ from the device copy
        # what the device loss column holds: None the losses, M a ranking, (M, hv) a
        # ranking with the hypervolume order inside the front
        self._dev_mode = None
        self._dev = None        # weakref to the plan holding the device copy
        self._plain = True      # rows == visible documents, integer tids ascending

    # -- per-document rows -----------------------------------------------------
    def _extract(self, doc):
        """(tid, vals row, active row) of a document, cached per object."""
        key = id(doc)
        hit = self._cache.get(key)
        if hit is not None and hit[0] is doc:
            return hit[1], hit[2], hit[3]
        misc = doc['misc']
        tid = misc.get('from_tid', doc['tid'])
        v = np.zeros(self.P)
        a = np.zeros(self.P, dtype=np.uint8)
        ix, vx = misc['idxs'], misc['vals']
        for i, lab in enumerate(self.labels):
            t = ix[lab]
            if t and t[0] == tid:
                v[i] = float(vx[lab][0])
                a[i] = 1
        self._cache[key] = (doc, tid, v, a)
        return tid, v, a

    def _put_row(self, r, tid, loss, v, a, doc):
        self.losses[r] = loss
        self.vals[:, r] = v
        self.active[:, r] = a
        if r == len(self.docs):
            self.docs.append(doc)
            self.tids.append(tid)
        else:
            self.docs[r] = doc
            self.tids[r] = tid
        if loss == math.inf:
            self._pending.add(r)
        else:
            self._pending.discard(r)
        self._touched.add(r)

    # -- sync ----------------------------------------------------------------
    def sync(self, trials, objectives=None, hypervolume=False):
        """Bring the columns up to date with ``trials.trials``.  ``objectives``
        = M: also the objective store ``Y[M][cap]``, from every ok trial's
        ``result['objectives']`` (ValueError naming the tid where an ok trial
        has none, or not M of them); ``push`` then ranks the device history by
        Pareto dominance instead of by the loss.  ``hypervolume``: the front
        is ordered by hypervolume subset selection (``check_hypervolume``)."""
        objectives = check_objectives(objectives)
        self.hv = check_hypervolume(hypervolume, objectives)
        view = trials.trials
        store = getattr(trials, '_store', None)
        journal = store.journal if store is not None else None
        # snapshot the journal (list, then gen: see _Journal.reset); entries
        # logged after the snapshot are read by the next sync
        jdocs = journal.docs if journal is not None else None
        jgen = journal.gen if journal is not None else None
        jlen = len(jdocs) if jdocs is not None else 0
        fresh = jgen is not None and jgen == self._jgen
        changed = jdocs[self._jpos:jlen] if fresh else []
        if fresh:
            for doc in changed:
                self._cache.pop(id(doc), None)  # misc / tid may have changed
        else:
            self._cache.clear()             # unknown changes: nothing cached is trusted
        same = (fresh and self._plain and self._owner is not None and
                self._owner() is trials and
                getattr(trials, '_epoch', None) == self._epoch and len(view) >= self._seen)
        if not (same and self._incremental(view, changed)):
            self._rebuild(view)
        self._owner = weakref.ref(trials)
        self._epoch = getattr(trials, '_epoch', None)
        self._jgen = jgen
        self._jpos = jlen if fresh else 0
        self._seen = len(view)
        self._sync_objectives(objectives)
        return self

    def _sync_objectives(self, M):
        """The objective store after the columns: the rows read since the last
        sync when that one kept a store of M objectives too, every row
        otherwise (a rebuild, a first call, another M, a call without
        objectives in between)."""
        self.M = M
        if M is None:
            self._obj_ok = False
            self._touched.clear()
            return
        full = not self._obj_ok or self.Y is None or self.Y.shape != (M, self.cap)
        if full:
            self.Y = np.full((M, self.cap), np.nan)
        rows = range(self.n) if full else sorted(r for r in self._touched if r < self.n)
        self._obj_ok = False        # (until every row is read: an error leaves a full re-read)
        for r in rows:
            self.Y[:, r] = _objectives_of(self.docs[r], M, self.tids[r])
        self._obj_dirty = 0 if full else min([self._obj_dirty] + list(rows))
        self._touched.clear()
        self._obj_ok = True

    def _incremental(self, view, changed):
        """Apply changed and appended documents; False = needs a rebuild."""
        dom = self.domain
        done = set()
        for doc in changed:
            k = id(doc)
            if k in done:
                continue
            done.add(k)
            if k in self._dropped and self._dropped[k][0] is doc:
                # a visible document the last rebuild left out (a first NaN
                # loss, or a duplicate tid that lost the dedupe) changed: it
                # may belong in the history now
                return False
            r = self._row.get(k)
            if r is None or self.docs[r] is not doc:
                continue                        # not a row (yet): appended below
            tid, v, a = self._extract(doc)
            loss = _loss_of(dom, doc)
            if tid != self.tids[r] or loss != loss:
                return False
            if not (np.array_equal(v, self.vals[:, r]) and np.array_equal(a, self.active[:, r])):
                self._vals_dirty = min(self._vals_dirty, r)
            if loss != self.losses[r]:
                self._loss_dirty = min(self._loss_dirty, r)
            self._put_row(r, tid, loss, v, a, doc)
        # safety net for results mutated in place (no journal entry): the
        # losses of every row still waiting for one (+inf) are re-read, and
        # those of every document the last rebuild left out (a NaN loss that
        # is now a number, a duplicate tid whose loss now wins the dedupe) --
        # all of them, however many: the reference re-reads every document on
        # every call (tpe.py:820-848), so a skipped check would be a silent
        # divergence; the cost is one loss lookup per such document
        for d, l0 in self._dropped.values():
            loss = _loss_of(dom, d)
            if not (loss == l0 or (loss != loss and l0 != l0)):
                return False
        for r in list(self._pending):
            loss = _loss_of(dom, self.docs[r])
            if loss != loss:
                return False
            if loss != math.inf:
                self.losses[r] = loss
                self._pending.discard(r)
                self._loss_dirty = min(self._loss_dirty, r)
                self._touched.add(r)
        new = view[self._seen:]
        self._grow(self.n + len(new))
        last = self.tids[-1] if self.tids else None
        for doc in new:
            if 'from_tid' in doc['misc']:
                return False
            tid, v, a = self._extract(doc)
            if not _is_int_tid(tid) or (last is not None and tid <= last):
                return False
            loss = _loss_of(dom, doc)
            if loss != loss:
                return False
            r = self.n
            self._put_row(r, tid, loss, v, a, doc)
            self._row[id(doc)] = r
            self.n = r + 1
            last = tid
        return True

    def _rebuild(self, view):
        """Full rebuild with the reference's dedupe and tid sort."""
        dom = self.domain
        dev = self._dev
        self._forget()
        self._dev = dev
        best = {}               # tid -> [loss, doc]
        seen = {}               # id(doc) -> its loss now
        for doc in view:
            tid = doc['misc'].get('from_tid', doc['tid'])
            loss = _loss_of(dom, doc)
            seen[id(doc)] = loss
            cur = best.get(tid)
            if cur is None:
                best[tid] = [loss, doc if loss == loss else None]
            elif loss <= cur[0]:
                cur[0], cur[1] = loss, doc
        rows = sorted(((t, e[0], e[1]) for t, e in best.items() if e[1] is not None),
                      key=lambda z: z[0])
        kept = {id(e[2]) for e in rows}
        self._dropped = {id(d): (d, seen[id(d)]) for d in view if id(d) not in kept}
        self._grow(len(rows))
        plain = True
        for r, (tid, loss, doc) in enumerate(rows):
            _, v, a = self._extract(doc)
            self._put_row(r, tid, loss, v, a, doc)
            self._row[id(doc)] = r
            plain &= 'from_tid' not in doc['misc']
        self.n = len(rows)
        # rows that are not 1:1 documents (merged from_tid results): every
        # later sync rebuilds
        self._plain = plain and all(_is_int_tid(t) for t in self.tids)
        self._vals_dirty = self._loss_dirty = 0

    # -- views ----------------------------------------------------------------
    def columns(self):
        """(tids, losses[n], vals[P, n], active[P, n]) copies."""
        n = self.n
        return (list(self.tids), self.losses[:n].copy(), self.vals[:, :n].copy(),
                self.active[:, :n].copy())

    def reference(self):
        """The reference point this sync's ``hypervolume`` means: the given
        one, the default one of the rows held, or None (off: no setting, or the
        default without a complete row)."""
        if self.hv is False or self.M is None:
            return None
        if self.hv is True:
            return default_reference(self.Y[:, :self.n])
        return self.hv

    # -- device copy ------------------------------------------------------------
    def push(self, plan):
        """Copy the rows and losses that changed since the last push into
        ``plan``'s device history."""
        if self._dev is None or self._dev() is not plan or \
                getattr(plan, '_history_owner', None) is not self:
            self._vals_dirty = self._loss_dirty = self._obj_dirty = 0
            self._dev_mode = None
        r0 = min(self._vals_dirty, self.n)
        if self.M is None:
            if self._dev_mode is not None:
                self._loss_dirty = 0        # the column holds a ranking: every loss goes again
            l0 = min(self._loss_dirty, r0, self.n)
            plan.update_history(self.n, r0, self.vals, self.active, self.cap, l0, self.losses)
            self._loss_dirty = self.n
        else:
            # no loss travels: set_objectives writes the whole column after the
            # rows (and after a deferred patch of them, tpe_engine.h)
            plan.update_history(self.n, r0, self.vals, self.active, self.cap, self.n,
                                self.losses)
            mode = self.M if self.hv is False else (self.M, self.hv)
            o0 = min(self._obj_dirty, self.n) if self._dev_mode == mode else 0
            # the setting goes before the ranking that reads it; a plan that
            # never saw one is off (Plan._hv_on), and is not told so again
            ref = self.reference()
            if ref is not None:
                plan.set_hv(ref, self.M, HV_N_PICK, HV_N_SAMPLES, HV_SEED, HV_METHOD)
            elif getattr(plan, '_hv_on', False):
                plan.set_hv(None)
            plan.set_objectives(self.Y, n=self.n, obj0=o0)
            self._obj_dirty = self.n
        self._dev_mode = self.M if self.M is None or self.hv is False else (self.M, self.hv)
        plan._history_owner = self
        self._dev = weakref.ref(plan)
        self._vals_dirty = self.n
        return self
