"""Generate tests/golden/anneal.npz and anneal.json by running the REFERENCE's
annealer and mix.suggest (build container only; the reference never travels to
the GPU box):

    oracle/setup_reference.sh /tmp/oracle
    python tests/golden/make_golden_anneal.py /tmp/oracle

anneal.json holds the names (spaces, histories, labels, new ids), the seeds and
settings, the tie-skip counts and mix.suggest's 64 (index, sub-seed) picks;
anneal.npz the numbers (tests/test_anneal_host.py reads both back).  Per history
k: h{k}_tids, h{k}_losses (+inf pending), h{k}_vals [P, n] (NaN: inactive).
Per case (a history, a seed, avg_best_idx, shrink_coef): case_hist, case_seed,
case_abi, case_sc, case_vals (the final misc.vals by label, NaN: absent) and
its events [case_off[c], case_off[c + 1]), one per hyperparameter node in the
reference's node-evaluation order:

ev_label  -- index of the label in the history's labels;
ev_size   -- 1 if the hp is active in the new trial, else 0 (the samplers then
             run with size 0 and draw nothing: asserted here);
ev_reused -- 1 the anchor came from the anchor list, 0 a fresh anchor was
             drawn, -1 no anchor (prior draw or inactive hp);
ev_good   -- the clipped rank of a fresh anchor (else -1);
ev_tid    -- the anchor's trial id (else -1);
ev_skip   -- 1 when two tied losses straddle the chosen rank, so that numpy's
             unstable argsort, not the algorithm, picked the tid;
ev_geo    -- the p argument of the node's rng.geometric call (NaN: none);
ev_kind, ev_a, ev_b -- the node's sampler call on the RandomState: 1 uniform
             (low, high), 2 normal (mu, sigma), 3 multinomial (pvals =
             ev_p[ev_poff[e] : ev_poff[e + 1]]), 4 randint (upper), 0 none
             (q is a constant of the space);
ev_value  -- the node's draw (NaN when inactive).

Only data is stored: histories, arguments and results.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else '/tmp/oracle'
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))          # tests/ for spaces.py

import hyperopt                                     # noqa: E402  (reference)
from hyperopt import anneal, mix, rand, hp, Trials, base   # noqa: E402
import spaces                                       # noqa: E402

assert os.path.abspath(os.path.dirname(hyperopt.__file__)).startswith(os.path.abspath(REF))

SEEDS = (0, 1, 2, 3, 11, 123, 4567, 2 ** 20 + 3)
SETTINGS = ((2.0, 0.1), (2.0, 0.0), (50.0, 0.1), (50.0, 0.0))


def plain(x):
    if isinstance(x, np.ndarray):
        return [plain(v) for v in x.tolist()]
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    if isinstance(x, (np.integer,)):
        return int(x)
    if isinstance(x, (np.floating,)):
        return float(x)
    return x


class RecordingRng(object):
    """Forwards to a RandomState and logs every draw call."""

    def __init__(self, rng, log):
        self._rng, self._log = rng, log
        self.last_geometric = None

    def seed(self, *a, **k):
        return self._rng.seed(*a, **k)

    def __getattr__(self, name):
        f = getattr(self._rng, name)

        def g(*a, **k):
            r = f(*a, **k)
            if name == 'geometric' and np.asarray(r).size == 1:
                self.last_geometric = int(np.asarray(r).ravel()[0])
            self._log.append([name] + [plain(v) for v in a] +
                             [[kk, plain(vv)] for kk, vv in sorted(k.items())])
            return r
        return g


def draw_of(calls, size):
    """(geometric p, kind, a, b, pvals) of one node's RandomState calls."""
    geo, kind, a, b, p = np.nan, 0, np.nan, np.nan, []
    for c in calls:
        name = c[0]
        kw = dict(x for x in c[1:] if isinstance(x, list) and len(x) == 2 and isinstance(x[0], str))
        pos = [x for x in c[1:] if not (isinstance(x, list) and len(x) == 2 and
                                        isinstance(x[0], str))]
        if size == 0:
            assert kw['size'] == 0, c
            continue
        first = lambda v: float(np.ravel(v)[0])     # noqa: E731
        if name == 'geometric':
            geo = float(pos[0])
        elif name in ('uniform', 'normal'):
            kind, a, b = (1 if name == 'uniform' else 2), first(pos[0]), first(pos[1])
        elif name == 'multinomial':
            kind, p = 3, [float(v) for v in np.ravel(kw['pvals'])]
        elif name == 'randint':
            kind, a = 4, float(pos[0])
        else:
            raise AssertionError(c)
    return geo, kind, a, b, p


def run_case(domain, trials, seed, new_id, avg_best_idx, shrink_coef):
    algo = anneal.AnnealingAlgo(domain, trials, seed, avg_best_idx=avg_best_idx,
                                shrink_coef=shrink_coef)
    calls = []
    algo.rng = RecordingRng(algo.rng, calls)
    events = []
    cur = {}
    orig_ltv = algo.choose_ltv
    orig_node = algo.on_node_hyperparameter

    def choose_ltv(label, size):
        n_best = len(algo.best_tids)
        n_calls = len(calls)
        loss, tid, val = orig_ltv(label, size=size)
        if size == 1:
            fresh = len(algo.best_tids) > n_best
            cur['reused'] = 0 if fresh else 1
            tid_i = int(np.asarray(tid).ravel()[0])
            cur['tid'] = tid_i
            if fresh:
                geo = [c for c in calls[n_calls:] if c[0] == 'geometric']
                assert len(geo) == 1
                tids = algo.node_tids[label]
                losses = np.asarray([algo.tid_losses_dct[t] for t in tids])
                r = int(np.clip(algo.rng.last_geometric - 1, 0, len(tids) - 1))
                srt = np.sort(losses)
                cur['good_idx'] = r
                cur['skip'] = int((r > 0 and srt[r - 1] == srt[r]) or
                                  (r + 1 < len(srt) and srt[r + 1] == srt[r]))
                if not cur['skip']:
                    assert losses[list(tids).index(tid_i)] == srt[r]
        return loss, tid, val

    def on_node_hyperparameter(memo, node, label):
        cur.clear()
        cur.update(reused=None, good_idx=None, tid=None, skip=0)
        n_calls = len(calls)
        size = int(memo[node.arg['size']])
        rval = orig_node(memo, node, label)
        value = None
        if size == 1:
            value = float(np.asarray(rval).ravel()[0])
        events.append([label, size, cur['reused'], cur['good_idx'], cur['tid'], cur['skip'],
                       draw_of(calls[n_calls:], size), value])
        return rval

    algo.choose_ltv = choose_ltv
    algo.on_node_hyperparameter = on_node_hyperparameter
    doc, = algo(new_id)
    vals = {k: plain(v) for k, v in doc['misc']['vals'].items()}
    return events, vals


def make_trials(domain, n_draw, seed, loss_seed, pending=(), quant=None, keep=None, limit=None):
    t = Trials()
    docs = rand.suggest(list(range(n_draw)), domain, t, seed)
    if keep is not None:
        docs = [d for d in docs if keep(d)]
    if limit is not None:
        docs = docs[:limit]
    losses = np.random.RandomState(loss_seed).rand(len(docs))
    if quant:
        losses = np.round(losses * quant) / quant
    for j, (doc, l) in enumerate(zip(docs, losses)):
        if j in pending:
            continue                    # stays JOB_STATE_NEW, status 'new': loss None
        doc['state'] = base.JOB_STATE_DONE
        doc['result'] = {'status': base.STATUS_OK, 'loss': float(l)}
    t.insert_trial_docs(docs)
    t.refresh()
    return t


def dump_history(domain, trials):
    labels = sorted(domain.params.keys())
    tids = [d['tid'] for d in trials.trials]
    losses = []
    for d in trials.trials:
        l = domain.loss(d['result'], d['spec'])
        losses.append(None if l is None else float(l))
    vals = {lab: [[d['tid'], plain(d['misc']['vals'][lab][0])] for d in trials.trials
                  if d['misc']['vals'][lab]] for lab in labels}
    return dict(labels=labels, tids=tids, losses=losses, vals=vals)


def histories():
    md = lambda: base.Domain(lambda x: 0.0, spaces.many_dists_space(hp))    # noqa: E731
    cd = lambda: base.Domain(lambda x: 0.0, spaces.cond_space(hp))          # noqa: E731
    out = []
    for name, mk in (('many_dists', md), ('cond', cd)):
        d = mk()
        out.append((name, 'n0', d, make_trials(d, 0, 1, 2)))
        out.append((name, 'n1', d, make_trials(d, 1, 3, 4)))
        out.append((name, 'n7_pending', d, make_trials(d, 7, 5, 6, pending=(4,))))
        out.append((name, 'n120_pending', d, make_trials(d, 120, 7, 8, pending=(17, 60, 119))))
    d = md()
    out.append(('many_dists', 'n120_tied', d, make_trials(d, 120, 9, 10, quant=250.0)))
    d = cd()
    # branch 2 of `top` never observed: its children have T = 0 (prior draws)
    out.append(('cond', 'n120_branch2_unseen', d,
                make_trials(d, 400, 11, 12, keep=lambda doc: doc['misc']['vals']['top'][0] != 2,
                            limit=120)))
    return out


def gen_mix():
    rec = []

    def stub(k):
        def f(new_ids, domain, trials, seed):
            rec.append([k, int(seed)])
            return []
        return f
    for seed in range(64):
        mix.suggest([0], None, None, seed,
                    p_suggest=[(.1, stub(0)), (.2, stub(1)), (.7, stub(2))])
    assert len(rec) == 64
    return rec


def main():
    np.seterr(all='ignore')
    out = dict(seeds=list(SEEDS), settings=[list(s) for s in SETTINGS], histories=[],
               mix=dict(p=[.1, .2, .7], picks=gen_mix()))
    fresh = skipped = 0
    for space, name, domain, trials in histories():
        h = dump_history(domain, trials)
        new_id = (max(h['tids']) + 1) if h['tids'] else 0
        cases = []
        for (abi, sc) in SETTINGS:
            for seed in SEEDS:
                events, vals = run_case(domain, trials, seed, new_id, abi, sc)
                cases.append(dict(seed=seed, avg_best_idx=abi, shrink_coef=sc, events=events,
                                  vals=vals))
                fresh += sum(1 for e in events if e[2] == 0)
                skipped += sum(1 for e in events if e[2] == 0 and e[5])
        out['histories'].append(dict(space=space, name=name, new_id=new_id, history=h,
                                     cases=cases))
        print(space, name, 'n', len(h['tids']), 'order', [e[0] for e in cases[0]['events']])
    out['fresh_anchors'] = fresh
    out['skipped_fresh_anchors'] = skipped
    print('fresh anchors', fresh, 'tie-skipped', skipped, '= %.2f %%' % (100.0 * skipped / fresh))
    assert skipped <= 0.05 * fresh
    write(out)


def write(out):
    z, meta = {}, dict(out, histories=[])
    ch, cseed, cabi, csc, coff, cvals = [], [], [], [], [0], []
    ev = {k: [] for k in ('label', 'size', 'reused', 'good', 'tid', 'skip', 'geo', 'kind', 'a', 'b',
                          'value')}
    ep, epoff = [], [0]
    none = lambda v: -1 if v is None else v         # noqa: E731
    for k, h in enumerate(out['histories']):
        hist = h['history']
        labels, tids = hist['labels'], hist['tids']
        meta['histories'].append(dict(space=h['space'], name=h['name'], new_id=h['new_id'],
                                      labels=labels))
        row = {t: r for r, t in enumerate(tids)}
        vals = np.full((len(labels), len(tids)), np.nan)
        for i, lab in enumerate(labels):
            for t, v in hist['vals'][lab]:
                vals[i, row[t]] = v
        z['h%d_tids' % k] = np.asarray(tids, dtype=np.int64)
        z['h%d_losses' % k] = np.asarray([np.inf if l is None else l for l in hist['losses']],
                                         dtype=np.float64)
        z['h%d_vals' % k] = vals
        for c in h['cases']:
            ch.append(k); cseed.append(c['seed']); cabi.append(c['avg_best_idx'])
            csc.append(c['shrink_coef'])
            cvals.append([c['vals'][lab][0] if c['vals'][lab] else np.nan for lab in labels])
            for label, size, reused, good, tid, skip, (geo, kind, a, b, p), value in c['events']:
                for key, v in zip(('label', 'size', 'reused', 'good', 'tid', 'skip', 'geo', 'kind',
                                   'a', 'b', 'value'),
                                  (labels.index(label), size, none(reused), none(good), none(tid),
                                   skip, geo, kind, a, b, np.nan if value is None else value)):
                    ev[key].append(v)
                ep.extend(p)
                epoff.append(len(ep))
            coff.append(len(ev['label']))
    width = max(len(v) for v in cvals)
    z['case_vals'] = np.asarray([v + [np.nan] * (width - len(v)) for v in cvals])
    z.update(case_hist=np.asarray(ch, np.int16), case_seed=np.asarray(cseed, np.int64),
             case_abi=np.asarray(cabi), case_sc=np.asarray(csc), case_off=np.asarray(coff, np.int32),
             ev_p=np.asarray(ep), ev_poff=np.asarray(epoff, np.int32))
    for key, v in ev.items():
        small = key in ('label', 'size', 'reused', 'skip', 'kind')
        z['ev_' + key] = np.asarray(v, dtype=np.int8 if small else
                                    (np.int32 if key in ('good', 'tid') else np.float64))
    np.savez_compressed(os.path.join(HERE, 'anneal.npz'), **z)
    with open(os.path.join(HERE, 'anneal.json'), 'w') as f:
        json.dump(meta, f)
    for fn in ('anneal.npz', 'anneal.json'):
        print(fn, os.path.getsize(os.path.join(HERE, fn)), 'bytes')
        assert os.path.getsize(os.path.join(HERE, fn)) < 256 * 1024


if __name__ == '__main__':
    main()
