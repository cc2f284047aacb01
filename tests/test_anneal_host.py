"""anneal.suggest / mix.suggest on the host against tests/golden/anneal.npz and
anneal.json (recorded from the reference by tests/golden/make_golden_anneal.py): the
module-level pieces of hyperopt_amd.anneal reproduce every recorded sampler
argument and anchor, the 'numpy' stream reproduces the reference's
suggestions value for value, and mix.suggest its picks and sub-seeds.

Cases in which two tied losses straddle the drawn rank are skipped where the
anchor's tid is compared (numpy's unstable argsort picked it, DESIGN section 3
"Tie hazard"); the fixture's share of them is checked against its 5 % cap."""
import json
import math
import os

import numpy as np
import pytest

import spaces
from hyperopt_amd import anneal, mix, hp, Trials
from hyperopt_amd import JOB_STATE_DONE, JOB_STATE_NEW
from hyperopt_amd.base import Domain

HERE = os.path.dirname(os.path.abspath(__file__))


def _domain(space):
    builder = {'many_dists': spaces.many_dists_space, 'cond': spaces.cond_space}[space]
    return Domain(lambda x: 0.0, builder(hp))


@pytest.fixture(scope='module')
def golden():
    """The fixture as nested dicts: names from anneal.json, numbers from
    anneal.npz (layout: tests/golden/make_golden_anneal.py).  An event is
    [label, size, reused, good_idx, tid, skip, sampler call, value, geometric p]."""
    with open(os.path.join(HERE, 'golden', 'anneal.json')) as f:
        g = json.load(f)
    z = dict(np.load(os.path.join(HERE, 'golden', 'anneal.npz')))
    opt = lambda v: None if v < 0 else int(v)       # noqa: E731
    for k, h in enumerate(g['histories']):
        cs = _domain(h['space']).space
        labels = h['labels']
        cat = [cs.by_label[lab].is_categorical for lab in labels]
        typed = lambda i, v: int(v) if cat[i] else float(v)     # noqa: E731
        tids, vals = z['h%d_tids' % k].tolist(), z['h%d_vals' % k]
        h['history'] = dict(
            labels=labels, tids=tids,
            losses=[None if l == math.inf else l for l in z['h%d_losses' % k].tolist()],
            vals={lab: [[t, typed(i, v)] for t, v in zip(tids, vals[i]) if v == v]
                  for i, lab in enumerate(labels)})
        h['cases'] = []
        for c in np.where(z['case_hist'] == k)[0]:
            events = []
            for e in range(z['case_off'][c], z['case_off'][c + 1]):
                kind, a, b = int(z['ev_kind'][e]), float(z['ev_a'][e]), float(z['ev_b'][e])
                call = {0: None, 1: ('uniform', a, b), 2: ('normal', a, b),
                        3: ('p', z['ev_p'][z['ev_poff'][e]:z['ev_poff'][e + 1]]),
                        4: ('randint', int(a) if kind == 4 else None)}[kind]
                value = float(z['ev_value'][e])
                events.append([labels[z['ev_label'][e]], int(z['ev_size'][e]), opt(z['ev_reused'][e]),
                               opt(z['ev_good'][e]), opt(z['ev_tid'][e]), int(z['ev_skip'][e]), call,
                               None if value != value else value, float(z['ev_geo'][e])])
            h['cases'].append(dict(
                seed=int(z['case_seed'][c]), avg_best_idx=float(z['case_abi'][c]),
                shrink_coef=float(z['case_sc'][c]), events=events,
                vals={lab: ([] if v != v else [typed(i, v)])
                      for i, (lab, v) in enumerate(zip(labels, z['case_vals'][c]))}))
    return g


def _trials(domain, hist):
    """A Trials holding the recorded history (pending trials: no loss)."""
    t = Trials()
    labels = hist['labels']
    by_tid = {tid: ({}, {}) for tid in hist['tids']}
    for lab in labels:
        for tid in hist['tids']:
            by_tid[tid][0][lab] = []
            by_tid[tid][1][lab] = []
        for tid, v in hist['vals'][lab]:
            by_tid[tid][0][lab] = [tid]
            by_tid[tid][1][lab] = [v]
    miscs = [dict(tid=tid, cmd=domain.cmd, workdir=domain.workdir, idxs=by_tid[tid][0],
                  vals=by_tid[tid][1]) for tid in hist['tids']]
    results = [{'status': 'new'} if l is None else {'status': 'ok', 'loss': l}
               for l in hist['losses']]
    docs = t.new_trial_docs(hist['tids'], [None] * len(miscs), results, miscs)
    for d, l in zip(docs, hist['losses']):
        d['state'] = JOB_STATE_NEW if l is None else JOB_STATE_DONE
    t.insert_trial_docs(docs)
    t.refresh()
    return t


def _columns(cs, hist):
    tids = hist['tids']
    row = {tid: r for r, tid in enumerate(tids)}
    losses = np.array([math.inf if l is None else l for l in hist['losses']], dtype=np.float64)
    vals = np.zeros((len(cs.labels), len(tids)))
    active = np.zeros((len(cs.labels), len(tids)), dtype=np.uint8)
    for lab in cs.labels:
        i = cs.by_label[lab].index
        for tid, v in hist['vals'][lab]:
            vals[i, row[tid]] = v
            active[i, row[tid]] = 1
    return tids, losses, vals, active


def _case_skipped(case):
    return any(e[5] for e in case['events'])


def test_fixture_tie_skip_share(golden):
    assert golden['skipped_fresh_anchors'] <= 0.05 * golden['fresh_anchors']
    n = sum(1 for h in golden['histories'] for c in h['cases'] for e in c['events']
            if e[2] == 0 and e[5])
    assert n == golden['skipped_fresh_anchors']
    assert golden['fresh_anchors'] >= 200


def test_evaluation_order_is_draw_order(golden):
    for h in golden['histories']:
        cs = _domain(h['space']).space
        for c in h['cases']:
            assert [e[0] for e in c['events']] == cs.draw_order


def test_pieces_reproduce_every_recorded_argument_and_anchor(golden):
    n_args = n_tids = 0
    for h in golden['histories']:
        cs = _domain(h['space']).space
        tids, losses, vals, active = _columns(cs, h['history'])
        row_of = {tid: r for r, tid in enumerate(tids)}
        order = anneal.loss_order(losses)
        for c in h['cases']:
            best = []
            for label, size, reused, good_idx, tid, skip, rec, value, geo in c['events']:
                d = cs.by_label[label]
                col = active[d.index]
                T = int(col.sum())
                if size == 0:
                    assert rec is None and value is None    # inactive: nothing drawn
                    continue
                if reused is None:                          # no observations: the prior
                    assert T == 0
                    want = anneal.value_params(d.dist, d.args, None, 1.0)
                    if d.dist == 'randint':
                        assert rec == ('randint', d.args[0])
                        continue
                else:
                    assert T > 0
                    got_row = anneal.reuse_anchor(best, col)
                    assert (got_row is not None) == bool(reused), (h['name'], label)
                    if got_row is None:
                        assert geo == 1.0 / c['avg_best_idx']
                        got_row = anneal.choose_anchor(order, col, good_idx)
                        if skip:
                            got_row = row_of[tid]           # numpy's pick among the tied
                        else:
                            assert tids[got_row] == tid, (h['name'], c['seed'], label)
                            n_tids += 1
                        best.append(got_row)
                    else:
                        assert tids[got_row] == tid
                    want = anneal.value_params(d.dist, d.args, vals[d.index, got_row],
                                               anneal.shrink(T, c['shrink_coef']))
                assert rec[0] == want[0], (label, rec, want)
                if want[0] == 'p':
                    assert list(rec[1]) == list(want[1]), (h['name'], label, rec, want)
                else:
                    assert rec[1] == want[1] and rec[2] == want[2], (h['name'], label, rec, want)
                n_args += 1
    assert n_args > 2000 and n_tids > 200


def test_numpy_stream_reproduces_reference_vals(golden):
    n = 0
    for h in golden['histories']:
        dom = _domain(h['space'])
        trials = _trials(dom, h['history'])
        for c in h['cases']:
            if _case_skipped(c):
                continue
            doc, = anneal.suggest([h['new_id']], dom, trials, c['seed'],
                                  avg_best_idx=c['avg_best_idx'], shrink_coef=c['shrink_coef'],
                                  rng_stream='numpy')
            assert doc['misc']['vals'] == c['vals'], (h['space'], h['name'], c['seed'])
            assert doc['misc']['idxs'] == {k: [h['new_id']] * len(v) for k, v in c['vals'].items()}
            n += 1
    assert n >= 300


def test_numpy_stream_takes_one_id():
    dom = _domain('many_dists')
    with pytest.raises(ValueError):
        anneal.suggest([0, 1], dom, Trials(), 0, rng_stream='numpy')
    with pytest.raises(ValueError):
        anneal.suggest([0], dom, Trials(), 0, rng_stream='mt19937')
    with pytest.raises(ValueError):
        anneal.suggest([0], dom, Trials(), 0, avg_best_idx=0.5, rng_stream='numpy')


def test_suggest_batch_numpy_shape():
    dom = _domain('cond')
    idxs, vals = anneal.suggest_batch([0, 1, 2], dom, Trials(), 3, rng_stream='numpy')
    assert set(idxs) == set(dom.space.labels) == set(vals)
    assert idxs['top'] == [0, 1, 2] and len(vals['aa']) == 3
    for lab in dom.space.labels:
        assert len(idxs[lab]) == len(vals[lab])


def test_rank_from_uniform_clip():
    assert anneal.rank_from_uniform(0.0, 2.0, 5) == 0
    assert anneal.rank_from_uniform(0.999999, 2.0, 5) == 4
    assert anneal.rank_from_uniform(0.9, 1.0, 5) == 0
    # P(g = 1) = p: u < p gives rank 0, u just above gives rank 1
    assert anneal.rank_from_uniform(0.49, 2.0, 5) == 0
    assert anneal.rank_from_uniform(0.51, 2.0, 5) == 1


def test_mix_reproduces_reference_picks(golden):
    rec = []

    def stub(k):
        def f(new_ids, domain, trials, seed):
            rec.append([k, seed])
            return ['doc%d' % k]
        return f
    p_suggest = list(zip(golden['mix']['p'], (stub(0), stub(1), stub(2))))
    for seed in range(64):
        out = mix.suggest([0], None, None, seed, p_suggest=p_suggest)
        assert out == ['doc%d' % rec[-1][0]]
    assert rec == golden['mix']['picks']
    assert all(isinstance(s, int) for _, s in rec)
    assert {k for k, _ in rec} == {0, 1, 2}


def test_mix_rejects_probabilities_not_summing_to_one():
    f = lambda *a, **k: []      # noqa: E731
    with pytest.raises(ValueError):
        mix.suggest([0], None, None, 0, p_suggest=[(.1, f), (.2, f), (.6, f)])


def test_exports():
    import hyperopt_amd
    assert hyperopt_amd.anneal is anneal and hyperopt_amd.mix is mix
