"""The lean direct pass behind the Chebyshev tables (DESIGN 5.10;
k_score_wave_tie_lean: the launch's fixed form alone, the slot's state staged
once per persistent block) against k_score_wave_tie, which the same library
keeps behind TPE_TIE_LEAN=0.  The switch is read once per process: every run
is a child interpreter, one per environment and form, with the screened
draw's size gate at 0 (TPE_DRAW_SCREEN_MIN) so that the small shape takes the
draw, the map and the gather a large suggest takes.

Compared in every case, byte for byte: the records, Plan.tie_counts and
Plan.tab_wmax.  Shape: test_gpu_table.py's -- u (a GW slot), n (GW, no table:
every wave tile listed) and lu (an LW slot) in one launch, N = 6000 trials,
NC = 2^18 + 8192 + 37 candidates: the last wave tile holds 37 candidates and
the last gathered block of a full list 7 waves past them.

Cases: the shape with the default window (sparse lists, lengths that are no
multiple of 8: the last gathered block has waves without a list entry); 24
suggestions with every wave hot (TPE_TABLE_TIE_LOG2=2000): 265 gathered blocks
per slot over G = ceil(32 * 256 / 72) = 114 persistent blocks, so the loop
runs three times on the state staged once; NC2 candidates (no wave tile past
them) with the narrowest window: lists of fewer than 8 entries, one gathered
block; the conditional space (an inactive hp: no list, no ticket, the
gather's record stands); candidate chunks (TPE_CHUNK_MB=36: a later launch
accumulates onto the records of the one before); a replayed graph
(TPE_GRAPH=1) against eager; a census launch (the <true> form: the records
and the counters of k_score_wave_tie<true>); and the default against TPE_TABLE=0.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_table as T
import test_gpu_tie_gather as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NC = T.NC
NC2 = (1 << 18) + 8192 + 1024 - 91     # 8 x 265 wave tiles, all holding candidates, the last 37
BASE = {'TPE_DRAW_SCREEN_MIN': '0'}
LEAN_OFF = {'TPE_TIE_LEAN': '0'}
SEEDS24 = T.SEEDS12 + [3001 + 23 * s for s in range(12)]
# launch_class's persistent blocks per slot: kTieLeanBlocksPerCu = 32 on 256 CUs over 3 x 24 rows
G_TIE = (32 * 256 + 3 * 24 - 1) // (3 * 24)


def _hex(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes().hex()


def _suggest(plan, seeds, nc, census=False):
    if census:
        plan.census(True)
    res = plan.suggest(seeds, nc)
    try:
        wmax = _hex(plan.tab_wmax(len(seeds)))
    except ValueError:      # (TPE_TABLE=0: no table pass)
        wmax = None
    out = dict(hex=T._hex(res), counts=plan.tie_counts(len(seeds)).tolist(), wmax=wmax,
               active=res['active'].tolist())
    if census:
        out['census'] = [int(c) for c in plan.census(False, n=13)]
    return out


def case_shape():
    dom, plan, _ = T._plan()
    return dict(_suggest(plan, T.SEEDS6, NC), labels=list(dom.space.labels))


def case_census():
    dom, plan, _ = T._plan()
    return dict(_suggest(plan, T.SEEDS6, NC, census=True), labels=list(dom.space.labels))


def case_many():
    dom, plan, _ = T._plan()
    return dict(_suggest(plan, SEEDS24, NC), labels=list(dom.space.labels))


def case_short():
    dom, plan, _ = T._plan()
    return dict(_suggest(plan, T.SEEDS6, NC2), labels=list(dom.space.labels))


def case_cond():
    dom, plan = G._cond_plan()
    return dict(_suggest(plan, T.SEEDS11, NC), labels=list(dom.space.labels))


def case_chunks():
    dom, plan, _ = T._plan()
    plan.profile(16)
    out = _suggest(plan, T.SEEDS11, NC)
    return dict(out, launches=plan.profile_read(0)[1], labels=list(dom.space.labels))


def case_graph():
    """fit_suggest three times on one plan: under TPE_GRAPH=1 the second and
    third calls replay the captured step."""
    from hyperopt_amd import _engine as E
    from hyperopt_amd.base import Domain
    dom = Domain(lambda x: 0.0, T._space())
    L, vals, act = T._history(dom)
    hps, conds, pprior = dom.space.engine_tables()
    plan = E.Plan(E.default_engine(), hps, conds, pprior, max_trials=T.N)
    plan.set_history(L, vals, act)
    out = []
    for i in range(3):
        res = plan.fit_suggest([31 + i] + T.SEEDS6[1:], NC)
        out.append(dict(hex=T._hex(res), counts=plan.tie_counts(6).tolist(),
                        wmax=_hex(plan.tab_wmax(6))))
    return dict(calls=out)


CASES = dict(shape=case_shape, census=case_census, many=case_many, short=case_short,
             cond=case_cond, chunks=case_chunks, graph=case_graph)


def run_cases(names):
    return {n: CASES[n]() for n in names}


def _child(names, env):
    code = ("import sys, json; sys.path.insert(0, 'tests'); import test_gpu_tie_lean as L; "
            "print('JSON' + json.dumps(L.run_cases(%r)))" % (list(names),))
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=dict(os.environ, **BASE, **env),
                       capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.split('JSON')[-1])


ENVS = {
    'plain': ({}, ('shape', 'census', 'cond')),
    'wide': (G.WIDE, ('many',)),
    'narrow': ({'TPE_TABLE_TIE_LOG2': '-1074'}, ('short',)),
    'chunks': ({'TPE_CHUNK_MB': '36'}, ('chunks',)),
    'graph': ({'TPE_GRAPH': '1'}, ('graph',)),
    'eager': ({}, ('graph',)),
}
_runs = {}


def pair(env):
    """(default form, TPE_TIE_LEAN=0) runs of an environment, made once."""
    if env not in _runs:
        assert os.environ.get('TPE_TIE_LEAN', '1') != '0', 'the default form is under test'
        extra, names = ENVS[env]
        _runs[env] = (_child(names, extra), _child(names, dict(extra, **LEAN_OFF)))
    return _runs[env]


def _same(on, off):
    assert on['counts'] == off['counts']
    assert on['wmax'] == off['wmax']
    assert on['hex'] == off['hex']


def _col(run, label):
    return np.asarray(run['counts'])[:, run['labels'].index(label)]


def test_two_kinds_ragged_lists():
    """u (GW) and lu (LW) in one launch, sparse lists: some list length is no
    multiple of 8, so a last gathered block has waves without a tile."""
    on, off = pair('plain')
    on, off = on['shape'], off['shape']
    _same(on, off)
    cu, cl = _col(on, 'u'), _col(on, 'lu')
    print('u', cu.tolist(), 'lu', cl.tolist())
    assert ((cu > 0) & (cu < G.WAVE_TILES)).all() and ((cl > 0) & (cl < G.WAVE_TILES)).all()
    assert (np.concatenate([cu, cl]) % 8 != 0).any()
    assert NC % 128 == 37                       # the last wave tile is partial
    assert (_col(on, 'n') == G.WAVE_TILES).all()  # ... and in n's list, with 7 waves past it


def test_three_iterations_per_block():
    """Every wave hot, 24 suggestions of 3 slots: 265 gathered blocks on 114
    persistent blocks (the old kernel's grid is 57: five iterations)."""
    on, off = pair('wide')
    on, off = on['many'], off['many']
    _same(on, off)
    assert (np.asarray(on['counts']) == G.WAVE_TILES).all()
    nblk = G.WAVE_TILES // 8
    assert G_TIE == 114 and 2 * G_TIE < nblk <= 3 * G_TIE


def test_single_gathered_block():
    """The narrowest window on a draw without a wave tile past its candidates:
    a certified slot lists fewer than 8 wave tiles."""
    on, off = pair('narrow')
    on, off = on['short'], off['short']
    _same(on, off)
    assert NC2 % 128 == 37 and 8 * ((NC2 + 1023) // 1024) == (NC2 + 127) // 128
    for lab in ('u', 'lu'):
        c = _col(on, lab)
        print(lab, c.tolist())
        assert ((c > 0) & (c < 8)).all(), (lab, c.tolist())


def test_inactive_hp():
    """The conditional space: an hp inactive in a suggestion has no list, takes
    no ticket and keeps the gather's record."""
    on, off = pair('plain')
    on, off = on['cond'], off['cond']
    _same(on, off)
    assert on['active'] == off['active']
    cnt, act = np.asarray(on['counts']), np.asarray(on['active'])
    for lab in ('a', 'b'):
        i = on['labels'].index(lab)
        print(lab, 'active', act[:, i].tolist(), 'counts', cnt[:, i].tolist())
        assert (act[:, i] == 0).any() and (act[:, i] == 1).any()
        assert (cnt[act[:, i] == 0, i] == 0).all() and (cnt[act[:, i] == 1, i] > 0).all()


def test_chunked_accumulates():
    """Candidate chunks: the later launches accumulate onto the records."""
    on, off = pair('chunks')
    on, off = on['chunks'], off['chunks']
    _same(on, off)
    assert on['launches'] == off['launches']
    one = _child(['chunks'], {})['chunks']
    print('launches', on['launches'], 'against', one['launches'])
    assert on['launches'] > one['launches']
    assert on['hex'] == one['hex']


def test_graph_replay():
    """TPE_GRAPH=1: each form's replays leave the other form's bytes, and the
    records of the eager calls."""
    graph, graph_off = pair('graph')
    eager, eager_off = pair('eager')
    for on, off in ((graph, graph_off), (eager, eager_off)):
        for a, b in zip(on['graph']['calls'], off['graph']['calls']):
            print('counts', a['counts'])
            assert a['counts'] == b['counts']
            assert a['wmax'] == b['wmax']
            assert a['hex'] == b['hex']
    assert [c['hex'] for c in graph['graph']['calls']] == [c['hex'] for c in eager['graph']['calls']]
    assert len({c['hex'] for c in graph['graph']['calls']}) == 3     # (three different seeds)


def test_census_form():
    """The census launch: the records and the counters of
    k_score_wave_tie<true>.  (A census build visits every envelope round, so
    its sums are not the plain launch's to the last bit, in either form.)"""
    on, off = pair('plain')
    _same(on['census'], off['census'])
    print('census', on['census']['census'])
    assert on['census']['census'] == off['census']['census']
    assert on['census']['census'][3] > 0


def test_against_direct_scoring():
    """The default against TPE_TABLE=0 (no tables, every pair scored directly):
    the same records."""
    on, _ = pair('plain')
    direct = _child(['shape'], {'TPE_TABLE': '0'})['shape']
    assert (np.asarray(direct['counts']) == -1).all()     # no such launch without tables
    assert on['shape']['hex'] == direct['hex']
