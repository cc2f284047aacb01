"""The screened draw's narrower zones and pooled rows (k_draw_zone's tail rank
and half-tile widening, k_draw_sorted_screen_run's dense rows):
whatever TPE_DRAW_SCREEN_TAIL, TPE_DRAW_SCREEN_HALVES and TPE_DRAW_SCREEN_POOL
say, every record, tab_wmax mark and kept tile is byte for byte what
TPE_DRAW_SCREEN=0 writes -- the zones only move the fallback rate, the pooled
rows (opt-in: TPE_DRAW_SCREEN_POOL=1) only which wave inverts and buckets an
element.

test_gpu_draw_screen_run.py's shape: space A, NC = 2^18 + 8192 + 77 candidates,
4 suggestions, a 6000-trial history: 33 sort blocks behind the pilot's, the last
of 77 candidates.  Every run is a child interpreter with TPE_DRAW_SCREEN_MIN=0.

The pooled rows at their edges.  Which sort blocks these are is computed by
test_pooled_rows_meet_their_edges from the device's own draws and hot
intervals with tools/table_error.py's draw_zones; as measured on the MI355X:
 - sort block 33 has 77 candidates, which go to waves 0 and 1 (one row and 13
   elements): waves 2 to 7 have empty lists beside them and the block's total
   is under 64.  Under the defaults its key range comes from listed elements
   for hp c (the good trials at its high edge) in suggestions 0 and 3 of the
   default set (lists of 6 and 0, of 5 and 1) and for b and c in suggestion 3
   of the few-below set (4 and 0, 5 and 1); under TPE_DRAW_SCREEN_TAIL=128 for
   most (suggestion, hp) pairs (lists of 4 to 12 and 0 to 3), which is what
   the pooled `tail=128` child is for;
 - the whole blocks hold a few hundred listed elements (under 3 half tiles:
   medians of 331 to 619 per hp in the few-below set, K = 3, and of 435 to
   771 in the default set, lists of at most 128 per wave; a few more under the
   default 4): no whole number of rows, e.g. few-below, hp a, suggestion 0,
   sort block 1: 46, 42, 39, 49, 51, 55, 54, 51;
 - a list overflows (more than 640 of a wave's 1024 elements inverted) under
   TPE_TABLE_TIE_LOG2=0: the tie window of 1 widens the hot intervals until a
   wave lists about 800 elements (hp d of the default set, a, c and d of
   few-below: 757 to 825), and about 1000 for the others.  Those sort blocks
   fall back; the pooled `tie=0` child is compared with a TPE_DRAW_SCREEN=0
   child of the same window.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_draw_screen import (FITS, LABELS_A, NC, NEG_INF, NWT, SEEDS, SORT, _child, _plan_a,
                                  _tiles, _u64hex, case_all, case_graph)  # noqa: F401
from test_gpu_draw_screen_run import _same_tiles_and_marks
import test_gpu_table as T

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import table_error as TE  # noqa: E402

pytestmark = pytest.mark.gpu

POOL = {'TPE_DRAW_SCREEN_POOL': '1'}
TIE0 = {'TPE_TABLE_TIE_LOG2': '0'}
PARENT = {'TPE_DRAW_SCREEN_TAIL': '128', 'TPE_DRAW_SCREEN_TILES': '2', 'TPE_DRAW_SCREEN_POOL': '0'}
CHILDREN = (
    ('default', {}),
    ('pool=1', POOL),
    ('pool=0', {'TPE_DRAW_SCREEN_POOL': '0'}),
    ('parent', PARENT),                      # the zones and loops before this change
    ('tail=1', dict(POOL, TPE_DRAW_SCREEN_TAIL='1')),
    ('tail=128', dict(POOL, TPE_DRAW_SCREEN_TAIL='128')),
    ('halves=0', dict(POOL, TPE_DRAW_SCREEN_HALVES='0')),
    ('halves=8', dict(POOL, TPE_DRAW_SCREEN_HALVES='8')),
    ('run=0', {'TPE_DRAW_SCREEN_RUN': '0'}),
    ('run=3', dict(POOL, TPE_DRAW_SCREEN_RUN='3')),
    ('screen=0', {'TPE_DRAW_SCREEN': '0'}),
)
NAMES = tuple(n for n, _ in CHILDREN)
# a tie window under which lists overflow, with its own reference
CHILDREN_TIE0 = (('tie=0', dict(POOL, **TIE0)), ('tie=0 screen=0', dict(TIE0, TPE_DRAW_SCREEN='0')))
SWITCHES = ('TPE_DRAW_SCREEN_TILES', 'TPE_DRAW_SCREEN_GUIDE_BITS', 'TPE_DRAW_SCREEN_RUN',
            'TPE_DRAW_SCREEN_TAIL', 'TPE_DRAW_SCREEN_HALVES', 'TPE_DRAW_SCREEN_POOL')


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    for k in ('TPE_DRAW_SCREEN', 'TPE_DRAW_SCREEN_INT', 'TPE_DRAW_PRUNE', 'TPE_TABLE_PREFILTER'):
        assert os.environ.get(k, '1') != '0', 'the default is under test'
    for k in SWITCHES:
        assert k not in os.environ, 'the default is under test'
    d = str(tmp_path_factory.mktemp('drawdense'))
    return {name: _child('case_all', os.path.join(d, '%d.npz' % i), env)
            for i, (name, env) in enumerate(CHILDREN + CHILDREN_TIE0)}


def test_records_equal(runs):
    """Space A under every fit set and space B: every child's records are
    those of TPE_DRAW_SCREEN=0."""
    off = runs['screen=0'][0]
    assert set(off) == {'A/' + f for f in FITS} | {'B'}
    for name in NAMES[:-1]:
        for k in off:
            assert runs[name][0][k]['hex'] == off[k]['hex'], (name, k)


def test_tiles_and_marks_equal(runs):
    """tab_wmax marks and Plan.cand_dump on every kept tile against
    TPE_DRAW_SCREEN=0."""
    dropped = 0
    for name in NAMES[:-1]:
        dropped += _same_tiles_and_marks(runs[name], runs['screen=0'], name)
    assert dropped > 0                                   # (the draw does prune here)


def test_list_overflow_falls_back(runs):
    """TPE_TABLE_TIE_LOG2=0: waves list more than kScreenList elements (which
    ones: test_pooled_rows_meet_their_edges), those sort blocks fall back, and
    every byte is that of TPE_DRAW_SCREEN=0 under the same window."""
    on, off = runs['tie=0'], runs['tie=0 screen=0']
    for k in off[0]:
        assert on[0][k]['hex'] == off[0][k]['hex'], k
        assert off[0][k]['stats'] == [0, 0, 0], k
    _same_tiles_and_marks(on, off, 'tie=0')
    for fit in ('default', 'few-below'):
        scr, fb, exact = on[0]['A/' + fit]['stats']
        print('tie=0 %s: %d screened, %d fell back, %d inverted' % (fit, scr, fb, exact))
        assert fb > 0, fit


def test_counters(runs):
    """(sort blocks screened, fallen back, elements inverted) per child."""
    st = {name: {k: runs[name][0][k]['stats'] for k in runs[name][0]} for name in NAMES}
    for name in NAMES:
        print(name, {k: v for k, v in st[name].items() if k != 'B'})
    for k in st['default']:
        assert st['pool=1'][k] == st['pool=0'][k], k      # the pooled rows count what the lists do
        assert st['pool=0'][k] == st['default'][k], k
        assert st['run=0'][k] == st['default'][k], k      # ... and all three kernels read one DrawZone
        assert st['run=3'][k] == st['default'][k], k
        assert st['screen=0'][k] == [0, 0, 0], k
    for fit in ('default', 'few-below'):
        k = 'A/' + fit
        assert st['default'][k][0] > 0 and st['parent'][k][0] > 0, k
        assert st['default'][k][2] < st['parent'][k][2], (k, st['default'][k], st['parent'][k])
    assert st['tail=1']['A/default'][1] > 0
    assert st['halves=0']['A/default'][1] > 0
    # the wider the zones, the more is inverted per screened block
    for a, b in (('halves=0', 'default'), ('default', 'halves=8')):
        sa, sb = st[a]['A/default'], st[b]['A/default']
        if sa[0] and sb[0]:
            assert sa[2] / sa[0] < sb[2] / sb[0], (a, b, sa, sb)


def test_graph_replay_matches_eager():
    """TPE_GRAPH=1 (child): replays with changed seeds equal the eager calls
    under zones and rows that are not the defaults (they are in the captured
    step's key and reach k_draw_zone's node), and under the defaults."""
    seen = []
    for env in ({}, dict(POOL, TPE_DRAW_SCREEN_TAIL='128', TPE_DRAW_SCREEN_HALVES='6')):
        eager, _ = _child('case_graph', None, env)
        graph, _ = _child('case_graph', None, dict(env, TPE_GRAPH='1'))
        assert graph['hex'] == eager['hex'], env
        assert graph['stats'][0] > 0 and list(graph['stats']) == list(eager['stats']), env
        seen.append(list(graph['stats']))
    assert seen[0] != seen[1]                            # (the two settings do screen differently)


# ------------------------------------------------------------------------
# which sort blocks meet the pooled rows' edges
# ------------------------------------------------------------------------
def case_lists(path=None):
    """TPE_DRAW_PRUNE=0 child: every draw of suggestions 0 and 3 in draw order
    (Plan.cand_dump writes all tiles) with the launch's hot intervals
    (Plan.tab_hot), for the default and the few-below set.  Per (fit, label,
    suggestion) and (tail, halves): the zones by tools/table_error.py's
    draw_zones, and per sort block behind the pilot's the elements of each
    wave's rows that lie in a zone -- its list, but for the few elements within
    the thresholds' margin of a zone edge -- and whether the block's key range
    comes from them (the first condition of a screened block)."""
    out = {}
    space = {'a': (-5, 5), 'b': (0, 1), 'c': (-300, -100), 'd': (2, 2.5)}
    for fit in ('default', 'few-below'):
        dom, plan = _plan_a(fit)
        plan.suggest(SEEDS, NC)
        hot = plan.tab_hot(len(SEEDS))
        for lab in LABELS_A:
            i = dom.space.by_label[lab].index
            center = 0.5 * (space[lab][0] + space[lab][1])
            for s in (0, 3):
                v, p = plan.cand_dump(s, i)
                x = np.empty(NC)
                x[p] = v
                h = hot[s, i]
                iv = [(l, u) for l, u in zip(h[2:10], h[10:18]) if l <= u]
                for tail, halves in ((24, 4), (128, 4)):
                    z = TE.draw_zones(x[:SORT], iv, h[0], h[1], center, 2, tail=tail, halves=halves)
                    if z is None:
                        continue
                    zlo, zhi = z
                    rows = []
                    for b0 in range(SORT, NC, SORT):
                        xb = x[b0:b0 + SORT]
                        inz = ((xb[:, None] >= zlo[None, :]) & (xb[:, None] <= zhi[None, :])).any(axis=1)
                        per = -(-xb.size // 512) * 64
                        lists = [int(inz[w * per:(w + 1) * per].sum()) for w in range(8)]
                        ranged = bool(inz.any() and xb[inz].min() <= zhi[0] and xb[inz].max() >= zlo[-1])
                        rows.append((lists, ranged))
                    out['%s/%s/%d/%d/%d' % (fit, lab, s, tail, halves)] = rows
    return out


def _child_lists(env=None):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, json; sys.path.insert(0, 'tests'); import test_gpu_draw_screen_dense as P; "
            "print('JSON' + json.dumps(P.case_lists()))")
    r = subprocess.run([sys.executable, '-c', code], cwd=root,
                       env=dict(os.environ, TPE_DRAW_SCREEN_MIN='0', TPE_DRAW_PRUNE='0', **(env or {})),
                       capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.split('JSON')[-1])


def test_pooled_rows_meet_their_edges():
    """The byte comparisons above run pooled rows with an empty list beside
    others, a block total under 64, a last row that is partly filled, and a
    list past kScreenList: among the sort blocks whose key range comes from
    listed elements there is
     - under the defaults a 77-candidate block (sort block 33) with listed
       elements in waves 0 and 1 at the most and a total under 64, and more
       such blocks under tail 128;
     - under the defaults a whole block of the few-below set whose total is no
       multiple of 64;
     - under TPE_TABLE_TIE_LOG2=0 a block with a list of more than 640."""
    rows = _child_lists()
    for rule in ('/24/4', '/128/4'):
        short = [(k, r[-1][0]) for k, r in rows.items() if k.endswith(rule) and r[-1][1]]
        print('77-candidate blocks with a key range from listed elements, %s: %s' % (rule, short))
        assert short, rule
        for k, lists in short:
            assert 0 < sum(lists) < 64 and lists[2:] == [0] * 6, (k, lists)
    assert sum(1 for k, r in rows.items() if k.endswith('/128/4') and r[-1][1]) > \
        sum(1 for k, r in rows.items() if k.endswith('/24/4') and r[-1][1])
    few = [(k, b + 1, r[b][0]) for k, r in rows.items() if k.startswith('few-below/') and
           k.endswith('/24/4') for b in range(32) if r[b][1] and sum(r[b][0]) % 64]
    print('few-below whole blocks, defaults: %d; the first: %s' % (len(few), few[:2]))
    assert few
    over = [(k, b + 1, r[b][0]) for k, r in _child_lists(TIE0).items() if k.endswith('/24/4')
            for b in range(32) if r[b][1] and max(r[b][0]) > 640]
    print('tie=0 blocks with a list over 640: %d; the first: %s' % (len(over), over[:2]))
    assert over
