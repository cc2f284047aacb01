"""The pruning sorted draw (k_draw_sorted_prune): behind
the prefilter the sort blocks after the pilot's neither rank nor write the
wave tiles the slot's hot intervals rule out; they leave -inf in tab_wmax, the
map and the gather leave those alone, and nothing downstream changes.

Suggests: test_gpu_table.py's shape (3 hps, N = 6000, 2^18 + 8192 + 37
candidates, SEEDS6: 34 sort blocks -- block 0 for the pilot, a 37-candidate
tail block and wave tiles past n_cand), its gap history (u's above table is
not certified: nothing dropped) and test_gpu_tie_gather.py's conditional plan
(compact grid, inactive slots).  The default run is compared with a child
interpreter under TPE_DRAW_PRUNE=0 (the switch is read once per process):
records and tie counts byte for byte; the default's -inf set contains the
child's, every other entry is bit-equal, and every extra -inf entry's score
in the child lies under the child's own tab_max - 2^-16 max(1, |tab_max|).
Plan.cand_dump: values and positions byte-equal on every wave tile that is
not -inf in the default.  A tile counts as dropped by the draw when it is -inf
and its positions in the default's dump are not the child's (it was never
written; a tile only the map's prefilter ruled out was): judged on the
process's first suggest, whose candidate buffer holds no earlier draw.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import test_gpu_table as T
import test_gpu_tie_gather as G
import test_gpu_table_scalar as S

pytestmark = pytest.mark.gpu

NC, NWT = T.NC, S.NWT
SEEDS6, SEEDS11 = T.SEEDS6, T.SEEDS11
SORT = 8192
WMAX = dict(plain=('u', 'lu'), gap=('u', 'lu'), cond=('u', 'a', 'b'))
DUMPS = dict(plain=[(0, 'u'), (0, 'lu'), (5, 'u'), (5, 'lu')], gap=[(0, 'u'), (0, 'lu')],
             cond=[(0, 'a'), (0, 'b'), (3, 'a'), (3, 'b')])
NEG_INF = np.array([-np.inf]).view(np.uint64)[0]


def _dump(dom, plan, kind, arrays):
    for s, lab in DUMPS[kind]:
        v, p = plan.cand_dump(s, dom.space.by_label[lab].index)
        assert v.shape == (NC,) and p.shape == (NC,)
        arrays['%s_%d_%s_v' % (kind, s, lab)] = v.view(np.uint64)
        arrays['%s_%d_%s_p' % (kind, s, lab)] = p


def case_all(path, repeat=False):
    """Every suggest of the module; the dumps go to the .npz file `path`."""
    arrays = {}
    dom, plan, _ = T._plan()
    out = dict(plain=S._suggest(dom, plan, SEEDS6, WMAX['plain']))
    _dump(dom, plan, 'plain', arrays)
    if repeat:
        out['again'] = S._suggest(dom, plan, SEEDS6, WMAX['plain'])
        dom, plan, _ = T._plan()
        out['fresh'] = S._suggest(dom, plan, SEEDS6, WMAX['plain'])
    dom, plan, _ = T._plan(True)
    out['gap'] = S._suggest(dom, plan, SEEDS6, WMAX['gap'])
    _dump(dom, plan, 'gap', arrays)
    dom, plan = G._cond_plan()
    out['cond'] = S._suggest(dom, plan, SEEDS11, WMAX['cond'])
    _dump(dom, plan, 'cond', arrays)
    np.savez(path, **arrays)
    return out


def case_plain(path):
    arrays = {}
    dom, plan, _ = T._plan()
    out = dict(plain=S._suggest(dom, plan, SEEDS6, WMAX['plain']))
    _dump(dom, plan, 'plain', arrays)
    np.savez(path, **arrays)
    return out


@pytest.fixture(scope='module')
def tmpdir_mod():
    with tempfile.TemporaryDirectory() as d:
        yield d


def _child(case, path, env):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, json; sys.path.insert(0, 'tests'); import test_gpu_draw_prune as P; "
            "print('JSON' + json.dumps(P.%s(%r)))" % (case, path))
    r = subprocess.run([sys.executable, '-c', code], cwd=root, env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.split('JSON')[-1]), dict(np.load(path))


@pytest.fixture(scope='module')
def on_run(tmpdir_mod):
    assert os.environ.get('TPE_DRAW_PRUNE', '1') != '0', 'the default is under test'
    assert os.environ.get('TPE_TABLE_PREFILTER', '1') != '0', 'the default is under test'
    path = os.path.join(tmpdir_mod, 'on.npz')
    return case_all(path, repeat=True), dict(np.load(path))


@pytest.fixture(scope='module')
def off_run(tmpdir_mod):
    return _child('case_all', os.path.join(tmpdir_mod, 'off.npz'), {'TPE_DRAW_PRUNE': '0'})


def _bits(run, lab, n_sug):
    return np.frombuffer(bytes.fromhex(run['wmax_' + lab]), dtype=np.uint64).reshape(n_sug, NWT)


def _tiles(a):
    """[NC] -> [NWT][128], the last wave tile padded with the array's last entry."""
    pad = NWT * 128 - a.size
    return np.concatenate([a, np.repeat(a[-1:], pad)]).reshape(NWT, 128)


def check_wmax_pair(a, b, ctx):
    """One (suggestion, hp)'s tab_wmax bits of the default run (a) and of the
    TPE_DRAW_PRUNE=0 child (b): a's -inf set contains b's, every other entry
    is bit-equal, every extra -inf tile scores under the child's own tie
    threshold, and some tiles are -inf but not all.  Returns the -inf share of
    a and the number of extra -inf entries."""
    da, db = a == NEG_INF, b == NEG_INF
    assert not (db & ~da).any()        # the default's -inf set contains the child's
    np.testing.assert_array_equal(a[~da], b[~da])
    extra = da & ~db
    w = b.view(np.float64)
    real = w[~db]
    tab_max = np.nan if np.isnan(real).any() else real.max()
    thr = tab_max - 2.0 ** -16 * max(1.0, abs(tab_max))
    assert (w[extra] < thr).all(), ctx + (float(w[extra].max()), thr)
    assert da.any() and not da.all(), ctx + (int(da.sum()),)
    return da.mean(), int(extra.sum())


@pytest.mark.parametrize('kind', ['plain', 'gap', 'cond'])
def test_draw_prune_changes_nothing_downstream(on_run, off_run, kind):
    (on, on_d), (off, off_d) = on_run, off_run
    on, off = on[kind], off[kind]
    n_sug = len(SEEDS11 if kind == 'cond' else SEEDS6)
    assert on['labels'] == off['labels']
    assert on['hex'] == off['hex']
    assert on['counts'] == off['counts']
    cnt = np.asarray(on['counts'])
    for lab in WMAX[kind]:
        a, b = _bits(on, lab, n_sug), _bits(off, lab, n_sug)
        c = cnt[:, on['labels'].index(lab)]
        if kind == 'gap' and lab == 'u':       # no certified pair: the draw drops nothing
            assert not (a == NEG_INF).any()
            continue
        fracs, extras = [], 0
        for s in range(n_sug):
            if c[s] == 0:                      # (cond: inactive, its wave scores are stale)
                continue
            frac, extra = check_wmax_pair(a[s], b[s], (kind, lab, s))
            fracs.append(frac)
            extras += extra
        assert fracs, (kind, lab)
        print('%s %s: -inf share of the wave tiles min %.4f median %.4f max %.4f; '
              '%d entries -inf beyond the map prefilter\'s' %
              (kind, lab, min(fracs), float(np.median(fracs)), max(fracs), extras))


@pytest.mark.parametrize('kind', ['plain', 'gap', 'cond'])
def test_cand_dump_on_kept_tiles(on_run, off_run, kind):
    (on, on_d), (off, off_d) = on_run, off_run
    n_sug = len(SEEDS11 if kind == 'cond' else SEEDS6)
    cnt = np.asarray(on[kind]['counts'])
    seen = 0
    for s, lab in DUMPS[kind]:
        if cnt[s, on[kind]['labels'].index(lab)] == 0:    # (cond: the inactive branch)
            continue
        seen += 1
        key = '%s_%d_%s_' % (kind, s, lab)
        kept = _bits(on[kind], lab, n_sug)[s] != NEG_INF
        va, vb = _tiles(on_d[key + 'v']), _tiles(off_d[key + 'v'])
        pa, pb = _tiles(on_d[key + 'p']), _tiles(off_d[key + 'p'])
        np.testing.assert_array_equal(va[kept], vb[kept])
        np.testing.assert_array_equal(pa[kept], pb[kept])
        # the child's positions: a permutation of each sort block's own range;
        # the default's kept ones are those, so distinct and inside the block
        full = off_d[key + 'p']
        for b0 in range(0, NC, SORT):
            blk = full[b0:b0 + SORT]
            np.testing.assert_array_equal(np.sort(blk), np.arange(b0, b0 + blk.size))
        if kind == 'gap' and lab == 'u':
            assert kept.all()
            np.testing.assert_array_equal(on_d[key + 'p'], off_d[key + 'p'])
        if kind == 'plain':
            # never written: -inf and not the child's positions (the first
            # suggest of this process: no earlier draw left them there)
            dropped = ~kept & (pa != pb).any(axis=1)
            assert dropped.any(), (lab, s)
            assert not dropped[:SORT // 128].any()         # the pilot's sort block is whole
            print('%s s=%d: %d of %d wave tiles dropped by the draw, %d -inf in all'
                  % (lab, s, int(dropped.sum()), NWT, int((~kept).sum())))
    assert seen >= 2, kind


def test_repeatable(on_run):
    """The same plan suggested twice and a fresh plan: the same tab_wmax bytes
    (the draw's -inf marks included), the same records and counts."""
    on, _ = on_run
    first = on['plain']
    for other in (on['again'], on['fresh']):
        for k in ('hex', 'counts') + tuple('wmax_' + l for l in WMAX['plain']):
            assert other[k] == first[k], k


def test_wide_window_drops_nothing(off_run, tmpdir_mod):
    """TPE_TABLE_TIE_LOG2=2000: the hot interval is everything -- no -inf
    entry, and the dump is the TPE_DRAW_PRUNE=0 child's everywhere."""
    wide, wide_d = _child('case_plain', os.path.join(tmpdir_mod, 'wide.npz'), dict(G.WIDE))
    _, off_d = off_run
    for lab in WMAX['plain']:
        assert not (_bits(wide['plain'], lab, len(SEEDS6)) == NEG_INF).any(), lab
    for k, v in wide_d.items():
        np.testing.assert_array_equal(v, off_d[k], err_msg=k)
