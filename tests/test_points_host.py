"""Host side of tpe.score_configs / tpe.suggest_from_pool (no GPU): the
configuration <-> column conversion, the activity a configuration's own values
imply, the contradiction check, skip_seen, the ranking rule, the startup
branch, and the C entry point's argument check on the loaded library."""
import ctypes
import os

import numpy as np
import pytest

import hyperopt_amd as H
from hyperopt_amd import hp, rand, tpe, Trials, trials_from_docs
from hyperopt_amd.base import Domain

import spaces

SPACES = {'many_dists': spaces.many_dists_space, 'cond': spaces.cond_space}


def _domain(name):
    return Domain(lambda x: 0.0, SPACES[name](hp))


def _prior_configs(dom, n, seed):
    """n configurations drawn from the prior, as {label: value} dicts of the
    active labels (what fmin returns)."""
    docs = rand.suggest(list(range(n)), dom, Trials(), seed)
    return docs, [{lab: v[0] for lab, v in d['misc']['vals'].items() if v} for d in docs]


def _done(docs, seed):
    for d, l in zip(docs, np.random.RandomState(seed).rand(len(docs))):
        d['state'] = H.JOB_STATE_DONE
        d['result'] = {'status': 'ok', 'loss': float(l)}
    return trials_from_docs(docs)


@pytest.mark.parametrize('name', sorted(SPACES))
def test_dicts_to_columns_and_back(name):
    dom = _domain(name)
    cs = dom.space
    _, cfgs = _prior_configs(dom, 40, 3)
    vals, present = tpe.config_columns(cs, cfgs)
    assert vals.shape == (len(cs.labels), 40) and vals.dtype == np.float64
    for j, c in enumerate(cfgs):
        for i, lab in enumerate(cs.labels):
            assert present[i, j] == (lab in c)
            if lab in c:
                assert vals[i, j] == c[lab]
            else:
                assert np.isnan(vals[i, j])
    # the activity the values imply is exactly the labels the prior draw set,
    # and agrees with CompiledSpace.is_active label by label
    act = tpe.active_columns(cs, vals)
    np.testing.assert_array_equal(act, present)
    for j, c in enumerate(cfgs):
        for i, lab in enumerate(cs.labels):
            assert act[i, j] == cs.is_active(lab, c)
    back = tpe.columns_to_configs(cs, vals, act)
    assert back == cfgs
    for c in back:
        for lab, v in c.items():
            assert isinstance(v, int) == cs.by_label[lab].is_categorical
    # an array in label order (NaN for absent) is the same pool
    v2, p2 = tpe.config_columns(cs, vals)
    np.testing.assert_array_equal(p2, present)
    np.testing.assert_array_equal(v2[present], vals[present])


def test_column_conversion_rejects_bad_input():
    cs = _domain('cond').space
    with pytest.raises(ValueError):
        tpe.config_columns(cs, [{'nope': 1.0}])
    with pytest.raises(ValueError):
        tpe.config_columns(cs, np.zeros((3, 5)))


def test_inactive_garbage_does_not_change_activity():
    cs = _domain('cond').space
    _, cfgs = _prior_configs(_domain('cond'), 30, 5)
    vals, present = tpe.config_columns(cs, cfgs)
    junk = np.where(present, vals, 1.0)     # 1.0 is a valid branch index
    np.testing.assert_array_equal(tpe.active_columns(cs, junk), present)


def test_invalid_choice_activates_no_child():
    cs = _domain('cond').space
    _, cfgs = _prior_configs(_domain('cond'), 4, 5)
    vals, _ = tpe.config_columns(cs, cfgs)
    top = cs.labels.index('top')
    vals[top] = [3.0, 1.5, np.nan, -1.0]    # upper, a fraction, NaN, negative
    vals[np.isnan(vals)] = 0.5
    vals[top, 2] = np.nan
    act = tpe.active_columns(cs, vals)
    for i, lab in enumerate(cs.labels):
        assert act[i].all() == (lab in ('top', 'aa')), lab
        assert act[i].any() == (lab in ('top', 'aa')), lab


def test_contradicting_dict_raises():
    dom = _domain('cond')
    _, cfgs = _prior_configs(dom, 6, 9)
    good = cfgs[0]
    b = int(good['top'])
    other = (b + 1) % 3
    # a label present under a branch not taken
    extra = dict(good)
    extra['lr%d' % other] = 0.01
    # a label missing under the taken branch
    short = {k: v for k, v in good.items() if k != 'lr%d' % b}
    for bad, word in ((extra, 'present'), (short, 'missing')):
        with pytest.raises(ValueError, match=word):
            tpe.suggest_from_pool([0], dom, Trials(), 1, pool=[good, bad])
    # the consistent pool passes (startup branch: no engine needed)
    assert len(tpe.suggest_from_pool([0], dom, Trials(), 1, pool=cfgs)) == 1


def test_seen_in_history_marks_exactly_the_history_rows():
    dom = _domain('cond')
    cs = dom.space
    docs, cfgs = _prior_configs(dom, 50, 11)
    hv, hp_ = tpe.config_columns(cs, cfgs[:20])
    hist_vals = np.where(hp_, hv, 0.0)      # the history keeps 0.0 in inactive slots
    pool_vals, pool_present = tpe.config_columns(cs, cfgs[10:])     # 10 seen, 30 new
    pool_act = tpe.active_columns(cs, pool_vals)
    seen = tpe.seen_in_history(pool_vals, pool_act, hist_vals, hp_.astype(np.uint8))
    np.testing.assert_array_equal(seen, np.arange(40) < 10)
    # what an inactive slot holds does not matter, the sign of zero neither
    junk = np.where(pool_present, pool_vals, -7.0)
    neg0 = np.where(hp_ & (hv != 0.0), hv, -0.0)
    np.testing.assert_array_equal(
        tpe.seen_in_history(junk, pool_act, neg0, hp_.astype(np.uint8)), seen)
    # an empty history has seen nothing
    assert not tpe.seen_in_history(pool_vals, pool_act, hist_vals[:, :0], hp_[:, :0]).any()


def test_skip_seen_leaves_too_few_raises_before_any_device_work():
    dom = _domain('cond')
    docs, cfgs = _prior_configs(dom, 25, 13)
    trials = _done(docs, 1)
    with pytest.raises(ValueError, match='eligible'):
        tpe.suggest_from_pool([25], dom, trials, 1, pool=cfgs, n_startup_jobs=0)
    with pytest.raises(ValueError, match='eligible'):
        tpe.suggest_from_pool([25, 26], dom, trials, 1, pool=cfgs + [cfgs[3]], n_startup_jobs=0)


def test_rank_pool_order():
    total = np.array([1.0, np.nan, 3.0, 3.0, -np.inf, 2.0, np.inf])
    every = np.ones(7, dtype=bool)
    np.testing.assert_array_equal(tpe.rank_pool(total, every, 7), [6, 2, 3, 5, 0, 4, 1])
    np.testing.assert_array_equal(tpe.rank_pool(total, every, 2), [6, 2])
    some = np.array([1, 1, 0, 1, 1, 0, 0], dtype=bool)
    np.testing.assert_array_equal(tpe.rank_pool(total, some, 4), [3, 0, 4, 1])


@pytest.mark.parametrize('as_array', [False, True])
def test_startup_branch_picks(as_array):
    dom = _domain('cond')
    cs = dom.space
    _, cfgs = _prior_configs(dom, 30, 17)
    vals, _ = tpe.config_columns(cs, cfgs)
    pool = vals if as_array else cfgs
    docs, _ = _prior_configs(dom, 5, 2)
    trials = _done(docs, 4)                 # 5 < n_startup_jobs = 20
    new_ids = [5, 6, 7]
    out = tpe.suggest_from_pool(new_ids, dom, trials, 123, pool=pool)
    want = np.random.RandomState(123).choice(30, 3, replace=False)
    assert [d['tid'] for d in out] == new_ids
    for d, w, nid in zip(out, want, new_ids):
        got = {lab: v[0] for lab, v in d['misc']['vals'].items() if v}
        assert got == cfgs[w]
        assert d['misc']['idxs'] == {lab: ([nid] if lab in cfgs[w] else []) for lab in cs.labels}
    with pytest.raises(ValueError):
        tpe.suggest_from_pool(list(range(31)), dom, trials, 1, pool=pool)
    assert tpe.suggest_from_pool([], dom, trials, 1, pool=pool) == []


def test_array_pool_is_converted_once_per_domain():
    dom = _domain('cond')
    _, cfgs = _prior_configs(dom, 12, 19)
    vals, _ = tpe.config_columns(dom.space, cfgs)
    tpe.suggest_from_pool([0], dom, Trials(), 1, pool=vals)
    first = dom._tpe_state.pool
    tpe.suggest_from_pool([1], dom, Trials(), 2, pool=vals)
    assert dom._tpe_state.pool is first and first.source is vals
    tpe.suggest_from_pool([2], dom, Trials(), 3, pool=vals.copy())
    assert dom._tpe_state.pool is not first


def test_score_configs_needs_a_history():
    dom = _domain('cond')
    _, cfgs = _prior_configs(dom, 3, 1)
    with pytest.raises(ValueError, match='history'):
        tpe.score_configs(cfgs, dom, Trials())


def test_exported_from_the_package():
    assert H.score_configs is tpe.score_configs
    assert H.suggest_from_pool is tpe.suggest_from_pool


def test_score_points_rejects_a_null_plan():
    from hyperopt_amd import _engine as E
    if not os.path.exists(E.LIB_PATH):
        pytest.skip('libtpe_engine.so not built (run __graft_entry__.build())')
    lib = E.load_library()
    buf = (ctypes.c_double * 4)()
    addr = ctypes.addressof(buf)
    assert lib.tpe_plan_score_points(None, addr, 4, 4, addr, None, None, 0, None) == E.TPE_E_INVALID
    assert lib.tpe_plan_score_points(None, None, 0, 0, None, None, None, 1, None) == E.TPE_E_INVALID
