"""The pending batch on the GPU at its kernel edges (tpe_batch.hip; DESIGN
5.16), on ``batch_edge_cases``' fixtures -- ``test_batch_edges_host.py`` proves
that each wrong rule of the update moves some entry of them by more than 4x
the bound used here.

One-hp spaces of every kind, the picks crafted onto the edges of
``pending_record``'s sigma search, the lattice of the quantized kinds and every
option of the categorical ones: the picks are the rule applied to the device's
own trace, and every entry of every round lies within
``batch_oracle.score_bound`` of the oracle replayed on the device's picks.
For ``uniform`` and ``normal`` the update is also replayed in float64 from the
device's own sides, to a derived allowance of a few ulp.  Then the launch
shapes no other test reaches: more than 256 blocks, k = BATCH_MAX, and a short
batch in device mode."""
import functools

import numpy as np
import pytest

from hyperopt_amd import _engine as E

import batch_edge_cases as X
import batch_oracle as B
from test_gpu_batch import _same, _batch, _check_identities, _check_trace

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _plan(name, n=None):
    dom, losses, vals, active = X.history(name, n)
    hps, conds, pprior = dom.space.engine_tables()
    plan = E.Plan(E.default_engine(), hps, conds, pprior, max_trials=losses.size)
    plan.set_history(np.ascontiguousarray(losses), np.ascontiguousarray(vals),
                     np.ascontiguousarray(active))
    plan.fit(gamma=X.GAMMA, prior_weight=X.PRIOR_WEIGHT)
    plan.group_fit()
    return plan


def _run(plan, case):
    """The case on the device, checked against the rule and the oracle; the
    worst |d| / bound over every entry of every round."""
    vals = np.ascontiguousarray(case.vals)
    total, idx, gain, trace = _batch(plan, vals, case.k, eligible=case.eligible)
    _check_identities(plan, case.model, vals, case.k, total, idx, gain, trace,
                      eligible=case.eligible, msg=case.name)
    res = _check_trace(case.model, vals, idx, trace, eligible=case.eligible, msg=case.name)
    with np.errstate(all='ignore'):
        r = np.abs(trace - res.scores) / res.bound
    return idx, trace, float(np.max(np.where(np.isnan(res.scores), 0.0, r)))


# ------------------------------------------------------------------ the edges
@pytest.mark.parametrize('kind', list(X.KINDS))
def test_one_hp_edges_match_the_oracle(kind):
    worst = 0.0
    for n in X.SIZES:
        case = X.case(kind, n)
        idx, trace, r = _run(_plan(kind, n), case)
        assert sorted(idx.tolist()) == list(range(case.k))
        worst = max(worst, r)
    print('%s: worst |d score| / bound over n = 1, 2, 40, 140: %.3g' % (kind, worst))


def test_two_branch_counts_each_groups_picks():
    case = X.two_branch_case()
    idx, trace, r = _run(_plan('two_branch'), case)
    np.testing.assert_array_equal(idx, X.oracle_run(case).picks)
    print('two_branch: worst |d score| / bound = %.3g' % r)


def test_many_dists_picks_are_the_oracles():
    case = X.many_dists_case()
    idx, trace, r = _run(_plan('many_dists'), case)
    np.testing.assert_array_equal(idx, X.oracle_run(case).picks)
    print('many_dists: worst |d score| / bound = %.3g' % r)


@pytest.mark.parametrize('kind', X.EXACT_MU)
def test_update_arithmetic_from_the_devices_own_sides(kind):
    """mu = x exactly, so the rounds can be replayed in float64 numpy from the
    device's sides of round 0 and its own mixture, and only the update's
    arithmetic differs.  Allowance (derived, not measured):
    |trace[t] - replay[t]| <= 64 eps (t + 1) (|J_b| + |Ja_t| + |lk| + log(W + 1) + 1):
    a round has fewer than 8 rounded operations, each at most 2 ulp of a
    quantity inside the bracket, logaddexp does not amplify, and a factor 4 of
    margin."""
    worst = 0.0
    for n in X.SIZES:
        case, plan = X.case(kind, n), _plan(kind, n)
        vals = np.ascontiguousarray(case.vals)
        m = vals.shape[1]
        _, idx, _, trace = _batch(plan, vals, case.k, eligible=case.eligible)
        jb, ja = plan.group_sides(0, m)
        mus = np.sort(plan.group_mixture(0, 0, side=1)[1])
        rep = X.replay(case.model, vals, idx, sides=(jb[None, :], ja[None, :]), mus={0: mus})
        _same(trace[0], rep.scores[0], case.name)
        allow = X.tight_allowance(jb, rep)
        assert np.isfinite(rep.scores).all() and np.isfinite(allow).all()
        r = np.abs(trace - rep.scores) / allow
        print('%s: worst |d score| / allowance = %.3g' % (case.name, r.max()))
        assert (r <= 1.0).all(), (case.name, np.argwhere(r > 1.0)[:5], r.max())
        worst = max(worst, float(r.max()))
    print('%s: worst |d score| / allowance over n = 1, 2, 40, 140: %.3g' % (kind, worst))


# ----------------------------------------------------- launch shapes and limits
def test_more_slots_than_one_pass_of_the_pick_kernel():
    """m = 65536 + 300: 258 blocks, so k_batch_pick's 256 threads walk the
    slots twice; the best eligible configuration lies in the last block."""
    case = X.slot_case()
    res = X.oracle_run(case)
    assert res.picks[0] == X.SLOT_BEST and (res.ratio > 4.0).all()
    assert set((res.picks // X.BLOCK).tolist()) == {256, 257}
    idx, trace, r = _run(_plan(X.SHAPE_KIND, X.SHAPE_N), case)
    np.testing.assert_array_equal(idx, res.picks)
    print('slots: worst |d score| / bound = %.3g' % r)


def test_the_largest_batch():
    case = X.kmax_case(E.BATCH_MAX)
    plan = _plan(X.SHAPE_KIND, X.SHAPE_N)
    idx, trace, r = _run(plan, case)
    assert trace.shape == (E.BATCH_MAX, X.KMAX_M)
    print('k = %d: worst |d score| / bound over all rounds = %.3g' % (E.BATCH_MAX, r))
    with pytest.raises(ValueError, match='1 <= k <= 1024'):
        plan.group_batch_points(np.ascontiguousarray(case.vals), E.BATCH_MAX + 1)


def test_a_short_batch_in_device_mode():
    """Three eligible configurations, k = 5: the call raises, the three are
    picked in rule order, idx is -1 and gain NaN from the first round without
    a selectable configuration, and nothing else is written."""
    case, plan = X.case(X.SHAPE_KIND, X.SHAPE_N), _plan(X.SHAPE_KIND, X.SHAPE_N)
    vals = np.ascontiguousarray(case.vals)
    eng, m, k = plan.engine, vals.shape[1], 5
    ld = m + 9
    few = np.zeros(m, dtype=np.uint8)
    few[[1, 4, m - 1]] = 1
    pad = np.full((1, ld), np.nan)
    pad[:, :m] = vals
    v = E.DeviceBuffer(eng, 8 * ld).upload(pad)
    el = E.DeviceBuffer(eng, m).upload(few)
    tot = E.DeviceBuffer(eng, 8 * ld).upload(np.full(ld, -7.0))
    d_idx = E.DeviceBuffer(eng, 4 * (k + 1))
    d_gain = E.DeviceBuffer(eng, 8 * (k + 1))
    d_trace = E.DeviceBuffer(eng, 8 * k * ld)

    def call(k_):
        d_idx.upload(np.full(k + 1, -7, dtype=np.int32))
        d_gain.upload(np.full(k + 1, -7.0))
        d_trace.upload(np.full((k, ld), -7.0))
        plan.group_score_points_device(v.ptr, m, ld, tot.ptr)
        try:
            plan.group_batch_points_device(v.ptr, m, ld, k_, d_idx.ptr, d_gain.ptr,
                                           eligible_ptr=el.ptr, trace_ptr=d_trace.ptr)
        finally:
            eng.synchronize()
        return (d_idx.download(np.empty(k + 1, dtype=np.int32)), d_gain.download(np.empty(k + 1)),
                d_trace.download(np.empty((k, ld))))

    with pytest.raises(ValueError, match='fewer than k'):
        call(k)
    di = d_idx.download(np.empty(k + 1, dtype=np.int32))
    dg = d_gain.download(np.empty(k + 1))
    dt = d_trace.download(np.empty((k, ld)))
    want = B.apply_rule(dt[:, :m], B.config_keys(case.model, vals), few != 0)
    assert sorted(di[:3].tolist()) == [1, 4, m - 1]
    np.testing.assert_array_equal(di[:k], want)
    assert list(want[3:]) == [-1, -1]
    assert np.isnan(dg[3:k]).all()
    _same(dg[:3], dt[np.arange(3), di[:3]])
    assert di[k] == -7 and dg[k] == -7.0 and (dt[:, m:] == -7.0).all()
    # the round that found nothing was still scored; the one after it did nothing
    assert (dt[4, :m] == -7.0).all()
    _check_trace(case.model, vals, di[:3], dt[:3, :m], eligible=few != 0, msg='short')
    # k = 3 then succeeds with the same picks
    di3, dg3, dt3 = call(3)
    np.testing.assert_array_equal(di3[:3], di[:3])
    _same(dg3[:3], dg[:3])
    _same(dt3[:3, :m], dt[:3, :m])
    assert (di3[3:] == -7).all() and (dt3[3:] == -7.0).all()
