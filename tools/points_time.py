"""Time tpe_plan_score_points (whole configurations under the fitted model)
against the only other way to get the same numbers: a loop of
Plan.score_candidates(hp, column) over every hyperparameter plus a host sum.

Shapes: config 2's space with a 1000-trial history at M = 4096 and 2^18
configurations; config 3's space (10 000 trials, conditional: 7 of 50 hps active
per configuration) at M = 2^16.  The pool is 4096 prior draws tiled to M
(a configuration's cost does not depend on its neighbours).  Per shape:
  device   one tpe_plan_score_points call on device buffers (HIP events on the
           call's stream around the call: activity + terms + sum), median of
           --reps calls after warm-up, alternating with
  loop     wall time of the per-hp loop on the same plan and pool
           (score_candidates of each hp's active column, terms summed on the
           host) -- and the fused call's own host-mode wall time beside it
  wall     tpe.score_configs end to end on the array pool (history sync, fit,
           upload of the pool, scoring, totals back)
  bound    the (configuration, component) pairs the call evaluates, the pairs
           per second that implies, and the time the same pairs take at the
           register-only rates of their arithmetic (tpe_microbench 3: the
           fp64 per-group-max log-sum-exp pair; 4: the quantized pair of two
           fp64 erf; 0: v_exp_f32 alone, one per log-sum-exp pair)
usage: python tools/points_time.py [--shapes cfg2:4096 cfg2:262144 cfg3:65536] [--reps N]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from anneal_time import build  # noqa: E402  (config 2 / 3 domains and histories)


def pool_columns(dom, m, seed=11, base=4096):
    """[P, m] columns (NaN where inactive) of `base` prior draws tiled to m."""
    import numpy as np
    from hyperopt_amd import rand, tpe, Trials
    docs = rand.suggest(list(range(base)), dom, Trials(), seed)
    cfgs = [{lab: v[0] for lab, v in d['misc']['vals'].items() if v} for d in docs]
    vals, _ = tpe.config_columns(dom.space, cfgs)
    return np.ascontiguousarray(vals[:, np.arange(m) % base])


def loop_scores(plan, vals, active):
    """The per-hp loop: each hp's active column through score_candidates."""
    import numpy as np
    total = np.zeros(vals.shape[1])
    for i in range(vals.shape[0]):
        on = active[i]
        if not on.any():
            continue
        lb, la, _, _ = plan.score_candidates(i, vals[i][on])
        total[on] += lb - la
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', nargs='+', default=['cfg2:4096', 'cfg2:262144', 'cfg3:65536'])
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    import numpy as np
    from hyperopt_amd import _engine as E
    E.load_library()                 # (before torch: one HIP runtime, _share_hip_runtime)
    import torch
    from hyperopt_amd import tpe
    stream = torch.cuda.Stream()
    built = {}
    for shape in args.shapes:
        cfg, m = shape.split(':')
        m = int(m)
        if cfg not in built:
            built[cfg] = build(cfg)
        dom, t = built[cfg]
        cs = dom.space
        vals = pool_columns(dom, m)
        active = tpe.active_columns(cs, vals)
        total0 = tpe.score_configs(vals, dom, t)           # builds plan + mirror, fits
        plan = dom._tpe_state.plan
        eng = plan.engine
        P = plan.n_hp
        # device time of the call, alternating with the per-hp loop's wall time
        dv = torch.from_numpy(vals).cuda()
        dt = torch.empty(m, dtype=torch.float64).cuda()
        torch.cuda.synchronize()
        ms, loop, host = [], [], []
        n_loop = max(3, args.reps // 4)
        for r in range(args.reps + 3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            plan.score_points_device(dv.data_ptr(), m, m, dt.data_ptr(), stream=stream.cuda_stream)
            b.record(stream)
            b.synchronize()
            if r >= 3:
                ms.append(a.elapsed_time(b))
            if 3 <= r < 3 + n_loop:
                t0 = time.perf_counter()
                lt = loop_scores(plan, vals, active)
                loop.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                ht = plan.score_points(vals)
                host.append(time.perf_counter() - t0)
        got = dt.cpu().numpy()
        assert np.array_equal(got, total0, equal_nan=True) and np.array_equal(ht, total0, equal_nan=True)
        fin = np.isfinite(lt) & np.isfinite(got)
        dmax = float(np.abs(lt - got)[fin].max())
        # pairs and the register-only price of their arithmetic
        lse = erf = 0.0
        for i, h in enumerate(cs.hps):
            if h.is_categorical:
                continue
            k = plan.mixture(i, 0)[0].size + plan.mixture(i, 1)[0].size
            if h.dist.startswith('q'):
                erf += float(active[i].sum()) * k
            else:
                lse += float(active[i].sum()) * k
        dev_ms = float(np.median(ms))
        r_exp, r_lse, r_erf = eng.microbench(0), eng.microbench(3), eng.microbench(4)
        bound_ms = 1e3 * (lse / r_lse + erf / r_erf)
        tag = '%s M=%d' % (cfg, m)
        print('%s device  score_points %.3f ms median (p90 %.3f ms), n=%d P=%d, active (hp, config) '
              'pairs %d of %d' % (tag, dev_ms, float(np.percentile(ms, 90)), plan.n, P,
                                  int(active.sum()), active.size))
        print('%s loop    per-hp score_candidates loop + host sum %.2f ms, fused host-mode call '
              '%.2f ms (wall, median of %d, alternating); max |loop - fused| = %.2e'
              % (tag, 1e3 * np.median(loop), 1e3 * np.median(host), len(loop), dmax))
        lat = []
        for i in range(max(3, args.reps // 4)):
            t0 = time.perf_counter()
            tpe.score_configs(vals, dom, t)
            lat.append(time.perf_counter() - t0)
        print('%s wall    tpe.score_configs %.2f ms (median of %d: sync + fit + upload + score + '
              'totals)' % (tag, 1e3 * np.median(lat), len(lat)))
        print('%s bound   %.3e log-sum-exp + %.3e quantized pairs: %.3e pairs/s; at the '
              'register-only pair rates (%.2e, %.2e /s) %.3f ms = %.0f %% of the call; one '
              'v_exp_f32 per log-sum-exp pair at %.2e /s: %.3f ms'
              % (tag, lse, erf, (lse + erf) / (1e-3 * dev_ms), r_lse, r_erf, bound_ms,
                 100.0 * bound_ms / dev_ms, r_exp, 1e3 * lse / r_exp))


if __name__ == '__main__':
    main()
