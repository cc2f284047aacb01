"""Time one device-resident joint draw -- tpe_plan_sample_points, the top 64
by tpe_plan_topk_points, their columns by tpe_plan_gather_points: the device
part of tpe.suggest_joint -- against the only way to the same picks without
those entry points: one Engine.sample call per hyperparameter with the plan's
below mixtures, tpe.active_columns on the host, Plan.score_points of the
masked array, a download and tpe.rank_pool.

Shapes: config 2's space (20 hps, 1000 trials) at 4096, 2^16 and 2^18
configurations; config 3's space (50 hps, conditional) at 2^16.  Per shape,
after warm-up, --reps rounds of, in this order in one process:
  joint     the three calls on device buffers, HIP events on the call's stream
            around them (sample + score + top-64 + gather);
  score     tpe_plan_score_points alone on the array the draw left (HIP
            events): what the draw, the selection and the gather add to it is
            joint - score;
  baseline  the host route's wall time, ending with the picks on the host (the
            mixtures are fetched once, outside the clock).
Each line gives the median with the 10th and 90th percentiles and the extremes
of the rounds.  The picks of the two routes are compared before anything is
timed.
usage: python tools/sample_time.py [--shapes cfg2:4096 ...] [--reps N] [--k 64]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from anneal_time import build  # noqa: E402  (config 2 / 3 domains and histories)


def below_mixtures(plan, cs):
    """Per hp, Engine.sample's arguments for its below mixture."""
    from hyperopt_amd import _engine as E
    out = []
    for i, t in enumerate(cs.engine_tables()[0]):
        w, mu, sg = plan.mixture(i, 0)
        cat = t.family == E.CAT
        out.append((t.family, w, None if cat else mu, None if cat else sg,
                    t.low if t.flags & E.HAS_LOW else None,
                    t.high if t.flags & E.HAS_HIGH else None,
                    t.q if t.flags & E.HAS_Q else None))
    return out


def baseline(plan, cs, mix, seed, m, k):
    """The host route: (picks[k], vals[P, m], total[m])."""
    import numpy as np
    from hyperopt_amd import tpe
    eng = plan.engine
    vals = np.empty((len(mix), m))
    for i, a in enumerate(mix):
        vals[i] = eng.sample(*a, seed=seed, stream=i, offset=0, n=m)
    vals[~tpe.active_columns(cs, vals)] = np.nan
    total = plan.score_points(vals)
    return tpe.rank_pool(total, np.ones(m, dtype=bool), k), vals, total


def spread(x):
    import numpy as np
    x = np.asarray(x)
    return '%.3f ms median (p10 %.3f, p90 %.3f, min %.3f, max %.3f)' % (
        np.median(x), np.percentile(x, 10), np.percentile(x, 90), x.min(), x.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', nargs='+',
                    default=['cfg2:4096', 'cfg2:65536', 'cfg2:262144', 'cfg3:65536'])
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--k', type=int, default=64)
    args = ap.parse_args()
    import numpy as np
    from hyperopt_amd import _engine as E
    E.load_library()                 # (before torch: one HIP runtime, _share_hip_runtime)
    import torch
    from hyperopt_amd import tpe
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    built = {}
    k, seed, warm = args.k, 12345, 3
    for shape in args.shapes:
        cfg, m = shape.split(':')
        m = int(m)
        if cfg not in built:
            built[cfg] = build(cfg)
        dom, t = built[cfg]
        cs = dom.space
        tpe.sample_configs(8, dom, t, 1)        # builds plan + mirror, fits
        plan = dom._tpe_state.plan
        P = plan.n_hp
        mix = below_mixtures(plan, cs)
        dv = torch.empty((P, m), dtype=torch.float64, device='cuda')
        dt = torch.empty(m, dtype=torch.float64, device='cuda')
        dt2 = torch.empty(m, dtype=torch.float64, device='cuda')
        di = torch.empty(k, dtype=torch.int32, device='cuda')
        do = torch.empty((P, k), dtype=torch.float64, device='cuda')
        torch.cuda.synchronize()

        def joint():
            plan.sample_points_device(seed, 0, m, m, dv.data_ptr(), dt.data_ptr(), stream=st)
            plan.topk_points(dt.data_ptr(), k, m=m, out=di.data_ptr(), stream=st)
            plan.gather_points(dv.data_ptr(), di.data_ptr(), k=k, ld=m, out=do.data_ptr(),
                               stream=st)

        # the two routes give the same picks
        joint()
        stream.synchronize()
        picks, bvals, btotal = baseline(plan, cs, mix, seed, m, k)
        assert np.array_equal(di.cpu().numpy(), picks)
        assert np.array_equal(dv.cpu().numpy(), bvals, equal_nan=True)
        assert np.array_equal(dt.cpu().numpy(), btotal, equal_nan=True)
        assert np.array_equal(do.cpu().numpy(), bvals[:, picks], equal_nan=True)
        active = int((~np.isnan(bvals)).sum())
        j_ms, s_ms, b_ms = [], [], []
        for r in range(args.reps + warm):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            joint()
            b.record(stream)
            b.synchronize()
            c, d = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            c.record(stream)
            plan.score_points_device(dv.data_ptr(), m, m, dt2.data_ptr(), stream=st)
            d.record(stream)
            d.synchronize()
            t0 = time.perf_counter()
            baseline(plan, cs, mix, seed, m, k)
            wall = 1e3 * (time.perf_counter() - t0)
            if r >= warm:
                j_ms.append(a.elapsed_time(b))
                s_ms.append(c.elapsed_time(d))
                b_ms.append(wall)
        assert torch.equal(dt, dt2)
        tag = '%s M=%d' % (cfg, m)
        print('%s joint    sample + score + top-%d + gather %s, n=%d P=%d, active (hp, config) '
              'pairs %d of %d' % (tag, k, spread(j_ms), plan.n, P, active, P * m))
        print('%s score    score_points_device alone on the drawn array %s; the draw, the '
              'selection and the gather add %.3f ms (medians)'
              % (tag, spread(s_ms), np.median(j_ms) - np.median(s_ms)))
        print('%s baseline %d Engine.sample calls + active_columns + score_points + rank_pool '
              '%s (wall); joint is %.1fx faster (medians, %d rounds, alternating)'
              % (tag, P, spread(b_ms), np.median(b_ms) / np.median(j_ms), len(j_ms)))
        sys.stdout.flush()


if __name__ == '__main__':
    main()
