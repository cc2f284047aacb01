"""Device time of c-TPE beside the plain whole-configuration
calls of the same build, in one session.

Config 2's space (20 hps) with a 1000-trial history; C = 1, 4, 16 constraints,
each feasible in about half of the rows, so every model is live (n_live = C +
1).  Per C and size, HIP events on the call's stream, median of --reps after
warm-up, the two variants alternating inside one loop:
  fit + score   tpe_plan_fit + tpe_plan_score_points against tpe_plan_ctpe_fit
                (host G: the copy is inside the window) + tpe_plan_ctpe_score_points,
                M = 4096 and 2^18 pool configurations (tools/points_time.py's)
  draw + top 64 tpe_plan_sample_points + tpe_plan_topk_points against
                tpe_plan_ctpe_sample_points + the same top-k, n = 4096 and 2^16
                (tools/sample_time.py's)
The expectation is about n_live times the plain call; the ratio is recorded,
not gated on.
usage: python tools/ctpe_time.py [--reps 20] [--out profiles/ctpe_time.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from anneal_time import build  # noqa: E402  (config 2's domain and history)
from points_time import pool_columns  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ctpe_time.txt'))
    args = ap.parse_args()
    import numpy as np
    from hyperopt_amd import _engine as E
    E.load_library()                 # (before torch: one HIP runtime, _share_hip_runtime)
    import torch
    from hyperopt_amd import tpe
    stream = torch.cuda.Stream()
    out = open(args.out, 'w') if args.out else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + '\n')
            out.flush()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    dom, t = build('cfg2')
    _, losses, hv, ha = tpe.build_history(dom, t)
    hps, conds, pprior = dom.space.engine_tables()
    plan = E.Plan(E.default_engine(), hps, conds, pprior, max_trials=losses.size)
    plan.set_history(losses, hv, ha)
    P, s = plan.n_hp, stream.cuda_stream
    say('c-TPE device time, config 2 (P = %d, %d trials), median of %d after 3 warm-up calls'
        % (P, losses.size, args.reps))
    for C in (1, 4, 16):
        G = np.ascontiguousarray(np.random.RandomState(C).rand(C, losses.size) - 0.5)
        nb, ghat = tpe.ctpe_counts(losses, G)
        plan.ctpe_fit(G, nb, ghat)
        n_live = len(plan.ctpe_info()[0])
        for kind, sizes in (('fit + score', (4096, 1 << 18)), ('draw + top 64', (4096, 1 << 16))):
            for m in sizes:
                dv = torch.from_numpy(pool_columns(dom, m)).cuda()
                dt = torch.empty(m, dtype=torch.float64).cuda()
                di = torch.empty(64, dtype=torch.int32).cuda()

                def plain():
                    plan.fit(stream=s)
                    if kind == 'fit + score':
                        plan.score_points_device(dv.data_ptr(), m, m, dt.data_ptr(), stream=s)
                    else:
                        plan.sample_points_device(5, 0, m, m, dv.data_ptr(), dt.data_ptr(),
                                                  stream=s)
                        plan.topk_points(dt.data_ptr(), 64, m=m, out=di.data_ptr(), stream=s)

                def ctpe():
                    plan.ctpe_fit(G, nb, ghat, stream=s)
                    if kind == 'fit + score':
                        plan.ctpe_score_points_device(dv.data_ptr(), m, m, dt.data_ptr(), stream=s)
                    else:
                        plan.ctpe_sample_points_device(5, 0, m, m, dv.data_ptr(), dt.data_ptr(),
                                                       stream=s)
                        plan.topk_points(dt.data_ptr(), 64, m=m, out=di.data_ptr(), stream=s)

                a, b = [], []
                for r in range(args.reps + 3):
                    x, y = timed(plain), timed(ctpe)
                    if r >= 3:
                        a.append(x)
                        b.append(y)
                pa, pb = float(np.median(a)), float(np.median(b))
                say('C=%-2d n_live=%-2d %-13s m=%-6d plain %8.3f ms (p90 %.3f)  c-TPE %8.3f ms '
                    '(p90 %.3f)  ratio %.2f' % (C, n_live, kind, m, pa, np.percentile(a, 90), pb,
                                                 np.percentile(b, 90), pb / pa))


if __name__ == '__main__':
    main()
