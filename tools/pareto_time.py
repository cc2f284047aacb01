"""Time the Pareto ranking pass of multi-objective TPE: device
time (HIP events on the call's stream, median and spread after warm-up) of
  pareto  one ``tpe_plan_set_objectives`` call with the objective matrix
          already on the device (obj0 = n: no upload) -- the count memset,
          k_pareto_count and k_pareto_loss;
  fit     ``tpe_plan_fit`` on the same plan and history, in the same session,
          alternating with it;
and on the host
  numpy   the vectorised numpy oracle (tests/pareto_oracle.py's rule: one
          row against all rows per step).  At n > 2e4 it is timed on 1000 rows
          and scaled by n / 1000 (every row costs the same), marked ~.
at n = 1e3, 1e4, 1e5 trials and M = 2, 4, 8 objectives, on a space of 8
uniform hps.  The last column names the larger of pareto and fit.
usage: python tools/pareto_time.py [--n 1000 10000 100000] [--m 2 4 8] [--reps N] [--out FILE]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

N_HP = 8


def oracle_rows(Y, rows):
    """dominated_by of ``rows`` by pareto_oracle.pareto_counts_fast's step."""
    import numpy as np
    ok = ~(np.isnan(Y) | (Y == np.inf)).any(axis=0)
    by = np.zeros(len(rows), dtype=np.int32)
    for k, i in enumerate(rows):
        yi = Y[:, i:i + 1]
        by[k] = (ok & (Y <= yi).all(axis=0) & (Y < yi).any(axis=0)).sum()
    return by


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', nargs='+', type=int, default=[1000, 10000, 100000])
    ap.add_argument('--m', nargs='+', type=int, default=[2, 4, 8])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pareto_time.txt'))
    args = ap.parse_args()
    import numpy as np
    from hyperopt_amd import _engine as E
    E.load_library()                 # (before torch: one HIP runtime, _share_hip_runtime)
    import torch
    from hyperopt_amd import hp
    from hyperopt_amd.base import Domain
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
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

    def stats(x):
        x = np.asarray(x)
        return '%9.3f ms (min %.3f, max %.3f)' % (np.median(x), x.min(), x.max())

    dom = Domain(lambda x: 0.0, {'x%d' % i: hp.uniform('x%d' % i, 0, 1) for i in range(N_HP)})
    hps, conds, pprior = dom.space.engine_tables()
    eng = E.default_engine()
    say('Pareto ranking pass against the fit: %d uniform hps, device time per call' % N_HP)
    for n in args.n:
        rng = np.random.RandomState(n)
        plan = E.Plan(eng, hps, conds, pprior, max_trials=n)
        plan.set_history(rng.rand(n), rng.rand(N_HP, n), np.ones((N_HP, n), dtype=np.uint8))
        for M in args.m:
            Y = np.round(rng.rand(M, n), 3)          # (ties among the coordinates)
            plan.set_objectives(Y)                   # upload + first ranking
            dy = torch.from_numpy(Y).cuda()
            torch.cuda.synchronize()
            _, _, splits, tiles = plan.pareto_shape(n, M)

            def pareto():
                plan.set_objectives_device(dy.data_ptr(), M, n, n, obj0=n, stream=sp)

            def fit():
                plan.fit(stream=sp)

            tp, tf = [], []
            for r in range(args.reps + 3):
                order = (pareto, fit) if r % 2 == 0 else (fit, pareto)
                res = {f: timed(f) for f in order}
                if r >= 3:
                    tp.append(res[pareto])
                    tf.append(res[fit])
            torch.cuda.synchronize()
            by = plan.pareto_get(n)[0]
            rows = np.arange(n) if n <= 20000 else rng.choice(n, 1000, replace=False)
            t0 = time.perf_counter()
            want = oracle_rows(Y, rows)
            host = (time.perf_counter() - t0) * (n / float(len(rows)))
            assert np.array_equal(by[rows], want)
            mp, mf = np.median(tp), np.median(tf)
            tag = 'n=%-6d M=%d' % (n, M)
            say('%s  grid %d x %d blocks, %d reps' % (tag, tiles, splits, len(tp)))
            say('%s  pareto %s' % (tag, stats(tp)))
            say('%s  fit    %s' % (tag, stats(tf)))
            say('%s  numpy  %s%9.1f ms on the host' % (tag, ' ' if len(rows) == n else '~', host * 1e3))
            say('%s  larger: %s (pareto / fit = %.2f)' % (tag, 'pareto' if mp > mf else 'fit',
                                                          mp / mf))
        plan.close()


if __name__ == '__main__':
    main()
