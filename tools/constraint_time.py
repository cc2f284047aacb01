"""Time the ranking pass of constrained TPE: device time (HIP
events on the call's stream, median and spread after warm-up) of one
``tpe_plan_set_objectives`` call with the matrices already on the device
(obj0 = n: no upload), with the constraint mode
  off   the count memset, k_pareto_count and k_pareto_loss;
  C=1   the memset, k_violation, k_cdom_count and k_pareto_loss;
  C=16  the same with 16 constraint rows;
at n = 1e3, 1e4, 1e5 trials and M = 1, 2, 8 objectives.  The three modes are
timed in blocks, twice round (off, 1, 16, off, 1, 16), in one session; the
ratio column is on / off, to hold against (M + 1) / M.
usage: python tools/constraint_time.py [--n ...] [--m ...] [--reps N] [--out FILE]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_HP = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', nargs='+', type=int, default=[1000, 10000, 100000])
    ap.add_argument('--m', nargs='+', type=int, default=[1, 2, 8])
    ap.add_argument('--reps', type=int, default=8)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'constraint_time.txt'))
    args = ap.parse_args()
    import numpy as np
    from hyperopt_amd import _engine as E
    E.load_library()                 # (before torch: one HIP runtime)
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
    say('ranking pass with the constraint mode off and on: device time per set_objectives call')
    for n in args.n:
        rng = np.random.RandomState(n)
        plan = E.Plan(eng, hps, conds, pprior, max_trials=n)
        plan.set_history(rng.rand(n), rng.rand(N_HP, n), np.ones((N_HP, n), dtype=np.uint8))
        G = np.round(rng.rand(16, n) - 0.7, 2)          # about a third of a row's entries violate
        for M in args.m:
            Y = np.round(rng.rand(M, n), 3)
            dy = torch.from_numpy(Y).cuda()
            torch.cuda.synchronize()
            t = {0: [], 1: [], 16: []}
            for rnd in range(2):
                for C in (0, 1, 16):
                    plan.set_constraints(np.ascontiguousarray(G[:C]) if C else None)
                    plan.set_objectives(Y)               # upload + first ranking in this mode
                    for r in range(args.reps + 2):
                        ms = timed(lambda: plan.set_objectives_device(dy.data_ptr(), M, n, n,
                                                                      obj0=n, stream=sp))
                        if r >= 2:
                            t[C].append(ms)
            torch.cuda.synchronize()
            plan.set_constraints(None)
            _, _, splits, tiles = plan.pareto_shape(n, M)
            tag = 'n=%-6d M=%d' % (n, M)
            say('%s  grid %d x %d blocks, %d samples per mode' % (tag, tiles, splits, len(t[0])))
            off = np.median(t[0])
            say('%s  off   %s' % (tag, stats(t[0])))
            for C in (1, 16):
                say('%s  C=%-2d  %s  on / off = %.2f  ((M + 1) / M = %.2f)'
                    % (tag, C, stats(t[C]), np.median(t[C]) / off, (M + 1.0) / M))
        plan.close()


if __name__ == '__main__':
    main()
