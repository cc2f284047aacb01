"""Time the hypervolume subset selection inside the Pareto front:
device time (HIP events on the call's stream, median and spread after warm-up)
of one ``tpe_plan_set_objectives`` call with the objective matrix already on
the device (obj0 = n: no upload), in one session and alternating,
  off     the mode off: the count memset, k_pareto_count and k_pareto_loss;
  on      the mode on, n_pick = 32 rounds, S = 1024 samples: the same counts,
          then k_hv_init, the rounds (k_hv_round + k_hv_pick) and k_hv_loss;
  on/1    the mode on with n_pick = 1 (no k_hv_round): (on - on/1) / 31 is
          the cost of one further round;
  fit     ``tpe_plan_fit`` on the same plan and history, the yardstick;
at n = 1e3, 1e4, 1e5 trials and M = 2 (the exact path), 4, 8 (Monte-Carlo)
objectives, on a space of 8 uniform hps.  The objectives are a trade-off (a
front of many rows); the line ``front`` gives its size and the picks made.
usage: python tools/pareto_hv_time.py [--n 1000 10000 100000] [--m 2 4 8] [--reps N] [--out FILE]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_HP = 8
N_PICK, N_SAMPLES = 32, 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', nargs='+', type=int, default=[1000, 10000, 100000])
    ap.add_argument('--m', nargs='+', type=int, default=[2, 4, 8])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pareto_hv_time.txt'))
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
    say('hypervolume subset selection inside the front: %d uniform hps, n_pick = %d, S = %d, '
        'device time per tpe_plan_set_objectives' % (N_HP, N_PICK, N_SAMPLES))
    for n in args.n:
        rng = np.random.RandomState(n)
        plan = E.Plan(eng, hps, conds, pprior, max_trials=n)
        plan.set_history(rng.rand(n), rng.rand(N_HP, n), np.ones((N_HP, n), dtype=np.uint8))
        for M in args.m:
            # a trade-off: objective 0 against the rest, so the front holds many rows
            Y = rng.rand(M, n)
            Y[1:] = 1.0 - Y[0] + 0.4 * Y[1:]
            Y = np.round(Y, 3)
            ref = [float(v) for v in Y.max(axis=1) + 0.1]
            plan.set_hv(None)
            plan.set_objectives(Y)                   # upload + first ranking
            dy = torch.from_numpy(Y).cuda()
            torch.cuda.synchronize()

            def rank():
                plan.set_objectives_device(dy.data_ptr(), M, n, n, obj0=n, stream=sp)

            def off():
                plan.set_hv(None)
                rank()

            def on():
                plan.set_hv(ref, n_pick=N_PICK, n_samples=N_SAMPLES)
                rank()

            def on1():
                plan.set_hv(ref, n_pick=1, n_samples=N_SAMPLES)
                rank()

            def fit():
                plan.fit(stream=sp)

            fns = [off, on, on1, fit]
            times = {f: [] for f in fns}
            for r in range(args.reps + 3):
                order = fns[r % 4:] + fns[:r % 4]
                for f in order:
                    t = timed(f)
                    if r >= 3:
                        times[f].append(t)
            on()
            torch.cuda.synchronize()
            by = plan.pareto_get(n)[0]
            picks, _, counts, R = plan.hv_get()
            plan.set_hv(None)
            tag = 'n=%-6d M=%d' % (n, M)
            m_off, m_on, m_on1, m_fit = (np.median(times[f]) for f in fns)
            say('%s  front %d rows, %d picks, %s, %d reps'
                % (tag, int((by == 0).sum()), R, 'exact' if M == 2 else 'Monte-Carlo',
                   len(times[on])))
            say('%s  off    %s' % (tag, stats(times[off])))
            say('%s  on     %s' % (tag, stats(times[on])))
            say('%s  on/1   %s' % (tag, stats(times[on1])))
            say('%s  fit    %s' % (tag, stats(times[fit])))
            say('%s  selection %.3f ms = on - off; one further round %.4f ms; on / off = %.2f; '
                'selection / fit = %.2f'
                % (tag, m_on - m_off, (m_on - m_on1) / (N_PICK - 1), m_on / m_off,
                   (m_on - m_off) / m_fit))
        plan.close()


if __name__ == '__main__':
    main()
