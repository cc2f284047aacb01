"""Device time of the pairwise importance pass beside the float64
numpy oracle on the same fit, in one session.

Config 2's space (20 hps, 190 pairs) and the 100-hp space of config 4 (4950
pairs) with 10^3 and 10^4 trials, 64 and 128 nodes per dim, all pairs.  The
device pass is tpe_plan_group_importance_pairs into device memory (the table
upload and five launches), HIP events on the call's stream, median of --reps
after 3 warm-up calls.  The FMA count is k_pair_gemm's alone, pairs x G^2 x
(K_below + K_above), and the rate divides it by the whole call's time: a lower
bound on the kernel's own.  The oracle (tests/pair_importance_oracle.py on the
plan's own components) is timed over --oracle-pairs pairs and scaled to all:
the only comparison there is, and no target.  A case whose workspace is past
the engine's cap is reported as refused.
usage: python tools/pair_importance_time.py [--reps 10]
                                [--out profiles/pair_importance_time.txt]
"""
import argparse
import itertools
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--oracle-pairs', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pair_importance_time.txt'))
    args = ap.parse_args()
    import numpy as np
    from hyperopt_amd import _engine as E
    E.load_library()                 # (before torch: one HIP runtime, _share_hip_runtime)
    import torch
    import pair_importance_oracle as PO
    import spaces
    from importance_time import history
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    out = open(args.out, 'w') if args.out else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + '\n')
            out.flush()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    say('pairwise importance pass, all pairs: device time of the call, median of %d after 3 '
        'warm-up calls; the numpy oracle over %d pairs, scaled to all' % (args.reps,
                                                                          args.oracle_pairs))
    for name, fn, n in (('config 2', spaces.cfg2_space, 1000), ('config 2', spaces.cfg2_space, 10000),
                        ('100-hp', spaces.cfg4_space, 1000), ('100-hp', spaces.cfg4_space, 10000)):
        dom, losses, hv, ha = history(fn, n)
        cs = dom.space
        hps, conds, pprior = cs.engine_tables()
        plan = E.Plan(E.default_engine(), hps, conds, pprior, max_trials=n)
        plan.set_history(losses, hv, ha)
        plan.fit()
        plan.group_fit()
        P = plan.n_hp
        pairs = list(itertools.combinations(range(P), 2))       # (one group: no conditions)
        ghat = min(25, int(np.ceil(0.25 * np.sqrt(n)))) / float(n)
        w = [plan.group_mixture(0, -1, side)[0] for side in (0, 1)]
        for G in (64, 128):
            head = '%-8s P=%-3d n=%-5d G=%-3d pairs=%-4d' % (name, P, n, G, len(pairs))
            d = torch.empty((3, len(pairs)), dtype=torch.float64).cuda()
            ptr = [d[j].data_ptr() for j in range(3)]
            try:
                ms = [timed(lambda: plan.importance_pairs_device(G, ghat, pairs, *ptr, stream=s))
                      for _ in range(args.reps + 3)][3:]
            except ValueError as e:
                say('%s refused: %s' % (head, e))
                continue
            pick = np.unique(np.linspace(0, len(pairs) - 1, args.oracle_pairs).astype(int))
            t0 = time.perf_counter()
            want = []
            for j in pick:
                dims = [(cs.by_label[cs.labels[i]].dist, cs.by_label[cs.labels[i]].args,
                         [plan.group_mixture(0, i, side)[1:3] for side in (0, 1)])
                        for i in pairs[j]]
                _, wa, _, wb, L = PO.planes(dims[0], dims[1], w, G)
                want.append(PO.integrate(L, wa, wb, ghat)['D'])
            t_or = (time.perf_counter() - t0) / pick.size
            got = d[0].cpu().numpy()[pick]
            fma = float(len(pairs)) * G * G * (w[0].size + w[1].size)
            say('%s device %9.3f ms (p90 %.3f; %.3g gemm FMAs, >= %.3g per s)  oracle %.3f s per '
                'pair -> %.1f s; max |D - oracle| / D %.2g'
                % (head, np.median(ms), np.percentile(ms, 90), fma, fma / (np.median(ms) * 1e-3),
                   t_or, t_or * len(pairs), (np.abs(got - np.array(want)) / np.array(want)).max()))


if __name__ == '__main__':
    main()
