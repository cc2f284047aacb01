"""Device time of the importance pass beside the float64 numpy
oracle on the same fit, in one session.

Config 2's space (20 hps) with 10^3 and 10^4 trials and the 100-hp space of
config 4 with 10^4 trials; n_live = 1 (a plain fit) and 5 (c-TPE with four
constraints, each feasible in about half of the rows).  The device pass is
tpe_plan_importance into device memory (k_importance + k_importance_sum), HIP
events on the call's stream, median of --reps after 3 warm-up calls.  The
oracle (tests/importance_oracle.py on the plan's own mixtures) is timed once
over --oracle-hps hps of model 0, spread evenly over the labels, and scaled to
P x n_live: the only comparison there is, and no target.
usage: python tools/importance_time.py [--reps 20] [--nodes 1024]
                                       [--out profiles/importance_time.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def history(space_fn, n):
    import numpy as np
    from hyperopt_amd import hp, rand, tpe, Trials
    from hyperopt_amd.base import Domain
    dom = Domain(lambda x: 0.0, space_fn(hp))
    t = Trials()
    docs = rand.suggest(list(range(n)), dom, t, 1)
    for d, l in zip(docs, np.random.RandomState(2).rand(n)):
        d['state'] = 2
        d['result'] = {'status': 'ok', 'loss': float(l)}
    t._insert_trial_docs(docs)
    t.refresh()
    return (dom,) + tuple(tpe.build_history(dom, t)[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--nodes', type=int, default=1024)
    ap.add_argument('--oracle-hps', type=int, default=4)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'importance_time.txt'))
    args = ap.parse_args()
    import numpy as np
    from hyperopt_amd import _engine as E
    E.load_library()                 # (before torch: one HIP runtime, _share_hip_runtime)
    import torch
    import importance_oracle as IO
    import spaces
    from hyperopt_amd import tpe
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

    G = args.nodes
    say('importance pass, %d nodes: device time, median of %d after 3 warm-up calls; the numpy '
        'oracle over %d hps of model 0, scaled to P x n_live' % (G, args.reps, args.oracle_hps))
    for name, fn, n in (('config 2', spaces.cfg2_space, 1000), ('config 2', spaces.cfg2_space, 10000),
                        ('100-hp', spaces.cfg4_space, 10000)):
        dom, losses, hv, ha = history(fn, n)
        cs = dom.space
        hps, conds, pprior = cs.engine_tables()
        plan = E.Plan(E.default_engine(), hps, conds, pprior, max_trials=n)
        plan.set_history(losses, hv, ha)
        P = plan.n_hp
        for C in (0, 4):
            if C:
                Gm = np.ascontiguousarray(np.random.RandomState(C).rand(C, n) - 0.5)
                nb, ghat = tpe.ctpe_counts(losses, Gm)
                plan.ctpe_fit(Gm, nb, ghat)
            else:
                plan.fit()
                ghat = np.array([min(25, int(np.ceil(0.25 * np.sqrt(n)))) / float(n)])
            n_live = ghat.size
            d = torch.empty((3, n_live, P), dtype=torch.float64).cuda()
            ptr = [d[j].data_ptr() for j in range(3)]
            ms = [timed(lambda: plan.importance_device(G, ghat, *ptr, stream=s))
                  for _ in range(args.reps + 3)][3:]
            pick = np.unique(np.linspace(0, P - 1, min(args.oracle_hps, P)).astype(int))
            k = pick.size
            t0 = time.perf_counter()
            want = []
            for i in pick:
                h = cs.by_label[cs.labels[i]]
                mix = [plan.mixture(i, side) for side in (0, 1)]
                if h.dist in ('randint', 'categorical'):
                    mix = [m[0] for m in mix]
                want.append(IO.importance(h.dist, h.args, mix[0], mix[1], ghat[0], G)['D'])
            t_or = (time.perf_counter() - t0) / k
            got = d[0, 0].cpu().numpy()[pick]
            terms = G * P * n_live * (n + 2)
            say('%-8s P=%-3d n=%-5d n_live=%d  device %8.3f ms (p90 %.3f; %.3g terms, %.3g per s)  '
                'oracle %.3f s per (model, hp) -> %.1f s; max |D - oracle| %.2g'
                % (name, P, n, n_live, np.median(ms), np.percentile(ms, 90), terms,
                   terms / (np.median(ms) * 1e-3), t_or, t_or * P * n_live,
                   np.abs(got - np.array(want)).max()))


if __name__ == '__main__':
    main()
