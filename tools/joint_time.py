"""Time the multivariate (joint) model next to the marginal one at the same
shapes, in one session: device time of tpe_plan_joint_fit, of
tpe_plan_joint_score_points against tpe_plan_score_points (device buffers,
HIP events on the call's stream, alternating, median after warm-up), and the
wall time of tpe.suggest_joint with and without ``multivariate=True``.

Shapes: config 2's 20-hp space over 1000 trials at 4096, 2^16 and 2^18
configurations; config 3's 50-hp conditional space (one unconditional hp) at
2^16; 100 uniform hps over 10^4 trials at 2^14.  The pool is 4096 prior draws
tiled to M.  `pairs` counts (configuration, component, root hp) triples of the
joint score, which are the marginal score's (configuration, component) pairs
of the same hps.
usage: python tools/joint_time.py [--shapes cfg2:4096 ...] [--reps N] [--out FILE]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from anneal_time import build  # noqa: E402  (config 2 / 3 domains and histories)
from points_time import pool_columns  # noqa: E402


def build_u100(n=10000):
    import numpy as np
    import spaces
    from hyperopt_amd import hp, rand, Trials
    from hyperopt_amd.base import Domain
    dom = Domain(lambda x: 0.0, spaces.cfg4_space(hp, 100))
    t = Trials()
    docs = rand.suggest(list(range(n)), dom, t, 1)
    for d, l in zip(docs, np.random.RandomState(2).rand(n)):
        d['state'] = 2
        d['result'] = {'status': 'ok', 'loss': float(l)}
    t._insert_trial_docs(docs)
    t.refresh()
    return dom, t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', nargs='+', default=['cfg2:4096', 'cfg2:65536', 'cfg2:262144',
                                                    'cfg3:65536', 'u100:16384'])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=None)
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

    built = {}
    for shape in args.shapes:
        cfg, m = shape.split(':')
        m = int(m)
        if cfg not in built:
            built[cfg] = build_u100() if cfg == 'u100' else build(cfg)
        dom, t = built[cfg]
        cs = dom.space
        vals = pool_columns(dom, m)
        total_j = tpe.score_configs(vals, dom, t, multivariate=True)   # plan, fit, joint fit
        plan = dom._tpe_state.plan
        roots = tpe.root_indices(cs)
        dv = torch.from_numpy(vals).cuda()
        dt = torch.empty(m, dtype=torch.float64).cuda()
        torch.cuda.synchronize()
        sp = stream.cuda_stream
        fit, jfit, js, ms = [], [], [], []
        for r in range(args.reps + 3):
            f = timed(lambda: plan.fit(stream=sp))
            jf = timed(lambda: plan.joint_fit(stream=sp))
            j = timed(lambda: plan.joint_score_points_device(dv.data_ptr(), m, m, dt.data_ptr(),
                                                             stream=sp))
            s = timed(lambda: plan.score_points_device(dv.data_ptr(), m, m, dt.data_ptr(),
                                                       stream=sp))
            if r >= 3:
                fit.append(f), jfit.append(jf), js.append(j), ms.append(s)
        plan.joint_score_points_device(dv.data_ptr(), m, m, dt.data_ptr(), stream=sp)
        torch.cuda.synchronize()
        assert np.array_equal(dt.cpu().numpy(), total_j, equal_nan=True)
        kb, ka = (plan.joint_mixture(-1, s)[0].size for s in (0, 1))
        triples = float(m) * (kb + ka) * len(roots)
        med = lambda x: float(np.median(x))  # noqa: E731
        tag = '%s M=%d' % (cfg, m)
        say('%s  n=%d P=%d root hps %d, K_below %d K_above %d' % (tag, plan.n, plan.n_hp,
                                                                  len(roots), kb, ka))
        say('%s  fit %.3f ms, joint_fit %.3f ms (device, median of %d)' % (tag, med(fit), med(jfit),
                                                                          len(fit)))
        say('%s  joint_score_points %.3f ms, score_points %.3f ms: ratio %.2f; %.3e root triples, '
            '%.3e /s' % (tag, med(js), med(ms), med(js) / med(ms), triples,
                         triples / (1e-3 * med(js))))
        wall = {}
        for mv in (False, True):
            lat = []
            for i in range(max(3, args.reps // 2)):
                t0 = time.perf_counter()
                tpe.suggest_joint([10 ** 6 + i], dom, t, 7 + i, n_configs=m, n_startup_jobs=0,
                                  multivariate=mv)
                lat.append(time.perf_counter() - t0)
            wall[mv] = 1e3 * med(lat)
        say('%s  suggest_joint wall %.2f ms, multivariate %.2f ms (sync + fit + draw + score + '
            'top-k, median)' % (tag, wall[False], wall[True]))


if __name__ == '__main__':
    main()
