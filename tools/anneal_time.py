"""Time anneal.suggest on config 2's and config 3's spaces and histories.

Per config, one line each:
  device     one tpe_plan_anneal call at S = 1 and S = 1024 (HIP events on the
             call's stream around the call: loss order + k_anneal + the copy
             of the records to the host), median of --reps calls after warm-up
  suggest    wall time of anneal.suggest end to end (a real Trials, one new
             finished trial between calls: history sync + row upload + the
             engine call + the document), and of tpe.suggest (defaults) on the
             same history for comparison
  host       wall time of anneal.suggest(rng_stream='numpy') for one
             suggestion on the same history (the reference's algorithm as the
             host states it: columns rebuilt, argsort, numpy samplers)
usage: python tools/anneal_time.py [--configs cfg2 cfg3] [--reps N]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def build(cfg):
    import numpy as np
    import big_configs
    import spaces
    from hyperopt_amd import hp, rand, Trials
    from hyperopt_amd.base import Domain
    if cfg == 'cfg3':
        return big_configs.cfg3_trials(hp, Domain, Trials, rand)
    dom = Domain(lambda x: 0.0, spaces.cfg2_space(hp))
    t = Trials()
    docs = rand.suggest(list(range(1000)), dom, t, 1)
    for d, l in zip(docs, np.random.RandomState(2).rand(1000)):
        d['state'] = 2
        d['result'] = {'status': 'ok', 'loss': float(l)}
    t._insert_trial_docs(docs)
    t.refresh()
    return dom, t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', nargs='+', default=['cfg2', 'cfg3'])
    ap.add_argument('--reps', type=int, default=50)
    args = ap.parse_args()
    import numpy as np
    from hyperopt_amd import _engine as E
    E.load_library()                 # (before torch: one HIP runtime, _share_hip_runtime)
    import torch
    from hyperopt_amd import anneal, tpe
    stream = torch.cuda.Stream()
    for cfg in args.configs:
        dom, t = build(cfg)
        n0 = len(t.trials)
        anneal.suggest(t.new_trial_ids(1), dom, t, 1)          # builds plan + mirror
        plan = dom._tpe_state.plan
        for S in (1, 1024):
            seeds = tpe.batch_seeds(7, S)
            ms = []
            for r in range(args.reps + 5):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                plan.anneal(seeds, 2.0, 0.1, stream=stream.cuda_stream)
                b.record(stream)
                b.synchronize()
                if r >= 5:
                    ms.append(a.elapsed_time(b))
            print('%s device  S=%-4d anneal call %.1f us median (p90 %.1f us), n=%d P=%d'
                  % (cfg, S, 1e3 * np.median(ms), 1e3 * np.percentile(ms, 90), n0, plan.n_hp))
        rng = np.random.RandomState(5)
        wall = {}
        for name, fn in (('anneal.suggest', anneal.suggest), ('tpe.suggest', tpe.suggest)):
            fn(t.new_trial_ids(1), dom, t, 2)                   # warm (tpe: first fit)
            lat = []
            for i in range(args.reps):
                ids = t.new_trial_ids(1)
                t0 = time.perf_counter()
                docs = fn(ids, dom, t, 100 + i)
                lat.append(time.perf_counter() - t0)
                t.insert_trial_docs(docs)
                t.refresh()
                t.trials[-1]['result'] = {'status': 'ok', 'loss': float(rng.rand())}
                t.trials[-1]['state'] = 2
            wall[name] = 1e3 * np.median(lat)
        print('%s suggest anneal.suggest %.3f ms, tpe.suggest %.3f ms (wall, median of %d, one new '
              'trial between calls)' % (cfg, wall['anneal.suggest'], wall['tpe.suggest'], args.reps))
        lat = []
        for i in range(max(3, args.reps // 10)):
            t0 = time.perf_counter()
            anneal.suggest(t.new_trial_ids(1), dom, t, 200 + i, rng_stream='numpy')
            lat.append(time.perf_counter() - t0)
        print("%s host    anneal.suggest(rng_stream='numpy') %.2f ms (wall, median of %d)"
              % (cfg, 1e3 * np.median(lat), len(lat)))


if __name__ == '__main__':
    main()
