"""Time the three models -- marginal (``multivariate=False``), the joint model
over the unconditional hps (``True``) and one joint model per group of hps
(``'groups'``) -- at the same shapes, in one session, alternating: device time
(HIP events on the call's stream, median and spread after warm-up) of
  score   one device-resident ``*_score_points`` call over M configurations;
  draw    one ``*_sample_points`` + top 64 (tpe_plan_topk_points) + gather
          (tpe_plan_gather_points) call sequence over M drawn configurations;
and, in a loop of their own, of the joint and the group fit.  The share of
k_group_score in the 'groups' score call comes from a kernel trace of this
script (``--only groups`` keeps the other two modes' kernels out of it).

Shapes: config 3's 50-hp conditional space (8 groups) over 1000 and 10^4
trials and config 2's 20-hp space (one group) over 1000 trials, each at 4096
and 2^16 configurations.  The pool is 4096 prior draws tiled to M.
usage: python tools/group_time.py [--shapes cfg3:1000:4096 ...] [--reps N] [--out FILE]
       [--only false|true|groups]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from points_time import pool_columns  # noqa: E402

MODES = (False, True, 'groups')
TOP = 64


def build(cfg, n):
    import numpy as np
    import spaces
    from hyperopt_amd import hp, rand, Trials
    from hyperopt_amd.base import Domain
    dom = Domain(lambda x: 0.0, (spaces.cfg3_space if cfg == 'cfg3' else spaces.cfg2_space)(hp))
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
    ap.add_argument('--shapes', nargs='+',
                    default=['cfg3:1000:4096', 'cfg3:1000:65536', 'cfg3:10000:4096',
                             'cfg3:10000:65536', 'cfg2:1000:4096', 'cfg2:1000:65536'])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--only', choices=['false', 'true', 'groups'], default=None)
    args = ap.parse_args()
    modes = MODES
    if args.only is not None:
        modes = ({'false': False, 'true': True}.get(args.only, 'groups'),)
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

    def stats(x):
        x = np.asarray(x)
        return '%.3f ms (min %.3f, max %.3f)' % (np.median(x), x.min(), x.max())

    built = {}
    for shape in args.shapes:
        cfg, n, m = shape.split(':')
        n, m = int(n), int(m)
        if (cfg, n) not in built:
            built[cfg, n] = build(cfg, n)
        dom, t = built[cfg, n]
        vals = pool_columns(dom, m)
        want = {mode: tpe.score_configs(vals, dom, t, multivariate=mode) for mode in modes}
        plan = dom._tpe_state.plan
        P = plan.n_hp
        # the three fits live side by side on the plan: refit them all once
        plan.fit()
        plan.joint_fit()
        plan.group_fit()
        dv = torch.from_numpy(vals).cuda()
        dd = torch.empty((P, m), dtype=torch.float64).cuda()
        dt = torch.empty(m, dtype=torch.float64).cuda()
        di = torch.empty(TOP, dtype=torch.int32).cuda()
        dc = torch.empty((P, TOP), dtype=torch.float64).cuda()
        torch.cuda.synchronize()
        sp = stream.cuda_stream
        score = {False: plan.score_points_device, True: plan.joint_score_points_device,
                 'groups': plan.group_score_points_device}
        sample = {False: plan.sample_points_device, True: plan.joint_sample_points_device,
                  'groups': plan.group_sample_points_device}

        def draw(mode, r):
            sample[mode](11 + r, 0, m, m, dd.data_ptr(), dt.data_ptr(), stream=sp)
            plan.topk_points(dt.data_ptr(), TOP, m=m, out=di.data_ptr(), stream=sp)
            plan.gather_points(dd.data_ptr(), di.data_ptr(), k=TOP, ld=m, out=dc.data_ptr(),
                               stream=sp)

        ts = {mode: [] for mode in modes}
        td = {mode: [] for mode in modes}
        for r in range(args.reps + 3):
            # alternating, and from another mode each round: the three share the
            # session's noise and no mode always runs behind the same neighbour
            for mode in modes[r % len(modes):] + modes[:r % len(modes)]:
                a = timed(lambda: score[mode](dv.data_ptr(), m, m, dt.data_ptr(), stream=sp))
                b = timed(lambda: draw(mode, r))
                if r >= 3:
                    ts[mode].append(a)
                    td[mode].append(b)
        for mode in modes:          # the timed calls compute what the entry point returns
            score[mode](dv.data_ptr(), m, m, dt.data_ptr(), stream=sp)
            torch.cuda.synchronize()
            assert np.array_equal(dt.cpu().numpy(), want[mode], equal_nan=True), mode
        # The fits in a loop of their own: a fit rewrites its scoring tables, and
        # the first score after it reads them cold (0.4 ms on config 2 at M = 4096);
        # inside the loop above that would fall on whichever mode was refitted.
        jfit, gfit = [], []
        for r in range(args.reps + 3):
            plan.fit(stream=sp)
            j = timed(lambda: plan.joint_fit(stream=sp))
            g = timed(lambda: plan.group_fit(stream=sp))
            if r >= 3:
                jfit.append(j)
                gfit.append(g)
        tag = '%s n=%d M=%d' % (cfg, n, m)
        say('%s  P=%d groups %d; joint_fit %s, group_fit %s (device, %d reps)'
            % (tag, P, plan.group_info()[1], stats(jfit), stats(gfit), len(gfit)))
        for mode in modes:
            say('%s  multivariate=%-8r score %s; sample + top %d + gather %s'
                % (tag, mode, stats(ts[mode]), TOP, stats(td[mode])))


if __name__ == '__main__':
    main()
