"""Time a batch for parallel workers: the device calls of one
``suggest_joint(multivariate='groups')`` with ``batch='topk'`` against
``batch='pending'`` at the same shapes, in one session, alternating: device
time (HIP events on the call's stream, median and spread after warm-up) of
  topk     ``group_sample_points`` over M configurations + the top
           max(4k, 64) (tpe_plan_topk_points) + their gather -- the parent's
           call, the yardstick;
  pending  the same draw + k greedy rounds (tpe_plan_group_batch_points) + the
           gather of the k picks;
  greedy   the k rounds alone, and their time per round.
The events bracket the stream's work; the greedy call's 4-byte read-back
waits for it on the host but adds no device time.

Shapes: config 2's 20-hp space (one group) over 1000 trials and config 3's
50-hp conditional space (8 groups) over 1000 trials, each at 4096 and 2^16
configurations, k = 8 and 64.
usage: python tools/batch_time.py [--shapes cfg2:1000:4096 ...] [--k 8 64] [--reps N] [--out FILE]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from group_time import build  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', nargs='+',
                    default=['cfg2:1000:4096', 'cfg2:1000:65536', 'cfg3:1000:4096',
                             'cfg3:1000:65536'])
    ap.add_argument('--k', nargs='+', type=int, default=[8, 64])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'batch_time.txt'))
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
        # fit through the entry point, then time the plan's calls
        tpe.sample_configs(8, dom, t, 1, multivariate='groups')
        plan = dom._tpe_state.plan
        P = plan.n_hp
        dd = torch.empty((P, m), dtype=torch.float64).cuda()
        dt = torch.empty(m, dtype=torch.float64).cuda()
        di = torch.empty(tpe.TOPK_MAX, dtype=torch.int32).cuda()
        dc = torch.empty((P, tpe.TOPK_MAX), dtype=torch.float64).cuda()
        torch.cuda.synchronize()
        sp = stream.cuda_stream
        for k in args.k:
            kk = min(m, tpe.TOPK_MAX, max(4 * k, 64))

            def draw(r):
                plan.group_sample_points_device(11 + r, 0, m, m, dd.data_ptr(), dt.data_ptr(),
                                                stream=sp)

            def topk(r):
                draw(r)
                plan.topk_points(dt.data_ptr(), kk, m=m, out=di.data_ptr(), stream=sp)
                plan.gather_points(dd.data_ptr(), di.data_ptr(), k=kk, ld=m, out=dc.data_ptr(),
                                   stream=sp)

            def greedy():
                plan.group_batch_points_device(dd.data_ptr(), m, m, k, di.data_ptr(), stream=sp)

            def pending(r):
                draw(r)
                greedy()
                plan.gather_points(dd.data_ptr(), di.data_ptr(), k=k, ld=m, out=dc.data_ptr(),
                                   stream=sp)

            tt, tp, tg = [], [], []
            for r in range(args.reps + 3):
                order = (topk, pending) if r % 2 == 0 else (pending, topk)
                res = {f: timed(lambda: f(r)) for f in order}
                g = timed(greedy)       # (on the draw the pending call left)
                if r >= 3:
                    tt.append(res[topk])
                    tp.append(res[pending])
                    tg.append(g)
            # the timed greedy call picks what the host-mode call picks
            torch.cuda.synchronize()
            got = di.cpu().numpy()[:k]
            want = plan.group_batch_points(dd.cpu().numpy(), k)[0]
            assert np.array_equal(got, want)
            tag = '%s n=%d M=%d k=%d' % (cfg, n, m, k)
            say('%s  P=%d groups %d (device, %d reps)' % (tag, P, plan.group_info()[1], len(tt)))
            say('%s  topk    (draw + top %d + gather)  %s' % (tag, kk, stats(tt)))
            say('%s  pending (draw + %d rounds + gather) %s' % (tag, k, stats(tp)))
            say('%s  greedy  (%d rounds alone)          %s; per round %.4f ms'
                % (tag, k, stats(tg), np.median(tg) / k))


if __name__ == '__main__':
    main()
