"""What ``objectives=2`` buys on two-objective problems: the dominated
hypervolume of the final front of
  mo-tpe   ``tpe.suggest(objectives=2)`` (the history ranked by Pareto dominance),
  sum-tpe  ``tpe.suggest`` on the sum of the two objectives,
  random   ``rand.suggest``,
over 5 seeds and 200 evaluations each, against the reference point (1.1, 1.1).

Problems (both with a concave front, so no weighted sum has an optimum
inside it):
  ff    Fonseca-Fleming in 3 dimensions, x in [-4, 4]^3:
        f1 = 1 - exp(-sum (x_i - 1/sqrt 3)^2), f2 = 1 - exp(-sum (x_i + 1/sqrt 3)^2);
        the front is the segment x_1 = x_2 = x_3 in [-1/sqrt 3, 1/sqrt 3].
  zdt2  ZDT2 in 4 dimensions, x in [0, 1]^4: f1 = x0, g = 1 + 3 (x1 + x2 + x3),
        f2 = g (1 - (f1 / g)^2); the front is g = 1, f2 = 1 - f1^2.  Here any
        point with x0 near 0 is nondominated however large its g, so the rank
        alone does not push g down: the case hypervolume-based selection
        inside the front (``--hv``) exists for.
The first problem's numbers are the README's.  Not a pass condition.

``--hv`` adds the two arms of the hypervolume subset selection inside the
front after the three above and writes to
profiles/pareto_hv_quality.txt instead:
  hv-auto  ``tpe.suggest(objectives=2, hypervolume=True)`` (the default
           reference point, from the history),
  hv-ref   ``tpe.suggest(objectives=2, hypervolume=(1.1, 1.1))``.
usage: python tools/pareto_quality.py [--hv] [--problems ff zdt2] [--seeds N] [--evals N]
                                      [--out FILE]
"""
import argparse
import functools
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REF = (1.1, 1.1)


def ff(x):
    a = 1.0 / math.sqrt(3.0)
    return (1.0 - math.exp(-sum((v - a) ** 2 for v in x)),
            1.0 - math.exp(-sum((v + a) ** 2 for v in x)))


def zdt2(x):
    f1 = x[0]
    g = 1.0 + 9.0 * sum(x[1:]) / (len(x) - 1)
    return f1, g * (1.0 - (f1 / g) ** 2)


def true_front(name, k=20001):
    if name == 'ff':
        a = 1.0 / math.sqrt(3.0)
        return [ff([a * (2.0 * i / (k - 1) - 1.0)] * 3) for i in range(k)]
    return [(i / (k - 1.0), 1.0 - (i / (k - 1.0)) ** 2) for i in range(k)]


# name: (function, dimensions, low, high)
PROBLEMS = {'ff': (ff, 3, -4.0, 4.0), 'zdt2': (zdt2, 4, 0.0, 1.0)}


def hypervolume(points, ref=REF):
    """Area dominated by 2-d ``points`` (minimised) inside the box below ``ref``."""
    pts = sorted((a, b) for a, b in points if a < ref[0] and b < ref[1])
    hv, best = 0.0, ref[1]
    for a, b in pts:
        if b < best:
            hv += (ref[0] - a) * (best - b)
            best = b
    return hv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--problems', nargs='+', default=['ff', 'zdt2'], choices=sorted(PROBLEMS))
    ap.add_argument('--seeds', type=int, default=5)
    ap.add_argument('--evals', type=int, default=200)
    ap.add_argument('--hv', action='store_true',
                    help='also the two hypervolume= arms; to profiles/pareto_hv_quality.txt')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, 'profiles',
                                'pareto_hv_quality.txt' if args.hv else 'pareto_quality.txt')
    import numpy as np
    from hyperopt_amd import fmin, hp, rand, tpe, Trials

    algos = [('mo-tpe', functools.partial(tpe.suggest, objectives=2)),
             ('sum-tpe', tpe.suggest),
             ('random', rand.suggest)]
    if args.hv:
        algos += [('hv-auto', functools.partial(tpe.suggest, objectives=2, hypervolume=True)),
                  ('hv-ref', functools.partial(tpe.suggest, objectives=2, hypervolume=REF))]
    out = open(args.out, 'w') if args.out else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + '\n')
            out.flush()

    say('dominated hypervolume of the final front against %r: %d evaluations, %d seeds'
        % (REF, args.evals, args.seeds))
    for name in args.problems:
        fn, dim, low, high = PROBLEMS[name]

        def objective(c):
            f1, f2 = fn([c['x%d' % i] for i in range(dim)])
            return {'status': 'ok', 'loss': f1 + f2, 'objectives': [f1, f2]}

        say('%s in %d dimensions (the true front: %.4f)'
            % (name, dim, hypervolume(true_front(name))))
        for label, algo in algos:
            hv = []
            for seed in range(args.seeds):
                t = Trials()
                space = {'x%d' % i: hp.uniform('x%d' % i, low, high) for i in range(dim)}
                fmin(objective, space, algo=algo, max_evals=args.evals, trials=t,
                     rstate=np.random.RandomState(seed))
                hv.append(hypervolume([d['result']['objectives'] for d in t.trials]))
            say('%-5s %-8s hypervolume mean %.4f  min %.4f  max %.4f  per seed %s'
                % (name, label, np.mean(hv), np.min(hv), np.max(hv),
                   ' '.join('%.4f' % v for v in hv)))


if __name__ == '__main__':
    main()
