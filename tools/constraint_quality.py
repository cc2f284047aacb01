"""What constrained TPE finds, against a penalty and against
random search: 200 evaluations, mean and range over 5 seeds.

  disc   minimise x + y on [-2, 2]^2 subject to x^2 + y^2 - 1 <= 0 and
         x - y - 1 <= 0: the unconstrained optimum (-2, -2) is infeasible, the
         constrained one is -sqrt(2) on the rim of the unit disc, a fifth of
         the box is feasible.  Figure: the best feasible loss (lower is
         better).
  binh   Binh-Korn: minimise (4 x^2 + 4 y^2, (x - 5)^2 + (y - 5)^2) on
         [0, 5] x [0, 3] subject to (x - 5)^2 + y^2 - 25 <= 0 and
         7.7 - (x - 8)^2 - (y + 3)^2 <= 0.  Figure: the hypervolume of the
         feasible trials against (140, 50) (higher is better).
  spot   minimise x + y on [-2, 2]^2 subject to |x - 1| - 0.1 <= 0 and
         |y - 1| - 0.1 <= 0: 0.25 % of the box is feasible and the loss pulls
         away from it, so feasible trials stay rarer than the good side of the
         split for a long time.  Figure: the feasible trials among the
         evaluations (higher is better).

Methods: ``tpe.suggest(constraints=2)``; ``tpe.suggest`` on the loss (every
objective) plus a fixed penalty for an infeasible trial; ``rand.suggest``.
``--model ctpe`` adds c-TPE: ``tpe.suggest_joint(constraints=2,
constraint_model='ctpe')``, and beside it ``suggest_joint(constraints=2)`` -- the
ranking through the same whole-configuration draw -- and writes to
profiles/ctpe_quality.txt.
usage: python tools/constraint_quality.py [--evals 200] [--seeds 5] [--model ctpe] [--out FILE]
"""
import argparse
import functools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

REF = (140.0, 50.0)
PENALTY = {'disc': 10.0, 'binh': 200.0, 'spot': 10.0}
FIGURE = {'disc': 'best feasible loss', 'binh': 'feasible hypervolume', 'spot': 'feasible trials'}


def disc(c):
    x, y = c['x'], c['y']
    return [x + y], [x * x + y * y - 1.0, x - y - 1.0]


def spot(c):
    x, y = c['x'], c['y']
    return [x + y], [abs(x - 1.0) - 0.1, abs(y - 1.0) - 0.1]


def binh(c):
    x, y = c['x'], c['y']
    return ([4.0 * x * x + 4.0 * y * y, (x - 5.0) ** 2 + (y - 5.0) ** 2],
            [(x - 5.0) ** 2 + y * y - 25.0, 7.7 - (x - 8.0) ** 2 - (y + 3.0) ** 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--evals', type=int, default=200)
    ap.add_argument('--seeds', type=int, default=5)
    ap.add_argument('--model', choices=['rank', 'ctpe'], default='rank')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, 'profiles', 'ctpe_quality.txt' if args.model == 'ctpe'
                                else 'constraint_quality.txt')
    import numpy as np
    from hyperopt_amd import fmin, hp, rand, tpe, Trials
    import hv_oracle as HO
    out = open(args.out, 'w') if args.out else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + '\n')
            out.flush()

    problems = {
        'disc': (disc, lambda: {'x': hp.uniform('x', -2, 2), 'y': hp.uniform('y', -2, 2)}, 1),
        'spot': (spot, lambda: {'x': hp.uniform('x', -2, 2), 'y': hp.uniform('y', -2, 2)}, 1),
        'binh': (binh, lambda: {'x': hp.uniform('x', 0, 5), 'y': hp.uniform('y', 0, 3)}, 2),
    }

    def objective(f, penalty):
        def fn(c):
            y, g = f(c)
            bad = penalty if penalty and max(g) > 0 else 0.0
            y = [v + bad for v in y]
            return {'status': 'ok', 'loss': y[0], 'objectives': y, 'constraints': g,
                    'raw': f(c)[0]}
        return fn

    def figure(name, trials):
        ok = [d['result'] for d in trials.trials if max(d['result']['constraints']) <= 0]
        if name == 'disc':
            return min([r['raw'][0] for r in ok] or [float('inf')])
        return float(len(ok)) if name == 'spot' else HO.hv2d([r['raw'] for r in ok], REF)

    say('constrained TPE, %d evaluations, %d seeds: mean [min, max]' % (args.evals, args.seeds))
    for name, (f, space, M) in problems.items():
        obj = {} if M == 1 else {'objectives': M}
        methods = [('tpe constraints=2', functools.partial(tpe.suggest, constraints=2, **obj), 0.0),
                   ('tpe + penalty', functools.partial(tpe.suggest, **obj), PENALTY[name]),
                   ('rand', rand.suggest, 0.0)]
        if args.model == 'ctpe':
            methods[1:1] = [
                ('joint constraints=2', functools.partial(tpe.suggest_joint, constraints=2, **obj),
                 0.0),
                ('joint c-TPE', functools.partial(tpe.suggest_joint, constraints=2,
                                                  constraint_model='ctpe', **obj), 0.0)]
        for label, algo, penalty in methods:
            vals = []
            for seed in range(args.seeds):
                t = Trials()
                fmin(objective(f, penalty), space(), algo=algo, max_evals=args.evals, trials=t,
                     rstate=np.random.RandomState(100 + seed))
                vals.append(figure(name, t))
            say('%-5s %-19s %s %10.4f [%.4f, %.4f]'
                % (name, label, FIGURE[name], np.mean(vals), min(vals), max(vals)))


if __name__ == '__main__':
    main()
