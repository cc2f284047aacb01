"""Mixture of suggest algorithms: each call is handed to one of several
suggest functions, drawn with given probabilities (semantics of
hyperopt/mix.py).

    fmin(..., algo=partial(mix.suggest, p_suggest=[
        (.1, rand.suggest), (.2, anneal.suggest), (.7, tpe.suggest)]))

The draw replays the reference's RandomState stream, so the same seed picks
the same algorithm and hands it the same sub-seed: one multinomial trial over
the probabilities, then one ``randint(2 ** 31)``.
"""
from __future__ import annotations

import numpy as np


def suggest(new_ids, domain, trials, seed, p_suggest):
    """``p_suggest``: (probability, suggest function) pairs.  The
    probabilities must add up to 1 (``np.isclose``), else ValueError."""
    weights = [float(w) for w, _ in p_suggest]
    algos = [fn for _, fn in p_suggest]
    if not np.isclose(sum(weights), 1.0):
        raise ValueError('mix.suggest: the probabilities of p_suggest add up to %r, not 1'
                         % sum(weights))
    stream = np.random.RandomState(seed)
    chosen = algos[int(np.argmax(stream.multinomial(1, weights)))]
    sub_seed = int(stream.randint(2 ** 31))
    return chosen(new_ids, domain, trials, seed=sub_seed)
