"""The fixtures of the greedy-batch tests, shared by the host test (which
proves every round of them decided under the oracle) and the GPU test (which
then asks the device for the oracle's picks) -- TEST INFRASTRUCTURE ONLY.

Histories: cfg2 (20 hps, 1000 rows) and cond (14 hps, 120 rows) from
tests/golden, and ``group_oracle.nested_space`` (9 hps, 80 rows).  The
configurations are prior draws of the space, built on the host so that both
tests hold the same ones."""
import functools

import numpy as np

import hyperopt_amd as H
from hyperopt_amd import hp, rand, tpe, Trials, trials_from_docs
from hyperopt_amd.base import Domain

from golden_io import load, load_json
from oracle_algo import oracle_hps
import batch_oracle as B
import group_oracle as G
import spaces

GAMMA, PRIOR_WEIGHT = 0.25, 1.0
GOLDEN = {'cfg2': spaces.cfg2_space, 'cond': spaces.cond_space}
NAMES = ('cfg2', 'cond', 'nested')
NESTED_SEED = 7
M, K = 257, 8
# the seed of each fixture's prior-drawn configurations: chosen so that every
# round is decided (test_batch_host.test_every_gpu_round_is_decided)
CONFIG_SEED = {'cfg2': 11, 'cond': 12, 'nested': 13}
# (m, k) of the launch-shape cases, on the first m configurations of `cond`
SHAPES = ((1, 1), (8, 8), (63, 8), (64, 8), (65, 8), (257, 8))


def done(docs, losses):
    for d, l in zip(docs, losses):
        d['state'] = H.JOB_STATE_DONE
        d['result'] = {'status': 'ok', 'loss': float(l)}
    return trials_from_docs(docs)


@functools.lru_cache(maxsize=None)
def history(name):
    """(domain, losses, vals, active) of a named history."""
    if name in GOLDEN:
        meta = load_json('suggest_meta.json')[name]
        d = load('suggest_%s.npz' % name)
        dom = Domain(lambda x: 0.0, GOLDEN[name](hp))
        assert list(meta['labels']) == dom.space.labels
        out = dom, d['losses'], d['vals'], d['active']
    else:
        dom = Domain(lambda x: 0.0, G.nested_space(hp))
        docs = rand.suggest(list(range(80)), dom, Trials(), NESTED_SEED)
        trials = done(docs, np.random.RandomState(NESTED_SEED + 100).rand(80))
        _, losses, vals, active = tpe.build_history(dom, trials)
        out = dom, losses, vals, active
    for a in out[1:]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def model(name):
    dom, losses, vals, active = history(name)
    h = oracle_hps(dom.space)
    return G.GroupModel([(lab, h[lab]) for lab in dom.space.labels], losses, vals, active,
                        GAMMA, PRIOR_WEIGHT)


@functools.lru_cache(maxsize=None)
def configs(name, seed=None, m=M):
    """vals[P, m]: prior draws of the fixture's space, NaN where inactive."""
    dom = history(name)[0]
    docs = rand.suggest(list(range(m)), dom, Trials(), CONFIG_SEED[name] if seed is None else seed)
    cfgs = [{lab: v[0] for lab, v in d['misc']['vals'].items() if v} for d in docs]
    vals = tpe.config_columns(dom.space, cfgs)[0]
    vals.setflags(write=False)
    return vals


@functools.lru_cache(maxsize=None)
def oracle_run(name, m=M, k=K):
    """The oracle's batch over the fixture's first m configurations."""
    return B.run(model(name), np.ascontiguousarray(configs(name)[:, :m]), k,
                 prior_weight=PRIOR_WEIGHT)
