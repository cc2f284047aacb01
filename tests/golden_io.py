"""Readers for the golden fixtures written by tests/golden/make_golden.py."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def load(name):
    """The arrays of fixture ``name`` (x.npz) and of its further parts
    x.part2.npz, x.part3.npz, ... (make_golden.py keeps every file under
    1 MiB by spreading a fixture's arrays over several)."""
    d = dict(np.load(os.path.join(GOLDEN, name), allow_pickle=False))
    stem = name[:-len('.npz')]
    k = 2
    while os.path.exists(os.path.join(GOLDEN, '%s.part%d.npz' % (stem, k))):
        part = np.load(os.path.join(GOLDEN, '%s.part%d.npz' % (stem, k)), allow_pickle=False)
        assert not set(part.files) & set(d), (name, k)
        d.update(part)
        k += 1
    return d


def load_json(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def unpack(d, key, i):
    off = d[key + '_off']
    return d[key][off[i]:off[i + 1]]


def ncases(d, key):
    return len(d[key + '_off']) - 1


def opt(v):
    v = float(v)
    return None if np.isnan(v) else v
