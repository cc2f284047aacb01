"""bench.py's host-side pieces: the --dump-outputs files and the result line
of a plain run (no GPU, no engine call)."""
import argparse
import os

import numpy as np


def test_dump_outputs_files(tmp_path):
    import bench
    from hyperopt_amd._engine import RESULT_DTYPE
    res = np.zeros((2, 3), dtype=RESULT_DTYPE)
    res['score'] = [[0.5, np.nan, -1.0], [np.nan, 2.0, np.nan]]
    res['value'] = [[1.5, np.nan, 7.0], [np.nan, -2.0, np.nan]]
    res['index'] = [[4, -1, 9_999_999], [-1, 0, 3]]
    res['active'] = [[1, 0, 1], [0, 1, 1]]
    out = str(tmp_path / 'dump')
    bench.dump_outputs(out, res)
    assert sorted(os.listdir(out)) == ['active.npy', 'index.npy', 'score.npy', 'value.npy']
    got = {n: np.load(os.path.join(out, n + '.npy')) for n in ('score', 'value', 'index', 'active')}
    for a in got.values():
        assert a.dtype == np.float64 and a.shape == (2, 3)
    # inactive slots are written as 0; an active slot keeps its NaN
    np.testing.assert_array_equal(got['score'], [[0.5, 0.0, -1.0], [0.0, 2.0, np.nan]])
    np.testing.assert_array_equal(got['value'], [[1.5, 0.0, 7.0], [0.0, -2.0, np.nan]])
    np.testing.assert_array_equal(got['index'], res['index'])
    np.testing.assert_array_equal(got['active'], res['active'])


def test_plain_result_line():
    import bench
    args = argparse.Namespace(steps=4, warmup=2, prune=3)
    line = bench.report(args, bench.CONFIGS['cfg4'], None, 1, 'single', 0.5, 8e12, 1e12, 1e12, 1,
                        10_000_000, None, None)
    assert line['ms_per_step'] == 125.0 and line['steps'] == 4 and line['warmup'] == 2
    assert line['value'] == 8e12 and line['unit'] == 'pairs/s' and line['higher_is_better'] is True
    assert line['metric'] == 'EI candidates scored/sec (x components)'
    assert line['dtype'].startswith('f64') and line['full'] is False
    for k in ('roofline', 'e2e', 'cpu_baseline', 'evaluated_pairs_per_s'):
        assert k not in line
