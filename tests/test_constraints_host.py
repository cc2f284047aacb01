"""The numpy oracle against DESIGN 5.19's rule as a double loop; the launch plan."""
import os
import subprocess

import numpy as np
import pytest

import constraint_oracle as CO
import pareto_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
N = 48


def _cdom(Y, v, j, i):
    """Row j c-dominates row i (two complete rows): the rule as written."""
    return bool(v[j] < v[i] or (v[j] == 0 and v[i] == 0 and PO.dominates(Y[:, j], Y[:, i])))


@pytest.mark.parametrize('feasible', [None, True, False])
@pytest.mark.parametrize('M,C', [(1, 1), (2, 3), (3, 16)])
def test_oracle_is_the_rule(M, C, feasible):
    Y, G = CO.history(N, M, C, feasible)
    v, by, of, s = CO.constraint_rank(Y, G)
    ok = PO.complete_rows(Y)
    if feasible is None:                                # NaN, +inf, -inf, an overflowing sum
        assert np.isinf(v[[6, 7]]).all() and v[8] >= 0 and (C == 1 or np.isinf(v[N - 2]))
    bb, ff = np.zeros(N, np.int32), np.zeros(N, np.int32)
    for i in np.flatnonzero(ok):
        for j in np.flatnonzero(ok):
            if _cdom(Y, v, j, i):
                bb[i] += 1
                ff[j] += 1
                assert s[j] < s[i]                      # strictly increasing along c-dominance
    assert (bb == by).all() and (ff == of).all() and bb.sum() > 0
    assert np.isinf(s[~ok]).all() and (by[~ok] == 0).all() and (of[~ok] == 0).all()
    # the order: feasible, then infeasible by ascending violation, then pending
    order = np.argsort(s, kind='stable')
    cls = np.where(~ok, 2, np.where(v == 0, 0, 1))[order]
    assert (np.diff(cls) >= 0).all()
    vi = v[order][cls == 1]
    assert (vi[:-1] <= vi[1:]).all()
    if feasible is True:                                # the Pareto oracle exactly
        pb, pf, ps = PO.pareto_rank(Y)
        assert (v == 0).all() and (by == pb).all() and (of == pf).all()
        assert s.tobytes() == ps.tobytes()


def test_constraint_plan_host_checks(tmp_path):
    """tpe_pareto_plan.hpp with the violation row; a sanitized stand-alone program."""
    exe = str(tmp_path / 'constraint_plan_check')
    src = os.path.join(ROOT, 'tests', 'host', 'constraint_plan_check.cpp')
    cc = subprocess.run(
        [HIPCC, '-x', 'hip', '--cuda-host-only', '-std=c++17', '-O1', '-g', '-Wall',
         '-Xarch_host', '-fsanitize=address,undefined',
         '-Xarch_host', '-fno-sanitize-recover=undefined', src, '-o', exe],
        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert cc.returncode == 0, cc.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       universal_newlines=True)
    assert r.returncode == 0, r.stdout
