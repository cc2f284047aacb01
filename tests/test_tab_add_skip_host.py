"""The scaled accumulator of the Chebyshev tables' certificate sums
(hyperopt_amd/csrc/tpe_tab_add.hpp, used by k_table_build and
k_table_build_lean) is plain C++: tests/host/tab_add_skip_check.cpp feeds
tab_add and tab_add_skip -- which leaves out the additions that change no bit --
the same sequences and compares (m, s) bit for bit after every term: random
terms, terms on either side of the -56 limit, a new maximum behind a run of
skipped terms, -inf first and throughout, a NaN in the middle, a single term
and none.  Built host-only with the address and undefined-behaviour sanitizers
and run as a stand-alone program (no GPU)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


def test_tab_add_skip_host_checks(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.fail('hipcc not found at %s' % HIPCC)
    exe = str(tmp_path / 'tab_add_skip_check')
    src = os.path.join(ROOT, 'tests', 'host', 'tab_add_skip_check.cpp')
    cc = subprocess.run(
        [HIPCC, '-x', 'hip', '--cuda-host-only', '-std=c++17', '-O1', '-g', '-Wall',
         '-Xarch_host', '-fsanitize=address,undefined',
         '-Xarch_host', '-fno-sanitize-recover=undefined', src, '-o', exe],
        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert cc.returncode == 0, cc.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       universal_newlines=True)
    assert r.returncode == 0, r.stdout
