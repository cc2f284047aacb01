"""The pooled rows of k_draw_sorted_screen_run (hyperopt_amd/csrc/
tpe_screen_pool.hpp) take a sort block's eight lists as one sequence
in rows of 64: tests/host/screen_pool_check.cpp checks the owner of every
pooled index -- empty lists, one wave holding everything, totals of 0, 1, 63,
64, 65 and 8 x 640 -- against the sequence written out.  Built host-only with
the address and undefined-behaviour sanitizers and run as a stand-alone program
(no GPU)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


def test_screen_pool_host_checks(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.fail('hipcc not found at %s' % HIPCC)
    exe = str(tmp_path / 'screen_pool_check')
    src = os.path.join(ROOT, 'tests', 'host', 'screen_pool_check.cpp')
    cc = subprocess.run(
        [HIPCC, '-x', 'hip', '--cuda-host-only', '-std=c++17', '-O1', '-g', '-Wall',
         '-Xarch_host', '-fsanitize=address,undefined',
         '-Xarch_host', '-fno-sanitize-recover=undefined', src, '-o', exe],
        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert cc.returncode == 0, cc.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       universal_newlines=True)
    assert r.returncode == 0, r.stdout
