"""The 32-bit key window of k_fit's large-history sort and the adjacent-pair
check that proves a sort on it (hyperopt_amd/csrc/tpe_fit_window.hpp) are
plain C++: tests/host/fit_window_check.cpp runs the device's route -- window
keys, a stable counting pass per varying byte, short runs of equal window keys
ranked by their full keys, the check -- against std::stable_sort on (key,
position), for distinct keys, equal keys, massive ties, keys the window cannot
order, windows that hold every varying bit and an outlier that widens them,
at 4097, 4160, 9999 and 10000 elements.  Built host-only with the address and
undefined-behaviour sanitizers and run as a stand-alone program (no GPU)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


def test_fit_window_host_checks(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.fail('hipcc not found at %s' % HIPCC)
    exe = str(tmp_path / 'fit_window_check')
    src = os.path.join(ROOT, 'tests', 'host', 'fit_window_check.cpp')
    cc = subprocess.run(
        [HIPCC, '-x', 'hip', '--cuda-host-only', '-std=c++17', '-O1', '-g', '-Wall',
         '-Xarch_host', '-fsanitize=address,undefined',
         '-Xarch_host', '-fno-sanitize-recover=undefined', src, '-o', exe],
        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert cc.returncode == 0, cc.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       universal_newlines=True)
    assert r.returncode == 0, r.stdout
