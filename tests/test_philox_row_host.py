"""The row form of Philox4x32-10 and the word form of the 53-bit uniforms
(hyperopt_amd/csrc/tpe_philox_row.hpp, used by k_draw_sorted_screen_run) are
plain C++: tests/host/philox_row_check.cpp checks the row form against the
general one in all four words and all 64 lanes -- on either side of a low word
that wraps -- and the word-form compare and decode against the integers.  Built
host-only with the address and undefined-behaviour sanitizers and run as a
stand-alone program (no GPU)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


def test_philox_row_host_checks(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.fail('hipcc not found at %s' % HIPCC)
    exe = str(tmp_path / 'philox_row_check')
    src = os.path.join(ROOT, 'tests', 'host', 'philox_row_check.cpp')
    cc = subprocess.run(
        [HIPCC, '-x', 'hip', '--cuda-host-only', '-std=c++17', '-O1', '-g', '-Wall',
         '-Xarch_host', '-fsanitize=address,undefined',
         '-Xarch_host', '-fno-sanitize-recover=undefined', src, '-o', exe],
        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert cc.returncode == 0, cc.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       universal_newlines=True)
    assert r.returncode == 0, r.stdout
