"""What launch_class decides on the host for the direct pass behind the
Chebyshev tables (hyperopt_amd/csrc/tpe_tie_plan.hpp) is plain C++:
tests/host/tie_plan_check.cpp checks tie_lean_form -- a suggest's table launch
takes k_score_wave_tie_lean, and each condition on its own (the switch, the
prune mode, the moment width, positions, lpdf outputs, the L2 warm-up) sends it
back to k_score_wave_tie -- and tie_grid: the all-hot case of
tests/test_gpu_tie_lean.py (114 persistent blocks, 57 for the old kernel),
config 4's rows, the caps at a slot's gathered blocks and at one, an exact
quotient, and the covering property for every pair count up to 9000.  Built
host-only with the address and undefined-behaviour sanitizers and run as a
stand-alone program (no GPU)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


def test_tie_plan_host_checks(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.fail('hipcc not found at %s' % HIPCC)
    exe = str(tmp_path / 'tie_plan_check')
    src = os.path.join(ROOT, 'tests', 'host', 'tie_plan_check.cpp')
    cc = subprocess.run(
        [HIPCC, '-x', 'hip', '--cuda-host-only', '-std=c++17', '-O1', '-g', '-Wall',
         '-Xarch_host', '-fsanitize=address,undefined',
         '-Xarch_host', '-fno-sanitize-recover=undefined', src, '-o', exe],
        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert cc.returncode == 0, cc.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       universal_newlines=True)
    assert r.returncode == 0, r.stdout
