"""TPE_DRAW_SCREEN_RUN (tpe_switches.hpp) reaches the chunk's screen_run and the
captured-graph key (tpe_level_plan.hpp): tests/host/screen_run_plan_check.cpp,
pure host code, built host-only with the address and undefined-behaviour
sanitizers and run as a stand-alone program (no GPU)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


def test_screen_run_plan_host_checks(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.fail('hipcc not found at %s' % HIPCC)
    exe = str(tmp_path / 'screen_run_plan_check')
    src = os.path.join(ROOT, 'tests', 'host', 'screen_run_plan_check.cpp')
    cc = subprocess.run(
        [HIPCC, '-x', 'hip', '--cuda-host-only', '-std=c++17', '-O1', '-g', '-Wall',
         '-Xarch_host', '-fsanitize=address,undefined',
         '-Xarch_host', '-fno-sanitize-recover=undefined', src, '-o', exe],
        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert cc.returncode == 0, cc.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       universal_newlines=True)
    assert r.returncode == 0, r.stdout
