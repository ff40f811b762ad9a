"""
The row helpers of the batched oracles (csrc/ehm_batch_host.h: sort_by_commutation, gather_rows,
scatter_rows, merge_retried) as a stand-alone host program under the address and
undefined-behaviour sanitizers.  tests/host/batch_host_main.cpp holds the cases and the plain
loops the helpers are checked against; this file builds it with the host compiler of build.py
and runs it as a child process.
"""

import os
import subprocess

from explicit_hybrid_mpc_amd import build as lib_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batch_row_helpers_under_sanitizers(tmp_path):
    exe = str(tmp_path / 'batch_host_main')
    src = os.path.join(ROOT, 'tests', 'host', 'batch_host_main.cpp')
    cmd = [lib_build._cxx(), '-O1', '-g', '-std=c++17', '-Wall', '-Werror',
           '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
           '-I', lib_build.SRC_DIR, src, '-o', exe]
    if os.path.basename(cmd[0]).startswith('hipcc'):
        cmd[1:1] = ['-x', 'c++']         # no host g++: the header has no device code to compile
    subprocess.run(cmd, check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'batch host helpers ok' in out.stdout
