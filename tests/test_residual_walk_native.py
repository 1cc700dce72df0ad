"""CPU: csrc/leon_residual.h as a stand-alone program under the address and undefined-behaviour sanitizers
(tests/native/residual_check.cpp): every task and lane of k_residual's decomposition walked for 16x16, 48x32, 128x16, 144x32, 592x32
and 4096x4096 with the record allocated at exactly record_bytes -- every specified element stored exactly once, no pad column by a lane
that must not store, nothing outside the record, and the tasks' group ids a permutation of 0 .. n_y + 2 n_c - 1.  Nothing is loaded
into this process."""
import os
import shutil
import subprocess

import pytest

from helpers import ROOT


def test_residual_walk_under_address_and_ub_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "residual_check")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", exe, os.path.join(ROOT, "tests", "native", "residual_check.cpp")], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "residual_check: 0 failed" in r.stdout, r.stdout[-1000:]
