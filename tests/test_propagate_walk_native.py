"""CPU: csrc/leon_propagate.h as a stand-alone program under the address and undefined-behaviour sanitizers
(tests/native/propagate_check.cpp): the walk of k_propagate's lanes over a map's work units, on both paths and through every plane
group, against the plain loop over cells, on heap buffers of exactly maps_bytes with sources in the last slot and vectors into its
bottom-right corner -- a dword read past the buffer fails here.  Nothing is loaded into this process."""
import os
import shutil
import subprocess

import pytest

from helpers import ROOT


def test_propagate_walk_under_address_and_ub_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "propagate_check")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", exe, os.path.join(ROOT, "tests", "native", "propagate_check.cpp")], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "propagate_check: 0 failed" in r.stdout, r.stdout[-1000:]
