"""CPU: csrc/leon_gauge.h as a stand-alone program under the address and undefined-behaviour sanitizers (tests/native/gauge_check.cpp):
the walk of k_gauge's 64 lanes over a box's macroblocks against the plain double loop for each set of sources, the record's judgement
and its order, word 0 = w * h, and the words at 2^24 * 65535 on the largest grid -- with every motion and activity record allocated at
exactly record_bytes.  Nothing is loaded into this process."""
import os
import shutil
import subprocess

import pytest

from helpers import ROOT


def test_gauge_walk_under_address_and_ub_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "gauge_check")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", exe, os.path.join(ROOT, "tests", "native", "gauge_check.cpp")], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "gauge_check: 0 failed" in r.stdout, r.stdout[-1000:]
