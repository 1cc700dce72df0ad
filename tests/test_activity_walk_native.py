"""CPU: csrc/leon_activity.h as a stand-alone program under the address and undefined-behaviour sanitizers
(tests/native/activity_check.cpp): the task and lane walk of k_activity and the walk of k_activity_summary in plain C++ against the
plain loop over the groups, for the widths and heights of tests/activity_cases.py, widths 1 .. 40, 120 x 68, 256 x 256 and a group whose
sum passes 2^32 -- with every list and map allocated at exactly its padded size, the capacity exactly grp_off[last] and the record at
exactly its pitch.  Nothing is loaded into this process."""
import os
import shutil
import subprocess

import pytest

from helpers import ROOT


def test_activity_walk_under_address_and_ub_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "activity_check")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", exe, os.path.join(ROOT, "tests", "native", "activity_check.cpp")], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "activity_check: 0 failed" in r.stdout, r.stdout[-1000:]
