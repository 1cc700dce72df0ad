"""CPU: csrc/leon_motion.h as a stand-alone program under the address and undefined-behaviour sanitizers (tests/native/motion_check.cpp):
the walk of k_motion's 256 lanes over mbs = 1 .. 2100 and 65536 macroblocks against the plain loop, with every map allocated at exactly
its padded size and the record at exactly its pitch -- the last lane's 4- and 16-byte reads stay inside the padding and the tail stores
inside the record, for every count.  Nothing is loaded into this process."""
import os
import shutil
import subprocess

import pytest

from helpers import ROOT


def test_motion_walk_under_address_and_ub_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "motion_check")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", exe, os.path.join(ROOT, "tests", "native", "motion_check.cpp")], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "motion_check: 0 failed" in r.stdout, r.stdout[-1000:]
