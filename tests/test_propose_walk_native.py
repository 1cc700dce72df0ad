"""CPU: csrc/leon_propose.h as a stand-alone program under the address and undefined-behaviour sanitizers
(tests/native/propose_check.cpp): the library's host text for a request (the hot predicate, the flood fill, the box, the filler)
against a brute-force fill that shares nothing with it and against k_propose's steps taken one thread after the other over an LDS
image of exactly the stated size, on every mask of the 3 x 3 and the 4 x 4 grid under both connectivities, on frames smaller than
their grid and on the largest grid -- with every motion and activity record allocated at exactly record_bytes.  Nothing is loaded
into this process."""
import os
import shutil
import subprocess

import pytest

from helpers import ROOT


def test_propose_texts_under_address_and_ub_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "propose_check")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", exe, os.path.join(ROOT, "tests", "native", "propose_check.cpp")], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "65536 masks of 4 x 4" in r.stdout and "propose_check: 0 failed" in r.stdout, r.stdout[-1000:]
