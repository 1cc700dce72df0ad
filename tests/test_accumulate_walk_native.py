"""CPU: csrc/leon_accumulate.h as a stand-alone program under the address and undefined-behaviour sanitizers
(tests/native/accumulate_check.cpp): the walk of k_accumulate's lanes over the work units of every plane asked for, on the funnelled
path and the element path, against the plain loop over elements, on heap buffers of exactly slots_bytes with sources in the last slot
and vectors into its bottom-right corner -- a dword read past the buffer fails here.  Nothing is loaded into this process."""
import os
import shutil
import subprocess

import pytest

from helpers import ROOT


def test_accumulate_walk_under_address_and_ub_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "accumulate_check")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", exe, os.path.join(ROOT, "tests", "native", "accumulate_check.cpp")], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "accumulate_check: 0 failed" in r.stdout, r.stdout[-1000:]
