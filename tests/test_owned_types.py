"""CPU: the owning types of csrc/leon_owned.h (device and pinned buffers, mirrors, stream and event handles), as a stand-alone
program under the address and undefined-behaviour sanitizers: tests/native/owned_check.cpp instantiates them with policies that count
what is live and refuse the k-th request.  Nothing is loaded into this process."""
import os
import shutil
import subprocess

import pytest

from helpers import ROOT


def test_owning_types_under_address_and_ub_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "owned_check")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", exe, os.path.join(ROOT, "tests", "native", "owned_check.cpp")], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert " 0 failed, 0 live at exit" in r.stdout, r.stdout[-1000:]


def test_the_header_needs_no_hip():
    """plain C++17: g++ compiles it alone"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    text = open(os.path.join(ROOT, "mpeg1video-decoder-webgl_amd", "csrc", "leon_owned.h")).read()
    assert "hip" not in "".join(line for line in text.splitlines() if line.lstrip().startswith("#include"))
    b = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c++", "-include",
                        os.path.join(ROOT, "mpeg1video-decoder-webgl_amd", "csrc", "leon_owned.h"), "/dev/null"], capture_output=True, text=True, timeout=120)
    assert b.returncode == 0, b.stderr[-3000:]
