"""CPU: the thread protocol of the pipeline (csrc/leon_pipe_flow.h: who waits for what, who wakes them, who owns a job, a window and an
arena) as a stand-alone program: tests/native/flow_check.cpp runs the parser, submit and notify roles on real threads around fake jobs
and windows -- plain runs, held windows, a stream still arriving, seeks, a failure, tear-down at every waiting point -- once under
ThreadSanitizer and once under the address and undefined-behaviour sanitizers.  Each run has a time limit: a deadlock is a failed test
whose output ends with the scenario that hung.  Nothing is loaded into this process and nothing runs on a GPU."""
import os
import shutil
import subprocess

import pytest

from helpers import ROOT

HEADER = os.path.join(ROOT, "mpeg1video-decoder-webgl_amd", "csrc", "leon_pipe_flow.h")
RUN_LIMIT = 120     # seconds: twice the minute a run may take


def _build_and_run(tmp_path, name, sanitize):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / name)
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *sanitize, "-pthread", "-o", exe,
                        os.path.join(ROOT, "tests", "native", "flow_check.cpp")], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    try:
        r = subprocess.run([exe], capture_output=True, text=True, timeout=RUN_LIMIT)
    except subprocess.TimeoutExpired as e:
        out = e.stdout.decode() if isinstance(e.stdout, bytes) else (e.stdout or "")
        pytest.fail("no end after %d s; the last lines printed:\n%s" % (RUN_LIMIT, out[-600:]))
    assert r.returncode == 0, (r.stdout[-1500:] + r.stderr[-6000:])
    last = r.stdout.strip().splitlines()[-1]
    n, rest = last.split(" ", 1)
    assert int(n) > 0 and rest == "scenarios, 0 failed, 0 live at exit", last


def test_thread_protocol_under_thread_sanitizer(tmp_path):
    _build_and_run(tmp_path, "flow_check_tsan", ["-fsanitize=thread"])


def test_thread_protocol_under_address_and_ub_sanitizers(tmp_path):
    _build_and_run(tmp_path, "flow_check_asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def test_the_header_needs_no_hip():
    """plain C++17: g++ compiles it alone"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    text = open(HEADER).read()
    assert "hip" not in "".join(line for line in text.splitlines() if line.lstrip().startswith("#include"))
    b = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c++", "-include", HEADER, "/dev/null"],
                       capture_output=True, text=True, timeout=120)
    assert b.returncode == 0, b.stderr[-3000:]
