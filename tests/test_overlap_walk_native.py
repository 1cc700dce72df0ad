"""CPU: csrc/leon_overlap.h as a stand-alone program under the address and undefined-behaviour sanitizers
(tests/native/overlap_check.cpp): the library's host texts for a set and a pair of sets (a stable sort and a walk) against
brute-force walks that share nothing with them -- not even the overlap, which they count with 128-bit products -- and against
k_suppress's and k_match's steps taken one thread after the other, 256 threads a step, over an LDS image of exactly the stated size,
with every input and output array allocated at exactly its stated bytes.  Nothing is loaded into this process."""
import os
import re
import shutil
import subprocess

import pytest

from helpers import ROOT


def test_overlap_texts_under_address_and_ub_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "overlap_check")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", exe, os.path.join(ROOT, "tests", "native", "overlap_check.cpp")], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    m = re.search(r"(\d+) sets suppressed, (\d+) pairs of sets matched", r.stdout)
    assert m and int(m.group(1)) >= 300 and int(m.group(2)) >= 250 and "overlap_check: 0 failed" in r.stdout, r.stdout[-1000:]
