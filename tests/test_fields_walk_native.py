"""CPU: csrc/leon_fields.h as a stand-alone program under the address and undefined-behaviour sanitizers (tests/native/fields_check.cpp):
the walk of k_fields' lanes over every tile of the output -- tables into the tile, horizontal pass, vertical pass into the packed tile,
16-byte lines and end elements out -- against the plain loop over samples, on heap buffers of exactly source_bytes whose last item's
channels end at the buffer's last byte, and the fp16 / bf16 rounding value by value.  Nothing is loaded into this process."""
import os
import shutil
import subprocess

import pytest

from helpers import ROOT


def test_fields_walk_under_address_and_ub_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "fields_check")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", exe, os.path.join(ROOT, "tests", "native", "fields_check.cpp")], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "fields_check:" in r.stdout and " 0 failed" in r.stdout, r.stdout[-1000:]
