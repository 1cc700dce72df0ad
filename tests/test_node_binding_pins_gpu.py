"""GPU, under Node: the two handles of napi/leon_napi.node pinned case by case (tests/node_handle_pins_gpu.js) -- a create() decoder
and two pipelines on tests/golden/streams/tiny_ip_32x32.jsv, every method with too few arguments, wrong types, wrong typed arrays, no
record and 65536 records, windows and indices that are not there, and every method again after destroy().  Every case is refused on
the host; tests/golden/node_handle_pins_gpu.json holds {class, message} of each, recorded once from the addon as it stood before its
call shapes were folded into helpers (tests/test_node_binding_pins.py: the same for what needs no device)."""
import os
import shutil

import pytest

from helpers import ROOT
from test_node_binding_pins import ADDON, assert_same_cases, run_pins

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")]


def test_handles_refuse_what_they_refused():
    assert os.path.exists(ADDON), "leon_napi.node is not built (__graft_entry__.build())"
    got, want = run_pins("node_handle_pins_gpu", os.path.join(ROOT, "tests", "golden", "streams", "tiny_ip_32x32.jsv"), timeout=120)
    assert len(want) > 200
    assert_same_cases(got, want)
