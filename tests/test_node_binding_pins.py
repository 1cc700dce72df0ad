"""CPU, under Node: the JavaScript host's two layers pinned case by case, without a device.

tests/node_wrapper_pins.js runs js/leon_pipeline.js over a recording stand-in for the addon (opts.backend): every constructor option and
every method, with what reached the backend or {class, message} of what was thrown.  tests/node_addon_refusal_pins.js asks the real
napi/leon_napi.node for everything it refuses before it touches a device -- an accepted option set is pinned by the library's "no
sequence header" on a 16-byte stream.  Each prints one JSON object; the fixtures under tests/golden/ were recorded once, from the layer
as it stood before its call shapes were folded into helpers, and a test only compares: a changed message, class, argument order, typed
array kind or length is a fixture diff somebody has to want."""
import json
import os
import shutil
import subprocess

import pytest

from helpers import ROOT

ADDON = os.path.join(ROOT, "mpeg1video-decoder-webgl_amd", "napi", "leon_napi.node")


def run_pins(script, *args, timeout=60):
    """the script's cases against its fixture, case by case: (got, want)"""
    out = subprocess.run(["node", os.path.join(ROOT, "tests", script + ".js")] + list(args), capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-3000:]
    got = json.loads(out.stdout)
    with open(os.path.join(ROOT, "tests", "golden", script + ".json")) as f:
        want = json.load(f)
    return got, want


def assert_same_cases(got, want):
    assert list(got) == list(want), (sorted(set(got) - set(want)), sorted(set(want) - set(got)))
    differ = [name for name in want if got[name] != want[name]]
    assert not differ, "\n".join("%s\n  got  %s\n  want %s" % (n, json.dumps(got[n])[:600], json.dumps(want[n])[:600]) for n in differ[:10])


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_wrapper_over_a_recording_backend():
    got, want = run_pins("node_wrapper_pins")
    assert len(want) > 350
    assert_same_cases(got, want)


@pytest.mark.skipif(shutil.which("node") is None or not os.path.exists(ADDON), reason="node or the addon is not there")
def test_addon_refusals_without_a_device():
    """(the script ends by itself only if every refusal released its threadsafe function: the timeout is that check)"""
    got, want = run_pins("node_addon_refusal_pins", timeout=60)
    assert len(want) > 100
    assert_same_cases(got, want)
