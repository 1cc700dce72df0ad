"""CPU: the library's sources hold one code path per decision.  Experiments that were measured and dropped live in git
history, not behind environment variables or compile-time switches of the shipped code (removed variants are
at a1657a4).  A new knob has to be added to KEPT_ENV on purpose."""
import os
import re

from helpers import ROOT

CSRC = os.path.join(ROOT, "mpeg1video-decoder-webgl_amd", "csrc")

# the debugging aids that tests or open defects rely on
KEPT_ENV = {
    "LEON_CONTIGUOUS", "LEON_DEBUG_ZERO_ALLOC", "LEON_DEBUG_POISON", "LEON_DEBUG_SERIAL", "LEON_DEBUG_CAPTURE",
    "LEON_DEBUG_GPU_PARSER_LIMIT", "LEON_DEBUG_NO_SLABS", "LEON_DEBUG_PIPE_TIMING",
}


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_environment_variables_read_by_the_library_are_the_kept_debugging_aids():
    names = set()
    for src in ("leon_hip.cpp", "leon_pipeline_impl.h", "leon_kernels.h", "leon_vlc_gpu.h"):
        text = _read(src)
        names |= set(re.findall(r'\b(?:getenv|env_int)\(\s*"(\w+)"', text))
        # every read names its variable literally (env_int's own getenv(name) is the one exception)
        others = [a for a in re.findall(r"\bgetenv\(\s*([^)]*)\)", text) if not a.startswith('"') and a != "name"]
        assert not others, "%s: getenv of a computed name: %s" % (src, others)
    assert names == KEPT_ENV, "added: %s, gone: %s" % (sorted(names - KEPT_ENV), sorted(KEPT_ENV - names))


def test_device_headers_have_no_compile_time_switches():
    for src in ("leon_kernels.h", "leon_vlc_gpu.h"):
        hits = [line.strip() for line in _read(src).splitlines() if re.match(r"\s*#\s*(?:if|ifdef|ifndef)\b.*\bLEON_", line)]
        assert not hits, "%s: %s" % (src, hits)
