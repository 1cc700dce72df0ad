"""CPU: boxes suppressed and matched by overlap (include/leon_pipeline.h, leon_pipeline_suppress_regions and
leon_pipeline_match_regions) -- the structs' sizes and the symbols; leon_pipeline_suppress_record and leon_pipeline_match_record, the
library's sort and walk, against the definitions in Python integers on every case of tests/overlap_cases.py, the words of refused
rows still holding the sentinel; every LEON_ERR_INVALID of the record calls and of the diagnostics (which refuse before a device is
asked for), the outputs untouched; the LDS figures the header states.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import overlap_cases as O
from helpers import ROOT


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


FILL = O.FILL


def test_struct_sizes_and_symbols(L, tmp_path):
    cfg, sup, mat = L.PipelineOverlapConfig, L.PipelineSuppressRegionsCall, L.PipelineMatchRegionsCall
    assert C.sizeof(cfg) == 16 and [getattr(cfg, f).offset for f in ("measure", "threshold", "reserved")] == [0, 4, 8]
    assert C.sizeof(sup) == 96
    assert [getattr(sup, f).offset for f in ("regions", "scores", "n", "k", "score_stride", "reserved0", "device_out", "device_order", "device_by", "device_count",
                                             "device_status", "stream", "reserved")] == [0, 8, 16, 20, 24, 28, 32, 40, 48, 56, 64, 72, 80]
    assert C.sizeof(mat) == 96
    assert [getattr(mat, f).offset for f in ("a", "b", "n", "ka", "kb", "reserved0", "device_match_a", "device_match_b", "device_overlap", "device_count", "device_status_a",
                                             "device_status_b", "stream", "reserved")] == [0, 8, 16, 20, 24, 28, 32, 40, 48, 56, 64, 72, 80, 88]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "leon_pipeline.h"\nint main(void){printf("%zu %zu %zu %d %d\\n", sizeof(leon_pipeline_overlap_config), '
                   'sizeof(leon_pipeline_suppress_regions_call), sizeof(leon_pipeline_match_regions_call), LEON_OVERLAP_IOU, LEON_OVERLAP_IOMIN);return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "sizes"), str(src)])
    assert subprocess.check_output([str(tmp_path / "sizes")], text=True).split() == ["16", "96", "96", "0", "1"]
    assert (L.OVERLAP_IOU, L.OVERLAP_IOMIN, L.OVERLAP_MAX_ROWS) == (0, 1, 1024)
    header = open(os.path.join(ROOT, "include", "leon_pipeline.h")).read()
    for step in ("suppress", "match"):
        for sym in ("leon_pipeline_%s_record", "leon_pipeline_%s_regions_device", "leon_pipeline_%s_regions", "leon_pipeline_%s_kernel"):
            assert hasattr(L.load(), sym % step) and sym % step in L.PIPELINE_SYMBOLS and re.search(r"\b%s\(" % (sym % step), header), sym % step


@pytest.mark.parametrize("index", range(len(O.suppress_cases())), ids=[c.name for c in O.suppress_cases()])
def test_suppress_record_against_the_definition(L, index):
    c = O.suppress_cases()[index]
    want = O.expected_suppress(L, index)
    k = c.rows.shape[1]
    for s in range(c.rows.shape[0]):
        sc = None if c.scores is None else c.scores[s * k * c.stride:]
        got = L.suppress_record(c.fw, c.fh, c.n_frames, c.rows[s], sc, score_stride=c.stride, threshold_q16=c.threshold, measure=c.measure, fill=FILL)
        O.assert_equal(got, [w[s] for w in want], O.SUPPRESS_NAMES, "%s, set %d" % (c.name, s))


@pytest.mark.parametrize("index", range(len(O.match_cases())), ids=[c.name for c in O.match_cases()])
def test_match_record_against_the_definition(L, index):
    c = O.match_cases()[index]
    want = O.expected_match(L, index)
    for s in range(c.a.shape[0]):
        got = L.match_record(c.fw, c.fh, c.n_frames, c.a[s], c.b[s], fill=FILL, **c.kw())
        O.assert_equal(got, [w[s] for w in want], O.MATCH_NAMES, "%s, set %d" % (c.name, s))


def test_optional_outputs_may_be_null(L):
    c = next(c for c in O.suppress_cases() if c.name == "chain")
    for off in ("with_out", "with_order", "with_status"):
        out, order, by, count, status = L.suppress_record(c.fw, c.fh, c.n_frames, c.rows[0], c.scores, threshold_q16=c.threshold, fill=FILL, **{off: False})
        assert by.tolist() == [-1, 0, -1] and count == 2
        assert ((out == FILL).all(), (order == FILL).all(), (status == FILL).all()) == (off == "with_out", off == "with_order", off == "with_status")
    ma, mb, ov, count, sa, sb = L.match_record(c.fw, c.fh, c.n_frames, c.rows[0], c.rows[0], fill=FILL, with_status=False)
    assert ma.tolist() == [0, 1, 2] and count == 3 and (sa == FILL).all() and (sb == FILL).all()


BAD_CONFIGS = [((2, 32768, 0, 0), "measure"), ((-1, 32768, 0, 0), "measure"), ((0, 0, 0, 0), "threshold"), ((1, 65537, 0, 0), "threshold"), ((0, -1, 0, 0), "threshold"),
               ((0, 32768, 1, 0), "reserved"), ((1, 1, 0, -1), "reserved")]


def config(L, words):
    return L.PipelineOverlapConfig(words[0], words[1], (C.c_int32 * 2)(words[2], words[3]))


def test_every_refusal_of_the_config_on_the_record_calls_and_the_diagnostics(L):
    rows = np.array([O.row(0, 0, 10, 10), O.row(4, 0, 10, 10)], dtype=np.int32)
    for words, text in BAD_CONFIGS:
        for call in (lambda cfg: L.suppress_record(64, 64, 1, rows, cfg=cfg), lambda cfg: L.match_record(64, 64, 1, rows, rows, cfg=cfg),
                     lambda cfg: L.suppress_kernel(64, 64, 1, rows, cfg=cfg), lambda cfg: L.match_kernel(64, 64, 1, rows, rows, cfg=cfg)):          # refused before a device is asked for
            with pytest.raises(L.LeonError) as e:
                call(config(L, words))
            assert e.value.code == L.ERR_INVALID and text in str(e.value), (words, str(e.value))
    for words in ((0, 1, 0, 0), (1, 65536, 0, 0)):          # the limits themselves are accepted
        assert L.suppress_record(64, 64, 1, rows, cfg=config(L, words))[3] >= 1 and L.match_record(64, 64, 1, rows, rows, cfg=config(L, words))[3] == 2


def test_refusals_of_the_arguments_leave_the_outputs_alone(L):
    lib, cfg = L.load(), L.PipelineOverlapConfig(0, 32768)
    rows = np.array([[O.row(0, 0, 10, 10), O.row(4, 0, 10, 10)]] * 2, dtype=np.int32)
    scores = np.zeros(32, dtype=np.int32)
    out, order, by, count, status = (np.full(s, FILL, dtype=np.int32) for s in ((2, 2, 8), (2, 2), (2, 2), 2, (2, 2)))
    R, SC, O_, OR, BY, N, S, CF = rows.ctypes.data, scores.ctypes.data, out.ctypes.data, order.ctypes.data, by.ctypes.data, count.ctypes.data, status.ctypes.data, C.byref(cfg)
    E = L.ERR_INVALID
    assert lib.leon_pipeline_suppress_record(64, 64, 1, None, R, 2, SC, 1, O_, OR, BY, N, S) == E
    for fw, fh, nf in ((0, 64, 1), (64, 0, 1), (4097, 64, 1), (64, 4097, 1), (64, 64, -1)):
        assert lib.leon_pipeline_suppress_record(fw, fh, nf, CF, R, 2, SC, 1, O_, OR, BY, N, S) == E, (fw, fh, nf)
        assert lib.leon_pipeline_match_record(fw, fh, nf, CF, R, 2, R, 2, BY, OR, S, N, None, None) == E, (fw, fh, nf)
        assert lib.leon_pipeline_suppress_kernel(0, fw, fh, nf, CF, R, 2, 2, SC, 1, O_, OR, BY, N, S) == E, (fw, fh, nf)
        assert lib.leon_pipeline_match_kernel(0, fw, fh, nf, CF, R, 2, R, 2, 2, BY, OR, S, N, None, None) == E, (fw, fh, nf)
    for k in (0, -1, 1025):
        assert lib.leon_pipeline_suppress_record(64, 64, 1, CF, R, k, SC, 1, O_, OR, BY, N, S) == E
        assert lib.leon_pipeline_match_record(64, 64, 1, CF, R, k, R, 2, BY, OR, S, N, None, None) == E
        assert lib.leon_pipeline_match_record(64, 64, 1, CF, R, 2, R, k, BY, OR, S, N, None, None) == E
        assert lib.leon_pipeline_suppress_kernel(0, 64, 64, 1, CF, R, 2, k, SC, 1, O_, OR, BY, N, S) == E
        assert lib.leon_pipeline_match_kernel(0, 64, 64, 1, CF, R, k, R, 2, 2, BY, OR, S, N, None, None) == E
        assert lib.leon_pipeline_match_kernel(0, 64, 64, 1, CF, R, 2, R, k, 2, BY, OR, S, N, None, None) == E
    for stride in (0, -1, 9):
        assert lib.leon_pipeline_suppress_record(64, 64, 1, CF, R, 2, SC, stride, O_, OR, BY, N, S) == E
        assert lib.leon_pipeline_suppress_record(64, 64, 1, CF, R, 2, None, stride, O_, OR, BY, N, S) == E
        assert lib.leon_pipeline_suppress_kernel(0, 64, 64, 1, CF, R, 2, 2, SC, stride, O_, OR, BY, N, S) == E
    for n in (0, -1, 65536):
        assert lib.leon_pipeline_suppress_kernel(0, 64, 64, 1, CF, R, n, 2, SC, 1, O_, OR, BY, N, S) == E
        assert lib.leon_pipeline_match_kernel(0, 64, 64, 1, CF, R, 2, R, 2, n, BY, OR, S, N, None, None) == E
    # null required pointers: regions, by, count; a, b, match_a, match_b, overlap, count
    for args in ((None, 2, SC, 1, O_, OR, BY, N, S), (R, 2, SC, 1, O_, OR, None, N, S), (R, 2, SC, 1, O_, OR, BY, None, S)):
        assert lib.leon_pipeline_suppress_record(64, 64, 1, CF, *args) == E
        assert lib.leon_pipeline_suppress_kernel(0, 64, 64, 1, CF, args[0], 2, *args[1:]) == E
    good = [R, 2, R, 2, BY, OR, S, N]
    for hole in (0, 2, 4, 5, 6, 7):
        args = list(good)
        args[hole] = None
        assert lib.leon_pipeline_match_record(64, 64, 1, CF, *args, None, None) == E, hole
        assert lib.leon_pipeline_match_kernel(0, 64, 64, 1, CF, *args[:4], 2, *args[4:], None, None) == E, hole
    assert lib.leon_pipeline_match_kernel(0, 64, 64, 1, None, *good[:4], 2, *good[4:], None, None) == E
    assert all((a == FILL).all() for a in (out, order, by, count, status)), "a refused call wrote an output"


def test_the_lds_the_header_states():
    """suppress: 16 bytes a row, 8 a key slot (K rounded up to a power of two), two dwords a row; match: 24 bytes a row of either set and
    a dword"""
    assert 16 * 1024 + 8 * 1024 + 8 * 1024 == 32768 and 24 * 2048 + 4 == 49156 <= 160 * 1024
    for path in ("include/leon_pipeline.h", "mpeg1video-decoder-webgl_amd/csrc/leon_overlap.h", "mpeg1video-decoder-webgl_amd/csrc/leon_pipeline_impl.h"):
        text = open(os.path.join(ROOT, path)).read()
        assert "32768" in text and "49156" in text, path
