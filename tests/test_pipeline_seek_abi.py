"""CPU: leon_pipeline_seek is part of the C ABI -- a C program compiled against include/leon_pipeline.h calls it, the
mode constants have their documented values, libleon_hip.so exports the symbol and the ctypes mirror declares it."""
import ctypes as C
import os
import subprocess

from helpers import ROOT


def test_a_c_program_calls_leon_pipeline_seek(tmp_path):
    src = tmp_path / "seek.c"
    src.write_text(
        '#include <stdio.h>\n#include "leon.h"\n#include "leon_pipeline.h"\n'
        "int main(void){\n"
        "    int (*fn)(leon_pipeline*, double, int32_t, int64_t*) = leon_pipeline_seek;\n"
        "    int64_t first = -7;\n"
        "    int rc = fn(NULL, 1.0, LEON_PIPELINE_SEEK_KEY, &first);\n"       # a null pipeline is refused, nothing written
        '    printf("%d %d %d %lld\\n", LEON_PIPELINE_SEEK_KEY, LEON_PIPELINE_SEEK_EXACT, rc, (long long)first);\n'
        "    return 0;}\n")
    exe = tmp_path / "seek"
    lib = os.path.join(ROOT, "mpeg1video-decoder-webgl_amd", "lib")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src), "-L", lib, "-lleon_hip",
                           "-Wl,-rpath," + lib])
    key, exact, rc, first = subprocess.check_output([str(exe)], text=True).split()
    assert (int(key), int(exact)) == (0, 1)
    assert int(rc) == -1 and int(first) == -7          # LEON_ERR_INVALID


def test_the_library_exports_it_and_the_binding_declares_it():
    import leon_ctypes as L
    lib = L.load()
    assert hasattr(lib, "leon_pipeline_seek")
    assert "leon_pipeline_seek" in L.PIPELINE_SYMBOLS
    assert lib.leon_pipeline_seek.argtypes == [C.c_void_p, C.c_double, C.c_int32, C.POINTER(C.c_int64)]
    assert (L.PIPELINE_SEEK_KEY, L.PIPELINE_SEEK_EXACT) == (0, 1)
    assert hasattr(L.Pipeline, "seek")
    first = C.c_int64(-7)
    assert lib.leon_pipeline_seek(None, 0.0, 0, C.byref(first)) == L.ERR_INVALID and first.value == -7
    assert lib.leon_abi_version() == 3
