"""CPU: the host code holds what it gets from the runtime -- device and pinned memory, events, streams -- in the owning types of
csrc/leon_owned.h.  Raw calls of the runtime's allocation, event and stream functions are left in the places listed here and nowhere
else: a new one has to be added to the list on purpose."""
import os
import re

from helpers import ROOT

CSRC = os.path.join(ROOT, "mpeg1video-decoder-webgl_amd", "csrc")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


# Who may call the runtime for memory, events and streams (leon_owned.h: everything else holds an owning type).  The whole list: the
# pool and its two functions, the policies of the owning types beside them, and the two exported calls that hand raw memory to callers.
RAW_RESOURCE_CALL = re.compile(r"\b(hipMalloc|hipHostMalloc|hipExtMallocWithFlags|hipFree|hipHostFree|big_alloc|big_free|hipEventCreate\w*|hipEventDestroy|"
                               r"hipStreamCreate\w*|hipStreamDestroy)\s*\(")
RAW_RESOURCE_CALLS_KEPT = {
    "leon_hip.cpp": [
        "hipError_t big_alloc(void** ptr, size_t bytes, int kind, bool* contiguous = nullptr, bool asked = false)",
        "e = hipExtMallocWithFlags(ptr, need, hipDeviceMallocContiguous);",
        "if (e != hipSuccess) e = hipMalloc(ptr, bytes);",
        "hipError_t big_free(void* p)",
        "return hipFree(p);",
        "return big_alloc(&p, bytes, kind, nullptr, asked) == hipSuccess ? p : nullptr;",                  # DeviceMem::get
        "void DeviceMem::give(void* p) { (void)big_free(p); }",
        "return hipHostMalloc(&p, bytes, hipHostMallocDefault) == hipSuccess ? p : nullptr;",              # PinnedMem::get
        "void PinnedMem::give(void* p) { (void)hipHostFree(p); }",
        "return hipEventCreateWithFlags(&e, flags) == hipSuccess ? e : nullptr;",                          # EventTraits::create
        "void EventTraits::destroy(hipEvent_t e) { (void)hipEventDestroy(e); }",
        "return hipStreamCreateWithFlags(&s, flags) == hipSuccess ? s : nullptr;",                         # StreamTraits::create
        "return hipStreamCreateWithPriority(&s, flags, priority) == hipSuccess ? s : nullptr;",
        "void StreamTraits::destroy(hipStream_t s) { (void)hipStreamDestroy(s); }",
        "if (big_alloc(ptr, bytes, kBigCaller, &c) != hipSuccess) {",                                      # leon_device_malloc
        "HIP_TRY(big_free(ptr));",                                                                         # leon_device_free
    ],
    "leon_pipeline_impl.h": [],
}


def test_raw_resource_calls_are_the_policies_and_the_pool():
    for src, kept in RAW_RESOURCE_CALLS_KEPT.items():
        code = [re.sub(r"//.*", "", line).strip() for line in _read(src).splitlines()]
        found = [line for line in code if RAW_RESOURCE_CALL.search(line)]
        assert found == kept, "%s: new: %s, gone: %s" % (src, [x for x in found if x not in kept], [x for x in kept if x not in found])
