"""CPU: tools/kernel_asm_diff.py's parse() splits a listing into each kernel's normalised instructions and its descriptor lines."""
import os
import sys

from helpers import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_asm_diff  # noqa: E402

LISTING = """\
\t.text
_ZN4leon8k_copy16EPKvPvm:
\ts_load_dword s0, s[0:1], 0x0 ; comment
.LBB3_2:
\ts_cbranch_scc1 .LBB3_2
\t.p2align 6
\ts_endpgm
.Lfunc_end3:
\t.amdhsa_kernel _ZN4leon8k_copy16EPKvPvm
\t\t.amdhsa_group_segment_fixed_size 5120
\t\t.amdhsa_next_free_vgpr 12 ; note
\t.end_amdhsa_kernel
_ZN4leon6helperEv:
\ts_nop 0
"""


def test_parse_keeps_instructions_and_descriptor_apart():
    got = kernel_asm_diff.parse(LISTING.splitlines(True))
    assert got == {"_ZN4leon8k_copy16EPKvPvm": (["s_load_dword s0, s[0:1], 0x0", "s_cbranch_scc1 .LBB_2", "s_endpgm"],
                                                [".amdhsa_group_segment_fixed_size 5120", ".amdhsa_next_free_vgpr 12"])}
