"""CPU: tools/kernel_asm_diff.py's parse() splits a listing into each kernel's normalised instructions and its descriptor lines;
rename() pairs a renamed kernel with its new name, also where the other tree has a kernel of that name."""
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


TWO = """\
_ZN4leon5k_oldEv:
\ts_nop 1
\ts_endpgm
.Lfunc_end0:
_ZN4leon5k_newEv:
\ts_nop 2
\ts_endpgm
.Lfunc_end1:
"""


def test_rename_onto_an_existing_name_wins_and_the_displaced_kernel_is_gone():
    old, new = "_ZN4leon5k_oldEv", "_ZN4leon5k_newEv"
    there = kernel_asm_diff.parse(TWO.splitlines(True))
    assert list(there) == [old, new]
    # whichever of the two the listing holds first
    for a in (there, dict(reversed(list(there.items())))):
        got, displaced = kernel_asm_diff.rename(a, {old: new})
        assert got == {new: (["s_nop 1", "s_endpgm"], [])} and displaced == [new]
    # no rename, and a rename onto a free name: nothing is displaced
    assert kernel_asm_diff.rename(there, {}) == (there, [])
    assert kernel_asm_diff.rename(there, {old: "_ZN4leon6k_thirdEv"}) == ({"_ZN4leon6k_thirdEv": there[old], new: there[new]}, [])
