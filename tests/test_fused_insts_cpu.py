"""The fused Edgewise pair is instantiated from two lists that cannot include each other: MOPK_FUSED_INSTS in csrc/fused_common.h
(declarations, dispatch, size lookups) and NTS x DKS in mop_amd/build.py (what is compiled).  They must name the same pairs."""
import os
import re

from conftest import ROOT


def test_the_x_macro_lists_exactly_what_build_py_compiles():
    from mop_amd import build
    src = open(os.path.join(ROOT, "mop_amd", "csrc", "fused_common.h")).read()
    lines = [ln for ln in src.splitlines() if ln.startswith("#define MOPK_FUSED_INSTS(X)")]
    assert len(lines) == 1 and not lines[0].rstrip().endswith("\\"), "the list is one #define on one line"
    pairs = [(int(nt), int(dk)) for nt, dk in re.findall(r"\bX\((\d+),\s*(\d+)\)", lines[0])]
    assert pairs == [(nt, dk) for nt in build.NTS for dk in build.DKS]
    # and nothing spells an instantiation by hand any more
    for f in build.FUSED:
        text = open(os.path.join(build.CSRC, f)).read()
        assert not re.search(r"_nt\d+_dk\d+|_nt##[A-Z_]+##_dk(16|32|64)", text), f
