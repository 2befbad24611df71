"""Every kernel launch of lion_amd/csrc goes through common.h's lion_launch: the launch syntax, the
dynamic-LDS limit slots and the call that configures them exist in common.h alone, and the compile-time constant a
generic lambda takes (BoolC / IntC) has one definition there."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lion_amd", "csrc")


def _sources():
    names = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".h")))
    assert "common.h" in names and len(names) > 20
    return {n: open(os.path.join(CSRC, n)).read() for n in names}


def test_launch_syntax_and_lds_slots_only_in_common_h():
    src = _sources()
    for token in ("<<<", "LionLdsLimit", "lion_dynamic_lds("):
        assert [n for n, text in src.items() if token in text] == ["common.h"], token
    common = src["common.h"]
    assert common.count("<<<") == 1                      # the helper's own launch
    assert "LION_LAUNCH_CHECK" in common                 # older sources built against these headers use it
    users = [n for n, text in src.items() if "lion_launch<" in text and n != "common.h"]
    assert len(users) >= 22, users                       # every .hip with a kernel, and conv3d_split_kernel.h


def test_constant_wrapper_has_one_definition():
    src = _sources()
    for name in ("BoolC", "IntC", "BoolT"):
        pat = re.compile(r"(struct\s+%s\b|using\s+%s\s*=)" % (name, name))
        where = [(n, len(pat.findall(text))) for n, text in src.items() if pat.search(text)]
        assert where == ([] if name == "BoolT" else [("common.h", 1)]), (name, where)
    assert "std::bool_constant" in src["common.h"] and "std::integral_constant" in src["common.h"]
