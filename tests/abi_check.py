"""What the CPU suites ask of C-ABI entry points by name, in one place: header <-> ctypes table <-> built library."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    """include/lion_hip.h without its block comments"""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lion_hip.h")).read(), flags=re.S)


def declared_bound_and_exported(names, returns="int"):
    """every name is declared in the header (returning `returns`, a regular expression), bound in _lib.SIGNATURES, exported by
    the library, and loaded by _lib.load() with the bound argument types"""
    from lion_amd import _lib
    assert os.path.exists(_lib.SO_PATH), "run __graft_entry__.build() first"
    txt, lib = header(), ctypes.CDLL(_lib.SO_PATH)
    for name in names:
        assert re.search(r"\b%s\s+%s\s*\(" % (returns, name), txt), f"{name} not declared in include/lion_hip.h"
        assert name in _lib.SIGNATURES, f"{name} not bound in _lib.SIGNATURES"
        assert hasattr(lib, name), f"{name} declared in include/lion_hip.h but not exported by the library"
        assert getattr(_lib.load(), name).argtypes == _lib.SIGNATURES[name][1]
