"""The ctypes declarations of hwbloomradixjoin_amd.lib() against the prototypes of include/hwbrj.h, and the
argument check every tuple wrapper makes before the library is called. No GPU."""
import ctypes
import os
import re

import pytest

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hwbrj.h")


def _prototypes():
    """{name: [is this parameter a pointer, ...]} of every hwbrj_* prototype of the header."""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    protos = {}
    for m in re.finditer(r"\b(hwbrj_\w+)\s*\(([^()]*)\)\s*;", text):
        params = [p.strip() for p in m.group(2).split(",")]
        protos[m.group(1)] = [] if params == ["void"] else ["*" in p for p in params]
    return protos


def _is_pointer(t):
    return t in (ctypes.c_void_p, ctypes.c_char_p, ctypes.c_wchar_p) or issubclass(t, ctypes._Pointer)


def test_declared_argtypes_match_the_header(hw, monkeypatch):
    """Every hwbrj_* entry lib() declares argtypes for has a prototype with as many parameters, pointers
    exactly where the ctypes entry is a pointer type. (A fresh load: only lib()'s own declarations.)"""
    monkeypatch.setattr(hw, "_LIB", None)
    L = hw.lib()
    declared = {n: f.argtypes for n, f in vars(L).items()
                if n.startswith("hwbrj_") and isinstance(f, ctypes._CFuncPtr) and f.argtypes is not None}
    assert len(declared) >= 50, sorted(declared)  # (the enumeration found lib()'s declarations)
    protos = _prototypes()
    for name, argtypes in sorted(declared.items()):
        assert name in protos, f"{name} is declared but include/hwbrj.h has no prototype of it"
        assert len(argtypes) == len(protos[name]), (name, len(argtypes), len(protos[name]))
        assert [_is_pointer(t) for t in argtypes] == protos[name], name


def test_join_materialize_checks_its_relations_with_a_capacity_too(hw):
    """CPU tensors are refused by the wrapper whether or not capacity is given: with one, they used to
    reach the device entry as host pointers."""
    import torch
    R, S = torch.zeros((8, 2), dtype=torch.int32), torch.zeros((8, 2), dtype=torch.int32)
    with pytest.raises(ValueError, match="R must be a contiguous"):
        hw.join_materialize_device(R, S, capacity=4)
    with pytest.raises(ValueError, match="R must be a contiguous"):
        hw.join_materialize_device(R, S)
