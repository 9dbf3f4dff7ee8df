"""A build's Bloom filter applied to a key column (hwbrj_build_filter_keys_device; include/hwbrj.h "The
build's filter as a selection bitmap"): the export, the Python name and signature, the refusal decided
before any device call (pointers that are never dereferenced) and the wrapper's argument checks. No
GPU."""
import ctypes
import inspect
import types

import pytest

KEYS, OUT = 0x1000, 0x2000
UNWRITTEN = 0x5A5A5A5A5A5A5A5A


def test_library_exports_the_entry(hw):
    assert hasattr(hw.lib(), "hwbrj_build_filter_keys_device")


def test_python_name_and_signature(hw):
    assert hasattr(hw, "filter_keys_device") and "filter_keys_device" in hw.__all__
    p = inspect.signature(hw.filter_keys_device).parameters
    assert list(p) == ["build", "Sk", "stream", "s_valid", "out"]
    assert p["stream"].default is None and p["stream"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    for name in ("s_valid", "out"):
        assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default is None
    rows = [r for r in hw._signatures() if r[0] == "hwbrj_build_filter_keys_device"]
    assert len(rows) == 1 and rows[0][1] is ctypes.c_int and len(rows[0][2]) == 8


@pytest.mark.parametrize("nS", [0, 40])
def test_a_null_build_gives_2_and_writes_nothing(hw, nS):
    L = hw.lib()
    n, ms = ctypes.c_uint64(UNWRITTEN), ctypes.c_double(-7.0)
    rc = L.hwbrj_build_filter_keys_device(None, KEYS, None, nS, OUT, ctypes.byref(n), None, ctypes.byref(ms))
    assert rc == 2 and b"build is NULL" in L.hwbrj_last_error()
    assert (n.value, ms.value) == (UNWRITTEN, -7.0)


def _col(n=8):
    import torch
    return torch.zeros(n, dtype=torch.int32)


def test_wrapper_refuses_a_freed_build_and_a_non_build(hw):
    import torch
    b = hw.Build(0, torch.device("cuda:0"))
    with pytest.raises(ValueError, match="freed"):
        hw.filter_keys_device(b, _col())
    with pytest.raises(ValueError, match="must be a Build"):
        hw.filter_keys_device(None, _col())
    with pytest.raises(ValueError, match="must be a Build"):
        hw.filter_keys_device(0x1234, _col())


def test_wrapper_refuses_columns_on_another_device(hw, monkeypatch):
    """A live handle on cuda:1 and a column elsewhere: refused by the wrapper, before the library sees
    the handle (the library here answers hwbrj_set_device only)."""
    import torch
    fake = types.SimpleNamespace(hwbrj_set_device=lambda i: 0)
    monkeypatch.setattr(hw, "lib", lambda: fake)
    b = hw.Build(0x1234, torch.device("cuda:1"))
    try:
        with pytest.raises(ValueError, match="but the build is on cuda:1"):
            hw.filter_keys_device(b, _col())
    finally:
        b._h = 0  # (never a real handle: nothing to free)


def test_wrapper_refuses_bad_bitmaps(hw):
    """_check_valid's checks, which come before the build is looked at."""
    import torch
    b = hw.Build(0, torch.device("cuda:0"))
    Sk = _col(40)
    with pytest.raises(ValueError, match="s_valid must be a torch.uint8 bitmap"):
        hw.filter_keys_device(b, Sk, s_valid=torch.zeros(5, dtype=torch.int32))
    with pytest.raises(ValueError, match="s_valid has 4 bytes, 40 keys need 5"):
        hw.filter_keys_device(b, Sk, s_valid=torch.zeros(4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="s_valid has 39 entries for 40 keys"):
        hw.filter_keys_device(b, Sk, s_valid=torch.ones(39, dtype=torch.bool))
    with pytest.raises(ValueError, match="s_valid must be a contiguous 1-D tensor"):
        hw.filter_keys_device(b, Sk, s_valid=torch.zeros((5, 2), dtype=torch.uint8))


def test_wrapper_refuses_a_bad_out(hw):
    """The checks of `out`, which also come before the build is looked at: 40 keys need 8 bytes (two
    dwords), at a 4-byte boundary."""
    import torch
    b = hw.Build(0, torch.device("cuda:0"))
    Sk = _col(40)
    with pytest.raises(ValueError, match="out must be a torch.uint8 tensor"):
        hw.filter_keys_device(b, Sk, out=torch.zeros(8, dtype=torch.int32))
    with pytest.raises(ValueError, match="out must be a torch.uint8 tensor"):
        hw.filter_keys_device(b, Sk, out=bytearray(8))
    with pytest.raises(ValueError, match="out has 7 bytes, 40 keys need 8"):
        hw.filter_keys_device(b, Sk, out=torch.zeros(7, dtype=torch.uint8))
    with pytest.raises(ValueError, match="out must be a contiguous 1-D tensor"):
        hw.filter_keys_device(b, Sk, out=torch.zeros((8, 2), dtype=torch.uint8)[:, 0])
    base = torch.zeros(64, dtype=torch.uint8)
    off = (1 - base.data_ptr()) % 4  # base[off:] starts one byte past a 4-byte boundary
    assert base[off:].data_ptr() % 4 == 1
    with pytest.raises(ValueError, match="out must start at a 4-byte boundary"):
        hw.filter_keys_device(b, Sk, out=base[off:])
    with pytest.raises(ValueError, match="freed"):  # a good out: the next check is the build's
        hw.filter_keys_device(b, Sk, out=torch.zeros(8, dtype=torch.uint8))
