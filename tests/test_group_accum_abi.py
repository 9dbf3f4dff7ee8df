"""Group accumulators of a prepared build (hwbrj_probe_keys_group_accum_device,
hwbrj_build_group_rows_device, hwbrj_build_group_reset; include/hwbrj.h "Group accumulators kept across
batches"): the exports, the Python names, the refusals decided before any device call (pointers that
are never dereferenced) and the wrappers' argument checks. No GPU."""
import ctypes
import inspect
import types

import pytest

KEYS, OUT = 0x1000, 0x2000
UNWRITTEN = 0x5A5A5A5A5A5A5A5A
EXPORTS = ("hwbrj_probe_keys_group_accum_device", "hwbrj_build_group_rows_device", "hwbrj_build_group_reset")


def test_library_exports_the_entries(hw):
    for name in EXPORTS:
        assert hasattr(hw.lib(), name), name


def test_python_names(hw):
    for name in ("AGG_SUM", "AGG_MINMAX", "group_accum_probe_keys_device"):
        assert hasattr(hw, name) and name in hw.__all__, name
    assert (hw.AGG_SUM, hw.AGG_MINMAX) == (0, 1)
    p = inspect.signature(hw.group_accum_probe_keys_device).parameters
    assert list(p) == ["build", "Sk", "Sv", "agg", "stream", "s_valid", "sv_valid"]
    assert p["agg"].default == hw.AGG_SUM and p["stream"].default is None
    for name in ("s_valid", "sv_valid"):
        assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default is None
    p = inspect.signature(hw.Build.group_rows).parameters
    assert list(p) == ["self", "agg", "kind", "capacity", "stream"]
    assert (p["agg"].default, p["kind"].default, p["capacity"].default) == (hw.AGG_SUM, hw.GROUP_ALL, None)
    assert list(inspect.signature(hw.Build.reset_group).parameters) == ["self", "agg"]


@pytest.mark.parametrize("agg", [0, 1, 2, -1])
def test_every_entry_on_a_null_build_gives_2_and_writes_nothing(hw, agg):
    L = hw.lib()
    n, pairs, ms = ctypes.c_uint64(UNWRITTEN), ctypes.c_uint64(UNWRITTEN), ctypes.c_double(-7.0)
    st = hw._Stats()
    ctypes.memset(ctypes.byref(st), 0x5A, ctypes.sizeof(st))
    rc = L.hwbrj_probe_keys_group_accum_device(None, KEYS, None, KEYS, None, 40, agg, ctypes.byref(n), ctypes.byref(pairs),
                                               None, ctypes.byref(st), ctypes.byref(ms))
    assert rc == 2 and b"build is NULL" in L.hwbrj_last_error()
    assert (n.value, pairs.value, ms.value) == (UNWRITTEN, UNWRITTEN, -7.0)
    assert bytes(st) == b"\x5a" * ctypes.sizeof(hw._Stats)
    for kind in (hw.GROUP_MATCHED, hw.GROUP_ALL, 2):
        rc = L.hwbrj_build_group_rows_device(None, agg, kind, OUT, 8, ctypes.byref(n), ctypes.byref(pairs), None,
                                             ctypes.byref(ms))
        assert rc == 2 and b"build is NULL" in L.hwbrj_last_error()
        assert (n.value, pairs.value, ms.value) == (UNWRITTEN, UNWRITTEN, -7.0)
    assert L.hwbrj_build_group_reset(None, agg) == 2 and b"build is NULL" in L.hwbrj_last_error()


def _cols(n=8):
    import torch
    return torch.zeros(n, dtype=torch.int32), torch.zeros(n, dtype=torch.int32)


def test_wrappers_refuse_a_freed_build(hw):
    import torch
    b = hw.Build(0, torch.device("cuda:0"))
    Sk, Sv = _cols()
    with pytest.raises(ValueError, match="freed"):
        hw.group_accum_probe_keys_device(b, Sk, Sv)
    with pytest.raises(ValueError, match="freed"):
        b.group_rows()
    with pytest.raises(ValueError, match="freed"):
        b.reset_group(hw.AGG_MINMAX)
    with pytest.raises(ValueError, match="must be a Build"):
        hw.group_accum_probe_keys_device(None, Sk, Sv)


def test_wrapper_refuses_columns_on_another_device(hw, monkeypatch):
    """A live handle on cuda:1 and columns elsewhere: refused by the wrapper, before the library sees the
    handle (the library here answers hwbrj_set_device only)."""
    import torch
    fake = types.SimpleNamespace(hwbrj_set_device=lambda i: 0)
    monkeypatch.setattr(hw, "lib", lambda: fake)
    b = hw.Build(0x1234, torch.device("cuda:1"))
    try:
        Sk, Sv = _cols()
        with pytest.raises(ValueError, match="but the build is on cuda:1"):
            hw.group_accum_probe_keys_device(b, Sk, Sv, hw.AGG_MINMAX)
    finally:
        b._h = 0  # (never a real handle: nothing to free)


def test_wrapper_refuses_bad_bitmaps(hw):
    """_group_probe's checks, which come before the build is looked at."""
    import torch
    b = hw.Build(0, torch.device("cuda:0"))
    Sk, Sv = _cols(40)
    for name in ("s_valid", "sv_valid"):
        with pytest.raises(ValueError, match=f"{name} must be a torch.uint8 bitmap"):
            hw.group_accum_probe_keys_device(b, Sk, Sv, **{name: torch.zeros(5, dtype=torch.int32)})
        with pytest.raises(ValueError, match=f"{name} has 4 bytes, 40 keys need 5"):
            hw.group_accum_probe_keys_device(b, Sk, Sv, **{name: torch.zeros(4, dtype=torch.uint8)})
        with pytest.raises(ValueError, match=f"{name} has 39 entries for 40 keys"):
            hw.group_accum_probe_keys_device(b, Sk, Sv, **{name: torch.ones(39, dtype=torch.bool)})
        with pytest.raises(ValueError, match=f"{name} must be a contiguous 1-D tensor"):
            hw.group_accum_probe_keys_device(b, Sk, Sv, **{name: torch.zeros((5, 2), dtype=torch.uint8)})
