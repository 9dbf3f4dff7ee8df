"""The key-column counting join's interface (hwbrj_join_keys_device / _async, include/hwbrj.h): the
exports, the Python wrappers, and the alignment check, which is decided before any device call, so
it is tested here with pointers that are never dereferenced. No GPU."""
import ctypes

import pytest

ALIGNED, MISALIGNED = 0x1000, 0x1004
PATTERN = 0x5A


def _filled_stats(hw):
    st = hw._Stats()
    ctypes.memset(ctypes.byref(st), PATTERN, ctypes.sizeof(st))
    return st


def _untouched(st):
    return bytes(st) == bytes([PATTERN]) * ctypes.sizeof(st)


def test_library_exports_key_column_joins(hw):
    assert hasattr(hw.lib(), "hwbrj_join_keys_device")
    assert hasattr(hw.lib(), "hwbrj_join_keys_device_async")


def test_python_interface(hw):
    for name in ("join_keys_device", "join_keys_device_async"):
        assert callable(getattr(hw, name))
        assert name in hw.__all__


@pytest.mark.parametrize("side", ["R", "S"])
def test_misaligned_column_is_refused_without_a_device(hw, side):
    """One side at 0x1004 (n = 4), the other aligned: code 2, a message saying align, and the stats
    struct keeps its pattern."""
    pr, ps = (MISALIGNED, ALIGNED) if side == "R" else (ALIGNED, MISALIGNED)
    st = _filled_stats(hw)
    rc = hw.lib().hwbrj_join_keys_device(pr, 4, ps, 4, None, hw.ALGO_PRO, None, ctypes.byref(st))
    assert rc == 2
    assert b"align" in hw.lib().hwbrj_last_error()
    assert _untouched(st)


@pytest.mark.parametrize("side", ["R", "S"])
def test_misaligned_column_is_refused_async(hw, side):
    pr, ps = (MISALIGNED, ALIGNED) if side == "R" else (ALIGNED, MISALIGNED)
    rc = hw.lib().hwbrj_join_keys_device_async(pr, 4, ps, 4, None, None)
    assert rc == 2
    assert b"align" in hw.lib().hwbrj_last_error()


def test_empty_column_is_not_refused_for_alignment(hw):
    """n = 0 on both sides with misaligned pointers passes the alignment check. The call still ends
    before any kernel: m = 3 is no filter size (code 2, naming m), or there is no device (code 10)."""
    bad = hw._BloomArgs(hw.BLOCKED, 3, 1, 1024)
    st = _filled_stats(hw)
    rc = hw.lib().hwbrj_join_keys_device(MISALIGNED, 0, MISALIGNED, 0, ctypes.byref(bad), hw.ALGO_PRO, None,
                                         ctypes.byref(st))
    assert rc in (2, 10)
    assert b"align" not in hw.lib().hwbrj_last_error()
    rc = hw.lib().hwbrj_join_keys_device_async(MISALIGNED, 0, MISALIGNED, 0, ctypes.byref(bad), None)
    assert rc in (2, 10)
    assert b"align" not in hw.lib().hwbrj_last_error()
