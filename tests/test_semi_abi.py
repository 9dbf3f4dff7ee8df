"""The existence joins' interface (hwbrj_join_semi_device, include/hwbrj.h): the export, the Python
wrapper and its constants, and the argument check that is decided before any device call. No GPU."""
import ctypes


def test_library_exports_semi_join(hw):
    assert hasattr(hw.lib(), "hwbrj_join_semi_device")


def test_python_interface(hw):
    assert callable(hw.semi_join_device)
    assert (hw.JOIN_SEMI, hw.JOIN_ANTI) == (0, 1)
    for name in ("semi_join_device", "JOIN_SEMI", "JOIN_ANTI"):
        assert name in hw.__all__


def test_unknown_kind_is_refused_without_a_device(hw):
    """kind = 5: return code 2 and a message, with no relation and no GPU."""
    n = ctypes.c_uint64(123)
    rc = hw.lib().hwbrj_join_semi_device(None, 0, None, 0, None, 5, None, 0, ctypes.byref(n), None, None, None)
    assert rc == 2
    assert b"kind" in hw.lib().hwbrj_last_error()
    assert n.value == 123  # (nothing was written)
