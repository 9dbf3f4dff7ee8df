"""The group joins on key columns with an S value column (hwbrj_join_keys_group_device,
hwbrj_join_keys_group_minmax_device, include/hwbrj.h): the exports, the Python wrappers, and every
refusal that is decided before any device call, tested with pointers that are never dereferenced.
No GPU."""
import ctypes

import pytest

ALIGNED, MISALIGNED, OUT = 0x1000, 0x1004, 0x2000
UNWRITTEN = 0x5A5A5A5A5A5A5A5A
ENTRIES = ["hwbrj_join_keys_group_device", "hwbrj_join_keys_group_minmax_device"]
WRAPPERS = ["group_join_keys_device", "group_minmax_join_keys_device"]


def _call(hw, entry, pr, nR, ps, pv, nS, out=None, cap=0, kind=0, args=None):
    """(return code, *n_out after the call) of one C entry; *n_out starts as UNWRITTEN."""
    n = ctypes.c_uint64(UNWRITTEN)
    a = ctypes.byref(args) if args is not None else None
    rc = getattr(hw.lib(), entry)(pr, nR, ps, pv, nS, a, kind, out, cap, ctypes.byref(n), None, None, None, None)
    return rc, n.value


def _bad_filter(hw):
    """m = 3 is no filter size: a call that passes every early refusal still ends before any kernel
    (code 2 naming m, or 10 without a device)."""
    return hw._BloomArgs(hw.BLOCKED, 3, 1, 1024)


def test_library_exports_group_joins_on_key_columns(hw):
    for name in ENTRIES:
        assert hasattr(hw.lib(), name)


def test_python_interface(hw):
    for name in WRAPPERS:
        assert callable(getattr(hw, name))
        assert name in hw.__all__


@pytest.mark.parametrize("column", ["Rkeys", "Skeys", "Svals"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_misaligned_column_is_refused_without_a_device(hw, entry, column):
    """One column of the three at 0x1004 (n = 4), the others aligned: code 2, a message saying align,
    *n_out kept."""
    p = {c: MISALIGNED if c == column else ALIGNED for c in ("Rkeys", "Skeys", "Svals")}
    rc, n = _call(hw, entry, p["Rkeys"], 4, p["Skeys"], p["Svals"], 4)
    assert rc == 2
    assert b"align" in hw.lib().hwbrj_last_error()
    assert n == UNWRITTEN


@pytest.mark.parametrize("entry", ENTRIES)
def test_empty_column_is_not_refused_for_alignment(hw, entry):
    """n = 0 on both sides with three misaligned pointers passes the alignment check, and so does an
    empty S with no value column at all."""
    for pv in (MISALIGNED, None):
        rc, _ = _call(hw, entry, MISALIGNED, 0, MISALIGNED, pv, 0, args=_bad_filter(hw))
        assert rc in (2, 10)
        msg = hw.lib().hwbrj_last_error()
        assert b"align" not in msg and b"d_Svals" not in msg


@pytest.mark.parametrize("entry", ENTRIES)
def test_2_pow_31_r_rows_are_refused_without_a_device(hw, entry):
    """r_payload is the R row index, an int32: 2^31 R rows give 3 and a message naming R; 2^31 - 1
    pass this check."""
    rc, n = _call(hw, entry, ALIGNED, 1 << 31, ALIGNED, ALIGNED, 4)
    assert rc == 3
    msg = hw.lib().hwbrj_last_error()
    assert b"key column R" in msg and b"2^31" in msg
    assert n == UNWRITTEN
    rc, _ = _call(hw, entry, ALIGNED, (1 << 31) - 1, ALIGNED, ALIGNED, 4, args=_bad_filter(hw))
    assert rc in (2, 10)
    assert b"2^31" not in hw.lib().hwbrj_last_error()


@pytest.mark.parametrize("entry", ENTRIES)
def test_2_pow_32_s_rows_are_refused_without_a_device(hw, entry):
    """The group join's own rule (32-bit counts): 2^32 S rows give 3. S row indices are never
    produced, so 2^31 S rows, and 2^32 - 1, pass."""
    rc, n = _call(hw, entry, ALIGNED, 4, ALIGNED, ALIGNED, 1 << 32)
    assert rc == 3
    assert b"2^32" in hw.lib().hwbrj_last_error()
    assert n == UNWRITTEN
    for nS in (1 << 31, (1 << 32) - 1):
        rc, _ = _call(hw, entry, ALIGNED, 4, ALIGNED, ALIGNED, nS, args=_bad_filter(hw))
        assert rc in (2, 10)
        msg = hw.lib().hwbrj_last_error()
        assert b"2^31" not in msg and b"2^32" not in msg


@pytest.mark.parametrize("entry", ENTRIES)
def test_missing_value_column_is_refused_without_a_device(hw, entry):
    rc, n = _call(hw, entry, ALIGNED, 4, ALIGNED, None, 4, out=OUT, cap=8)
    assert rc == 2
    assert b"d_Svals" in hw.lib().hwbrj_last_error()
    assert n == UNWRITTEN


@pytest.mark.parametrize("entry", ENTRIES)
def test_unknown_kind_is_refused_without_a_device(hw, entry):
    for kind in (-1, 2, 99):
        rc, n = _call(hw, entry, ALIGNED, 4, ALIGNED, ALIGNED, 4, out=OUT, cap=8, kind=kind)
        assert rc == 2
        assert b"kind" in hw.lib().hwbrj_last_error()
        assert n == UNWRITTEN


@pytest.mark.parametrize("entry", ENTRIES)
def test_capacity_without_an_output_is_refused_without_a_device(hw, entry):
    rc, n = _call(hw, entry, ALIGNED, 4, ALIGNED, ALIGNED, 4, out=None, cap=8)
    assert rc == 2
    assert b"d_out" in hw.lib().hwbrj_last_error()
    assert n == UNWRITTEN


@pytest.mark.parametrize("entry", ENTRIES)
def test_misaligned_output_is_refused_without_a_device(hw, entry):
    rc, n = _call(hw, entry, ALIGNED, 4, ALIGNED, ALIGNED, 4, out=OUT + 8, cap=8)
    assert rc == 2
    assert b"d_out" in hw.lib().hwbrj_last_error() and b"align" in hw.lib().hwbrj_last_error()
    assert n == UNWRITTEN


@pytest.mark.parametrize("name", WRAPPERS)
def test_wrappers_refuse_what_is_no_column(hw, name):
    """_check_keys' ValueErrors, raised before the library is called: an int64 tensor, a 2-D tensor
    and a strided view in each of the three places, and a value column of another length than Sk
    (every tensor here is on the CPU, so each case is refused for that alone as well; the GPU file
    checks the same cases with device tensors)."""
    import torch
    fn = getattr(hw, name)
    T = torch.zeros((8, 2), dtype=torch.int32)
    good = torch.zeros(8, dtype=torch.int32)
    for bad in (torch.zeros(8, dtype=torch.int64), T, T[:, 0], good):
        for cols in ((bad, good, good), (good, bad, good), (good, good, bad)):
            with pytest.raises(ValueError):
                fn(*cols)
    with pytest.raises(ValueError):
        fn(good, good, torch.zeros(12, dtype=torch.int32))
    with pytest.raises(TypeError):
        fn(good, good)  # (the value column is not optional)
