"""The row-index joins on key columns (hwbrj_join_keys_pairs_device, hwbrj_join_keys_semi_device,
hwbrj_join_keys_outer_device, include/hwbrj.h): the exports, the Python wrappers, and every refusal
that is decided before any device call, tested with pointers that are never dereferenced. No GPU."""
import ctypes

import pytest

ALIGNED, MISALIGNED, OUT = 0x1000, 0x1004, 0x2000
UNWRITTEN = 0x5A5A5A5A5A5A5A5A
ENTRIES = ["pairs", "semi", "outer"]


def _call(hw, entry, pr, nR, ps, nS, out=None, cap=0, kind=0, args=None):
    """(return code, *n_out after the call) of one C entry; *n_out starts as UNWRITTEN."""
    L = hw.lib()
    n = ctypes.c_uint64(UNWRITTEN)
    a = ctypes.byref(args) if args is not None else None
    if entry == "pairs":
        rc = L.hwbrj_join_keys_pairs_device(pr, nR, ps, nS, a, out, cap, ctypes.byref(n), None, None, None)
    elif entry == "semi":
        rc = L.hwbrj_join_keys_semi_device(pr, nR, ps, nS, a, kind, out, cap, ctypes.byref(n), None, None, None)
    else:
        rc = L.hwbrj_join_keys_outer_device(pr, nR, ps, nS, a, kind, out, cap, ctypes.byref(n), None, None, None,
                                            None)
    return rc, n.value


def test_library_exports_row_index_joins(hw):
    for name in ("hwbrj_join_keys_pairs_device", "hwbrj_join_keys_semi_device", "hwbrj_join_keys_outer_device"):
        assert hasattr(hw.lib(), name)


def test_python_interface(hw):
    for name in ("join_keys_pairs_device", "semi_join_keys_device", "outer_join_keys_device"):
        assert callable(getattr(hw, name))
        assert name in hw.__all__


@pytest.mark.parametrize("side", ["R", "S"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_misaligned_column_is_refused_without_a_device(hw, entry, side):
    """One side at 0x1004 (n = 4), the other aligned: code 2, a message saying align, *n_out kept."""
    pr, ps = (MISALIGNED, ALIGNED) if side == "R" else (ALIGNED, MISALIGNED)
    rc, n = _call(hw, entry, pr, 4, ps, 4)
    assert rc == 2
    assert b"align" in hw.lib().hwbrj_last_error()
    assert n == UNWRITTEN


@pytest.mark.parametrize("entry", ENTRIES)
def test_empty_column_is_not_refused_for_alignment(hw, entry):
    """n = 0 on both sides with misaligned pointers passes the alignment check. The call still ends
    before any kernel: m = 3 is no filter size (code 2, naming m), or there is no device (code 10)."""
    bad = hw._BloomArgs(hw.BLOCKED, 3, 1, 1024)
    rc, _ = _call(hw, entry, MISALIGNED, 0, MISALIGNED, 0, args=bad)
    assert rc in (2, 10)
    assert b"align" not in hw.lib().hwbrj_last_error()


@pytest.mark.parametrize("side", ["R", "S"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_2_pow_31_rows_are_refused_without_a_device(hw, entry, side):
    """A row index is an int32: 2^31 rows on either side give 3 and a message naming that side;
    2^31 - 1 rows pass this check (and end at the missing device, or at m = 3)."""
    nR, nS = (1 << 31, 4) if side == "R" else (4, 1 << 31)
    rc, n = _call(hw, entry, ALIGNED, nR, ALIGNED, nS)
    assert rc == 3
    msg = hw.lib().hwbrj_last_error()
    assert b"key column " + side.encode() in msg and b"2^31" in msg
    assert n == UNWRITTEN
    bad = hw._BloomArgs(hw.BLOCKED, 3, 1, 1024)
    rc, _ = _call(hw, entry, ALIGNED, min(nR, (1 << 31) - 1), ALIGNED, min(nS, (1 << 31) - 1), args=bad)
    assert rc in (2, 10)
    assert b"2^31" not in hw.lib().hwbrj_last_error()


@pytest.mark.parametrize("entry", ["semi", "outer"])
def test_unknown_kind_is_refused_without_a_device(hw, entry):
    for kind in (-1, 3, 99):
        rc, n = _call(hw, entry, ALIGNED, 4, ALIGNED, 4, out=OUT, cap=8, kind=kind)
        assert rc == 2
        assert b"kind" in hw.lib().hwbrj_last_error()
        assert n == UNWRITTEN


@pytest.mark.parametrize("entry", ENTRIES)
def test_capacity_without_an_output_is_refused_without_a_device(hw, entry):
    rc, n = _call(hw, entry, ALIGNED, 4, ALIGNED, 4, out=None, cap=8)
    assert rc == 2
    assert b"d_out" in hw.lib().hwbrj_last_error()
    assert n == UNWRITTEN


@pytest.mark.parametrize("name", ["join_keys_pairs_device", "semi_join_keys_device", "outer_join_keys_device"])
def test_wrappers_refuse_what_is_no_key_column(hw, name):
    """_check_keys' ValueErrors, raised before the library is called: a strided view, an int64
    tensor and a CPU tensor (every tensor here is on the CPU, so each case is refused for that
    alone as well; the GPU file checks the same cases with device tensors)."""
    import torch
    fn = getattr(hw, name)
    T = torch.zeros((8, 2), dtype=torch.int32)
    good = torch.zeros(8, dtype=torch.int32)
    for bad in (T[:, 0], torch.zeros(8, dtype=torch.int64), good):
        with pytest.raises(ValueError):
            fn(bad, good)
        with pytest.raises(ValueError):
            fn(good, bad)
