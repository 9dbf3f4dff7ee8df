"""The outer joins' interface (hwbrj_join_outer_device, include/hwbrj.h): the export, the Python
wrapper and its constants, and the argument check that is decided before any device call. Also, on
the CPU, that the relations of tests/test_gpu_outer.py::test_every_mode have false-positive survivors
under every filter it lists (the oracle's counting join). No GPU."""
import ctypes

import numpy as np
import pytest


def test_library_exports_outer_join(hw):
    assert hasattr(hw.lib(), "hwbrj_join_outer_device")


def test_python_interface(hw):
    assert callable(hw.outer_join_device)
    assert (hw.OUTER_S, hw.OUTER_R, hw.OUTER_FULL) == (0, 1, 2)
    for name in ("outer_join_device", "OUTER_S", "OUTER_R", "OUTER_FULL"):
        assert name in hw.__all__


def test_unknown_kind_is_refused_without_a_device(hw):
    """kind = 7: return code 2 and a message naming kind, with no relation and no GPU."""
    n = ctypes.c_uint64(123)
    rc = hw.lib().hwbrj_join_outer_device(None, 0, None, 0, None, 7, -1, None, 0, ctypes.byref(n), None, None,
                                          None, None)
    assert rc == 2
    assert b"kind" in hw.lib().hwbrj_last_error()
    assert n.value == 123  # (nothing was written)


def test_every_mode_relations_have_false_positives(hw, orc):
    """filtered > the S rows with a partner, for every filter of test_every_mode and its seed; and
    the three classes have at least 1,000 rows each."""
    import test_gpu_outer as t
    R, S = t.mode_relations(orc)
    assert R[:, 0].max() <= 40000 and S.shape[0] == 300000
    mask = np.isin(S[:, 0], R[:, 0])
    partnered = int(mask.sum())
    assert partnered >= 1000 and int((~mask).sum()) >= 1000
    assert int((~np.isin(R[:, 0], S[:, 0])).sum()) >= 1000
    assert np.unique(S[mask, 0]).size <= 30000
    for name, a in t._args(hw).items():
        if a is None:
            continue
        c = a._c()
        _, filtered, _ = orc.bpro(R, S, 8, c.variant, c.m, c.k, c.B, True)
        print(name, filtered, partnered)
        assert filtered > partnered, name
