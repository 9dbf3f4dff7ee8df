"""The group join's interface (hwbrj_join_group_device, include/hwbrj.h): the export, the Python
wrapper, its constants and its mirror of hwbrj_group_row_t, and the argument check that is decided
before any device call. Also, on the CPU, that the numpy reference of tests/test_gpu_group.py agrees
with the oracle's pairs: the sum of its counts is the number of pairs, and so are its sums. No GPU."""
import ctypes

import numpy as np


def test_library_exports_group_join(hw):
    assert hasattr(hw.lib(), "hwbrj_join_group_device")


def test_python_interface(hw):
    assert callable(hw.group_join_device)
    assert (hw.GROUP_MATCHED, hw.GROUP_ALL) == (0, 1)
    for name in ("group_join_device", "GROUP_MATCHED", "GROUP_ALL", "GroupRows"):
        assert name in hw.__all__
    assert hw.GroupRows._fields == ("r_payload", "count", "sum", "raw")


def test_row_layout(hw):
    """hwbrj_group_row_t: 16 bytes, r_payload at 0, count at 4, sum at 8."""
    row = hw._GroupRow
    assert ctypes.sizeof(row) == 16
    assert (row.r_payload.offset, row.count.offset, row.sum.offset) == (0, 4, 8)
    assert (row.r_payload.size, row.count.size, row.sum.size) == (4, 4, 8)


def test_unknown_kind_is_refused_without_a_device(hw):
    """kind = 7: return code 2 and a message naming kind, with no relation and no GPU."""
    n = ctypes.c_uint64(123)
    rc = hw.lib().hwbrj_join_group_device(None, 0, None, 0, None, 7, None, 0, ctypes.byref(n), None, None, None, None)
    assert rc == 2
    assert b"kind" in hw.lib().hwbrj_last_error()
    assert n.value == 123  # (nothing was written)


def _pinned(orc, ref, R, S):
    """reference(R, S) against orc.join_pairs: the counts add up to the pairs, and every R row's
    count and sum are those of the pairs that carry its payload (R payloads are distinct)."""
    pairs = np.asarray(orc.join_pairs(R, S), dtype=np.int32).reshape(-1, 2)
    assert int(ref[:, 1].sum()) == pairs.shape[0]
    assert ref.shape == (R.shape[0], 3) and np.array_equal(ref[:, 0], R[:, 1].astype(np.int64))
    order = np.argsort(ref[:, 0])
    i = order[np.searchsorted(ref[order, 0], pairs[:, 0].astype(np.int64))]
    assert np.array_equal(ref[i, 0], pairs[:, 0].astype(np.int64))
    cnt, sm = np.zeros(R.shape[0], dtype=np.int64), np.zeros(R.shape[0], dtype=np.int64)
    np.add.at(cnt, i, 1)
    np.add.at(sm, i, pairs[:, 1].astype(np.int64))
    assert np.array_equal(ref[:, 1], cnt) and np.array_equal(ref[:, 2], sm)
    return pairs.shape[0]


def test_reference_is_pinned_to_the_oracle(orc):
    import test_gpu_group as g
    import test_gpu_outer as t
    R, S = t.mode_relations(orc)  # (case 1 of tests/test_gpu_group.py, seed 5)
    assert np.unique(R[:, 1]).size == R.shape[0]
    assert _pinned(orc, g.reference(R, S), R, S) >= 60000
    # duplicate keys on both sides, the extreme keys and payloads, keys without a partner
    rng = np.random.default_rng(3)
    keys = np.array([2**31 - 1, -2**31, 0, -1, 5, 6, 7, 8], dtype=np.int64)
    R = t._rel(np.repeat(keys, 3), rng)
    Sk = np.concatenate([np.repeat(keys[:6], [4, 3, 2, 1, 5, 1]), [100, 101, 100]])
    S = t._rel(Sk, rng)
    S[:4, 1] = [2**31 - 1, 2**31 - 1, -2**31, -2**31]
    ref = g.reference(R, S)
    assert _pinned(orc, ref, R, S) == 3 * 16
    assert int((ref[:, 1] == 0).sum()) == 6
    assert g.reference(R[:0], S).shape == (0, 3) and not g.reference(R, S[:0])[:, 1:].any()
