"""The min/max group join's interface (hwbrj_join_group_minmax_device, include/hwbrj.h): the export,
the Python wrapper and its mirror of hwbrj_group_minmax_row_t, and the argument check that is decided
before any device call. Also, on the CPU, that the numpy reference of tests/test_gpu_group_minmax.py
agrees with the oracle's pairs: per R row the count, the smallest and the largest S payload of the
pairs that carry its payload, and the identities INT32_MAX / INT32_MIN where there is none. No GPU."""
import ctypes

import numpy as np

INT_MAX, INT_MIN = 2**31 - 1, -2**31


def test_library_exports_group_minmax_join(hw):
    assert hasattr(hw.lib(), "hwbrj_join_group_minmax_device")


def test_python_interface(hw):
    assert callable(hw.group_minmax_join_device)
    for name in ("group_minmax_join_device", "GroupMinMaxRows", "GROUP_MATCHED", "GROUP_ALL"):
        assert name in hw.__all__
    assert hw.GroupMinMaxRows._fields == ("r_payload", "count", "min", "max", "raw")


def test_row_layout(hw):
    """hwbrj_group_minmax_row_t: 16 bytes, r_payload at 0, count at 4, min at 8, max at 12."""
    row = hw._GroupMinMaxRow
    assert ctypes.sizeof(row) == 16
    assert (row.r_payload.offset, row.count.offset, row.min.offset, row.max.offset) == (0, 4, 8, 12)
    assert (row.r_payload.size, row.count.size, row.min.size, row.max.size) == (4, 4, 4, 4)
    r = row(-1, 2**32 - 1, INT_MIN, INT_MAX)  # (count unsigned, the others signed)
    assert (r.r_payload, r.count, r.min, r.max) == (-1, 2**32 - 1, INT_MIN, INT_MAX)


def test_unknown_kind_is_refused_without_a_device(hw):
    """kind = 7: return code 2 and a message naming kind, with no relation and no GPU."""
    n = ctypes.c_uint64(123)
    rc = hw.lib().hwbrj_join_group_minmax_device(None, 0, None, 0, None, 7, None, 0, ctypes.byref(n), None, None, None,
                                                 None)
    assert rc == 2
    assert b"kind" in hw.lib().hwbrj_last_error()
    assert n.value == 123  # (nothing was written)


def _pinned(orc, ref, R, S):
    """reference(R, S) against orc.join_pairs: every R row's count, min and max are those of the
    pairs that carry its payload (R payloads are distinct), the identities where it has no pair."""
    pairs = np.asarray(orc.join_pairs(R, S), dtype=np.int32).reshape(-1, 2)
    assert int(ref[:, 1].sum()) == pairs.shape[0]
    assert ref.shape == (R.shape[0], 4) and np.array_equal(ref[:, 0], R[:, 1].astype(np.int64))
    order = np.argsort(ref[:, 0])
    i = order[np.searchsorted(ref[order, 0], pairs[:, 0].astype(np.int64))]
    assert np.array_equal(ref[i, 0], pairs[:, 0].astype(np.int64))
    cnt = np.zeros(R.shape[0], dtype=np.int64)
    mn, mx = np.full(R.shape[0], INT_MAX, dtype=np.int64), np.full(R.shape[0], INT_MIN, dtype=np.int64)
    np.add.at(cnt, i, 1)
    np.minimum.at(mn, i, pairs[:, 1].astype(np.int64))
    np.maximum.at(mx, i, pairs[:, 1].astype(np.int64))
    assert np.array_equal(ref[:, 1], cnt) and np.array_equal(ref[:, 2], mn) and np.array_equal(ref[:, 3], mx)
    lone = ref[:, 1] == 0
    assert (ref[lone, 2] == INT_MAX).all() and (ref[lone, 3] == INT_MIN).all()
    assert (ref[~lone, 2] <= ref[~lone, 3]).all()
    return pairs.shape[0]


def test_reference_is_pinned_to_the_oracle(orc):
    import test_gpu_group_minmax as g
    import test_gpu_outer as t
    R, S = t.mode_relations(orc)  # (case 1 of tests/test_gpu_group_minmax.py, seed 5)
    assert np.unique(R[:, 1]).size == R.shape[0]
    assert _pinned(orc, g.reference(R, S), R, S) >= 60000
    # duplicate keys on both sides, the extreme keys and payloads, keys without a partner
    rng = np.random.default_rng(3)
    keys = np.array([2**31 - 1, -2**31, 0, -1, 5, 6, 7, 8], dtype=np.int64)
    R = t._rel(np.repeat(keys, 3), rng)
    Sk = np.concatenate([np.repeat(keys[:6], [4, 3, 2, 1, 5, 1]), [100, 101, 100]])
    S = t._rel(Sk, rng)
    S[:4, 1] = [INT_MAX, 1, -1, INT_MIN]  # key INT_MAX: both extremes
    S[7:9, 1] = [-1, 1]                   # key 0: exactly {-1, 1}
    S[4:7, 1] = [-5, INT_MIN, -7]         # key INT_MIN: all negative
    ref = g.reference(R, S)
    assert _pinned(orc, ref, R, S) == 3 * 16
    assert int((ref[:, 1] == 0).sum()) == 6
    by_key = {int(k): ref[np.isin(ref[:, 0], R[R[:, 0] == np.int32(k), 1])] for k in keys}
    assert (by_key[INT_MAX][:, 1:] == [4, INT_MIN, INT_MAX]).all() and by_key[INT_MAX].shape[0] == 3
    assert (by_key[0][:, 1:] == [2, -1, 1]).all()
    assert (by_key[INT_MIN][:, 1:] == [3, INT_MIN, -5]).all()
    assert (by_key[-1][:, 1] == 1).all() and (by_key[-1][:, 2] == by_key[-1][:, 3]).all()
    assert (by_key[7][:, 1:] == [0, INT_MAX, INT_MIN]).all()
    assert g.reference(R[:0], S).shape == (0, 4)
    assert (g.reference(R, S[:0])[:, 1:] == [0, INT_MAX, INT_MIN]).all()
