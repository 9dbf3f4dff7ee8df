"""Key columns with validity bitmaps (hwbrj_join_keys_nulls_device, hwbrj_join_keys_pairs_nulls_device,
hwbrj_join_keys_semi_nulls_device, hwbrj_join_keys_outer_nulls_device, include/hwbrj.h): the exports,
the wrappers' keywords, pack_validity, and every refusal that is decided before any device call,
tested with pointers that are never dereferenced. No GPU."""
import ctypes
import inspect

import numpy as np
import pytest

KEYS, KEYS_BAD, VALID, OUT = 0x1000, 0x1004, 0x3000, 0x2000
UNWRITTEN = 0x5A5A5A5A5A5A5A5A
ENTRIES = ["count", "pairs", "semi", "outer"]
WRAPPERS = ["join_keys_device", "join_keys_pairs_device", "semi_join_keys_device", "outer_join_keys_device"]


def _call(hw, entry, pr, vr, nR, ps, vs, nS, out=None, cap=0, kind=0, args=None, algorithm=0):
    """(return code, *n_out after the call, *stats' bytes after the call) of one C entry; *n_out starts
    as UNWRITTEN and *stats as 0x5A bytes (the counting entry has no n_out)."""
    L = hw.lib()
    n = ctypes.c_uint64(UNWRITTEN)
    st = hw._Stats()
    ctypes.memset(ctypes.byref(st), 0x5A, ctypes.sizeof(st))
    a = ctypes.byref(args) if args is not None else None
    if entry == "count":
        rc = L.hwbrj_join_keys_nulls_device(pr, vr, nR, ps, vs, nS, a, algorithm, None, ctypes.byref(st))
    elif entry == "pairs":
        rc = L.hwbrj_join_keys_pairs_nulls_device(pr, vr, nR, ps, vs, nS, a, out, cap, ctypes.byref(n), None,
                                                  ctypes.byref(st), None)
    elif entry == "semi":
        rc = L.hwbrj_join_keys_semi_nulls_device(pr, vr, nR, ps, vs, nS, a, kind, out, cap, ctypes.byref(n), None,
                                                 ctypes.byref(st), None)
    else:
        rc = L.hwbrj_join_keys_outer_nulls_device(pr, vr, nR, ps, vs, nS, a, kind, out, cap, ctypes.byref(n), None, None,
                                                  ctypes.byref(st), None)
    return rc, n.value, bytes(st)


def _unwritten(hw, n, st):
    return n == UNWRITTEN and st == b"\x5a" * ctypes.sizeof(hw._Stats)


def _past_the_bitmap_checks(hw, entry, vr, vs, args):
    """A call that gets past the bitmaps' checks and still ends before any kernel, with or without a
    device: an unknown kind (semi, outer: 2), a capacity without d_out (pairs: 2), an unknown
    algorithm (count: 2 from the engine, or 10 where there is no device). Returns (rc, message)."""
    rc, _, _ = _call(hw, entry, KEYS, vr, 40, KEYS, vs, 40, out=None, cap=8, kind=99, args=args, algorithm=99)
    msg = hw.lib().hwbrj_last_error()
    assert rc in ((2, 10) if entry == "count" else (2,))
    if rc == 2:
        assert {"count": b"algorithm", "pairs": b"d_out", "semi": b"kind", "outer": b"kind"}[entry] in msg
    return rc, msg


def test_library_exports_the_nulls_entries(hw):
    for name in ("hwbrj_join_keys_nulls_device", "hwbrj_join_keys_pairs_nulls_device",
                 "hwbrj_join_keys_semi_nulls_device", "hwbrj_join_keys_outer_nulls_device"):
        assert hasattr(hw.lib(), name)


def test_wrappers_take_the_keywords(hw):
    for name in WRAPPERS:
        p = inspect.signature(getattr(hw, name)).parameters
        for kw in ("r_valid", "s_valid"):
            assert p[kw].kind is inspect.Parameter.KEYWORD_ONLY and p[kw].default is None
    assert callable(hw.pack_validity) and "pack_validity" in hw.__all__


@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("side", ["R", "S"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_misaligned_bitmap_is_refused_without_a_device(hw, entry, side, off):
    """One bitmap at an address = 1, 2 or 3 (mod 4), everything else in order: 2, "align", nothing
    written."""
    vr, vs = (VALID + off, VALID) if side == "R" else (None, VALID + off)
    rc, n, st = _call(hw, entry, KEYS, vr, 40, KEYS, vs, 40, out=OUT, cap=8)
    assert rc == 2
    assert b"align" in hw.lib().hwbrj_last_error() and b"bitmap" in hw.lib().hwbrj_last_error()
    assert _unwritten(hw, n, st)


@pytest.mark.parametrize("entry", ENTRIES)
def test_misaligned_bitmap_of_an_empty_column_is_not_refused(hw, entry):
    """n = 0 on both sides with bitmaps at odd addresses passes the alignment check. The call still
    ends before any kernel: m = 3 is no filter size (2, naming m), or there is no device (10)."""
    bad = hw._BloomArgs(hw.BLOCKED, 3, 1, 1024)
    rc, _, _ = _call(hw, entry, KEYS, VALID + 1, 0, KEYS, VALID + 3, 0, args=bad)
    assert rc in (2, 10)
    assert b"align" not in hw.lib().hwbrj_last_error()


def _unsupported(hw):
    return {"global_b4": hw._BloomArgs(hw.BLOCKED, 1 << 20, 1, 4), "basic_k3": hw._BloomArgs(hw.BASIC, 1 << 22, 3, 0),
            "basic_k0": hw._BloomArgs(hw.BASIC, 1 << 22, 0, 0)}


@pytest.mark.parametrize("which", ["R", "S", "both"])
@pytest.mark.parametrize("cfg", ["global_b4", "basic_k3", "basic_k0"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_unsupported_filter_with_a_bitmap_gives_9(hw, entry, cfg, which):
    vr = VALID if which != "S" else None
    vs = VALID if which != "R" else None
    rc, n, st = _call(hw, entry, KEYS, vr, 40, KEYS, vs, 40, out=OUT, cap=8, args=_unsupported(hw)[cfg])
    assert rc == 9
    assert b"bitmap" in hw.lib().hwbrj_last_error()
    assert _unwritten(hw, n, st)


@pytest.mark.parametrize("cfg", ["global_b4", "basic_k3", "basic_k0"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_unsupported_filter_without_bitmaps_is_the_counterparts_business(hw, entry, cfg):
    """Both bitmaps NULL: not 9, the call goes on to the counterpart's own checks."""
    rc, msg = _past_the_bitmap_checks(hw, entry, None, None, _unsupported(hw)[cfg])
    assert rc != 9 and b"bitmap" not in msg


@pytest.mark.parametrize("cfg", [None, "blocked", "sectorized", "basic_k1"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_supported_filters_pass_the_bitmap_checks(hw, entry, cfg):
    """The partition-slice configurations and no filter get past both checks with aligned bitmaps."""
    args = {None: None, "blocked": hw._BloomArgs(hw.BLOCKED, 1 << 24, 1, 1024),
            "sectorized": hw._BloomArgs(hw.SECTORIZED, 1 << 24, 2, 1024), "basic_k1": hw._BloomArgs(hw.BASIC, 1 << 24, 1, 0)}[cfg]
    rc, msg = _past_the_bitmap_checks(hw, entry, VALID, VALID, args)
    assert rc != 9 and b"bitmap" not in msg


@pytest.mark.parametrize("side", ["R", "S"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_counterparts_key_alignment_still_comes_first(hw, entry, side):
    pr, ps = (KEYS_BAD, KEYS) if side == "R" else (KEYS, KEYS_BAD)
    rc, n, st = _call(hw, entry, pr, VALID, 4, ps, VALID, 4)
    assert rc == 2
    msg = hw.lib().hwbrj_last_error()
    assert b"align" in msg and b"key column " + side.encode() in msg
    assert _unwritten(hw, n, st)


@pytest.mark.parametrize("side", ["R", "S"])
@pytest.mark.parametrize("entry", ["pairs", "semi", "outer"])
def test_2_pow_31_rows_are_refused_naming_the_side(hw, entry, side):
    nR, nS = (1 << 31, 4) if side == "R" else (4, 1 << 31)
    rc, n, st = _call(hw, entry, KEYS, VALID, nR, KEYS, VALID, nS)
    assert rc == 3
    msg = hw.lib().hwbrj_last_error()
    assert b"key column " + side.encode() in msg and b"2^31" in msg
    assert _unwritten(hw, n, st)


@pytest.mark.parametrize("entry", ["semi", "outer"])
def test_unknown_kind_is_refused_without_a_device(hw, entry):
    for kind in (-1, 3, 99):
        rc, n, st = _call(hw, entry, KEYS, VALID, 4, KEYS, VALID, 4, out=OUT, cap=8, kind=kind)
        assert rc == 2
        assert b"kind" in hw.lib().hwbrj_last_error()
        assert _unwritten(hw, n, st)


@pytest.mark.parametrize("entry", ["pairs", "semi", "outer"])
def test_capacity_without_an_output_is_refused_without_a_device(hw, entry):
    rc, n, st = _call(hw, entry, KEYS, VALID, 4, KEYS, VALID, 4, out=None, cap=8)
    assert rc == 2
    assert b"d_out" in hw.lib().hwbrj_last_error()
    assert _unwritten(hw, n, st)


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 31, 32, 33, 1000])
def test_pack_validity_is_numpys_little_endian_packbits(hw, n):
    import torch
    v = np.random.default_rng(n).integers(0, 2, size=n).astype(bool)
    got = hw.pack_validity(torch.from_numpy(v))
    assert got.dtype == torch.uint8 and got.dim() == 1 and got.is_contiguous()
    assert got.shape[0] == (n + 31) // 32 * 4  # padded to a multiple of 4 bytes
    want = np.packbits(v, bitorder="little")
    g = got.numpy()
    assert np.array_equal(g[: want.size], want)
    assert not g[want.size:].any()  # the padding is zero
    for bad in (torch.zeros(4, dtype=torch.uint8), torch.zeros((2, 2), dtype=torch.bool), np.zeros(4, dtype=bool)):
        with pytest.raises(ValueError):
            hw.pack_validity(bad)


@pytest.mark.parametrize("name", WRAPPERS)
def test_wrappers_refuse_what_is_no_validity(hw, name):
    """_check_valid's ValueErrors, raised before the key columns are looked at and before the library
    is called (every tensor here is on the CPU; the GPU file checks a bitmap on the wrong device)."""
    import torch
    fn = getattr(hw, name)
    keys = torch.zeros(40, dtype=torch.int32)
    bitmap = torch.zeros(16, dtype=torch.uint8)
    bad = {"int32 mask": torch.ones(40, dtype=torch.int32),
           "numpy mask": np.ones(40, dtype=bool),
           "bool mask, wrong length": torch.ones(39, dtype=torch.bool),
           "bitmap too short": torch.zeros(4, dtype=torch.uint8),
           "2-D bitmap": torch.zeros((5, 1), dtype=torch.uint8),
           "strided bitmap": bitmap[::2],
           "misaligned bitmap": bitmap[1:9]}
    assert bitmap.data_ptr() % 4 == 0
    for what, v in bad.items():
        with pytest.raises(ValueError, match="r_valid"):
            fn(keys, keys, r_valid=v)
        with pytest.raises(ValueError, match="s_valid"):
            fn(keys, keys, s_valid=v)
    with pytest.raises(TypeError):
        fn(keys, keys, None, None, None, None, None, bitmap)  # keyword-only
