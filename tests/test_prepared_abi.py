"""Prepared builds (hwbrj_build_keys_device, the hwbrj_probe_keys_* entries, hwbrj_build_unmatched_device;
include/hwbrj.h "Prepared builds"): the exports, the Python names, and every refusal that is decided
before any device call, tested with pointers that are never dereferenced. No GPU."""
import ctypes
import inspect

import pytest

KEYS, KEYS_BAD, VALID, OUT = 0x1000, 0x1004, 0x3000, 0x2000
UNWRITTEN = 0x5A5A5A5A5A5A5A5A
BUILD_COUNT, BUILD_ROWS = 0, 1
EXPORTS = ("hwbrj_build_keys_device", "hwbrj_build_free", "hwbrj_build_info", "hwbrj_build_export_filter",
           "hwbrj_probe_keys_device", "hwbrj_probe_keys_pairs_device", "hwbrj_probe_keys_semi_device",
           "hwbrj_probe_keys_outer_device", "hwbrj_probe_keys_group_device", "hwbrj_probe_keys_group_minmax_device",
           "hwbrj_build_unmatched_device", "hwbrj_build_reset_marks")
NAMES = ("Build", "build_keys_device", "BUILD_COUNT", "BUILD_ROWS", "PROBE_MARK_INNER", "PROBE_MARK_S",
         "probe_keys_device", "probe_keys_pairs_device", "semi_probe_keys_device", "outer_probe_keys_device",
         "group_probe_keys_device", "group_minmax_probe_keys_device")
PROBES = ("count", "pairs", "semi", "outer", "group", "minmax")


def _build(hw, pr, vr, nR, args=None, purpose=BUILD_ROWS, null_out=False):
    """(return code, *build after the call) of hwbrj_build_keys_device; *build starts as UNWRITTEN."""
    h = ctypes.c_void_p(UNWRITTEN)
    rc = hw.lib().hwbrj_build_keys_device(pr, vr, nR, ctypes.byref(args) if args is not None else None, purpose, None,
                                          None if null_out else ctypes.byref(h), None)
    return rc, h.value


def _probe(hw, entry, build, kind=0):
    """(return code, *n_out, *stats' bytes) of one probe entry on `build`, with S in order."""
    L = hw.lib()
    n = ctypes.c_uint64(UNWRITTEN)
    st = hw._Stats()
    ctypes.memset(ctypes.byref(st), 0x5A, ctypes.sizeof(st))
    if entry == "count":
        rc = L.hwbrj_probe_keys_device(build, KEYS, None, 40, 0, None, ctypes.byref(st))
    elif entry == "pairs":
        rc = L.hwbrj_probe_keys_pairs_device(build, KEYS, None, 40, OUT, 8, ctypes.byref(n), None, ctypes.byref(st), None)
    elif entry == "semi":
        rc = L.hwbrj_probe_keys_semi_device(build, KEYS, None, 40, kind, OUT, 8, ctypes.byref(n), None, ctypes.byref(st),
                                            None)
    elif entry == "outer":
        rc = L.hwbrj_probe_keys_outer_device(build, KEYS, None, 40, kind, OUT, 8, ctypes.byref(n), None, None,
                                             ctypes.byref(st), None)
    else:
        fn = L.hwbrj_probe_keys_group_device if entry == "group" else L.hwbrj_probe_keys_group_minmax_device
        rc = fn(build, KEYS, None, KEYS, None, 40, kind, OUT, 8, ctypes.byref(n), None, None, ctypes.byref(st), None)
    return rc, n.value, bytes(st)


def test_library_exports_the_prepared_entries(hw):
    for name in EXPORTS:
        assert hasattr(hw.lib(), name), name


def test_python_names(hw):
    for name in NAMES:
        assert hasattr(hw, name) and name in hw.__all__, name
    assert (hw.BUILD_COUNT, hw.BUILD_ROWS, hw.PROBE_MARK_INNER, hw.PROBE_MARK_S) == (0, 1, 3, 4)
    for m in ("free", "info", "export_filter", "unmatched_rows", "reset_marks", "__enter__", "__exit__", "__del__"):
        assert callable(getattr(hw.Build, m)), m
    p = inspect.signature(hw.build_keys_device).parameters
    assert list(p) == ["Rk", "args", "purpose", "r_valid", "stream"]
    assert p["args"].default is None and p["purpose"].default == hw.BUILD_ROWS and p["r_valid"].default is None
    for name in NAMES[6:]:
        p = inspect.signature(getattr(hw, name)).parameters
        assert list(p)[0] == "build" and "Rk" not in p and "args" not in p, name
        assert p["s_valid"].kind is inspect.Parameter.KEYWORD_ONLY and p["s_valid"].default is None
    for name in ("group_probe_keys_device", "group_minmax_probe_keys_device"):
        p = inspect.signature(getattr(hw, name)).parameters
        assert p["sv_valid"].kind is inspect.Parameter.KEYWORD_ONLY and p["sv_valid"].default is None


@pytest.mark.parametrize("purpose", [-1, 2, 99])
def test_unknown_purpose_is_refused(hw, purpose):
    rc, h = _build(hw, KEYS, None, 40, purpose=purpose)
    assert rc == 2 and h == UNWRITTEN
    assert b"purpose" in hw.lib().hwbrj_last_error()


@pytest.mark.parametrize("purpose", [BUILD_COUNT, BUILD_ROWS])
def test_null_build_argument_is_refused(hw, purpose):
    rc, _ = _build(hw, KEYS, None, 40, purpose=purpose, null_out=True)
    assert rc == 2
    assert b"build" in hw.lib().hwbrj_last_error()


@pytest.mark.parametrize("purpose", [BUILD_COUNT, BUILD_ROWS])
def test_misaligned_key_column_is_refused(hw, purpose):
    rc, h = _build(hw, KEYS_BAD, None, 40, purpose=purpose)
    assert rc == 2 and h == UNWRITTEN
    assert b"align" in hw.lib().hwbrj_last_error() and b"key column R" in hw.lib().hwbrj_last_error()


@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("purpose", [BUILD_COUNT, BUILD_ROWS])
def test_misaligned_bitmap_is_refused(hw, purpose, off):
    rc, h = _build(hw, KEYS, VALID + off, 40, purpose=purpose)
    assert rc == 2 and h == UNWRITTEN
    assert b"align" in hw.lib().hwbrj_last_error() and b"bitmap" in hw.lib().hwbrj_last_error()


@pytest.mark.parametrize("purpose", [BUILD_COUNT, BUILD_ROWS])
def test_misaligned_bitmap_of_an_empty_column_is_not_refused(hw, purpose):
    """nR = 0 with a bitmap (and a column) at odd addresses passes the alignment checks. The call still
    ends before any kernel: m = 3 is no filter size (2, naming m)."""
    rc, h = _build(hw, KEYS_BAD, VALID + 1, 0, args=hw._BloomArgs(hw.BLOCKED, 3, 1, 1024), purpose=purpose)
    assert rc == 2 and h == UNWRITTEN
    msg = hw.lib().hwbrj_last_error()
    assert b"align" not in msg and b"power of 2" in msg


@pytest.mark.parametrize("with_bitmap", [False, True])
@pytest.mark.parametrize("purpose", [BUILD_COUNT, BUILD_ROWS])
@pytest.mark.parametrize("cfg", ["global_b4", "basic_k3", "basic_k0"])
def test_unsupported_filters_give_9(hw, cfg, purpose, with_bitmap):
    args = {"global_b4": hw._BloomArgs(hw.BLOCKED, 1 << 20, 1, 4), "basic_k3": hw._BloomArgs(hw.BASIC, 1 << 22, 3, 0),
            "basic_k0": hw._BloomArgs(hw.BASIC, 1 << 22, 0, 0)}[cfg]
    rc, h = _build(hw, KEYS, VALID if with_bitmap else None, 40, args=args, purpose=purpose)
    assert rc == 9 and h == UNWRITTEN
    assert b"partition slices" in hw.lib().hwbrj_last_error()


def test_2_pow_31_rows_are_refused_under_build_rows(hw):
    rc, h = _build(hw, KEYS, VALID, 1 << 31, purpose=BUILD_ROWS)
    assert rc == 3 and h == UNWRITTEN
    assert b"2^31" in hw.lib().hwbrj_last_error() and b"key column R" in hw.lib().hwbrj_last_error()
    # the same rows with an unsupported filter: the row limit comes first, as in the one-shot entries
    rc, h = _build(hw, KEYS, VALID, 1 << 31, args=hw._BloomArgs(hw.BLOCKED, 1 << 20, 1, 4), purpose=BUILD_ROWS)
    assert rc == 3 and h == UNWRITTEN


@pytest.mark.parametrize("entry", PROBES)
def test_probe_on_a_null_build_gives_2(hw, entry):
    rc, n, st = _probe(hw, entry, None)
    assert rc == 2
    assert b"build is NULL" in hw.lib().hwbrj_last_error()
    assert n == UNWRITTEN and st == b"\x5a" * ctypes.sizeof(hw._Stats)


def test_build_entries_on_a_null_build(hw):
    L = hw.lib()
    out = (ctypes.c_uint64 * 16)()
    n = ctypes.c_uint64(UNWRITTEN)
    assert L.hwbrj_build_info(None, out, 16) == 2
    assert L.hwbrj_build_export_filter(None, OUT, 8) == 2
    assert L.hwbrj_build_unmatched_device(None, OUT, 8, ctypes.byref(n), None, None) == 2 and n.value == UNWRITTEN
    assert L.hwbrj_build_reset_marks(None) == 2
    assert L.hwbrj_build_free(None) == 0  # (nothing to free)


@pytest.mark.parametrize("kind", [3, 4])
@pytest.mark.parametrize("nulls", [False, True])
def test_one_shot_outer_join_still_refuses_the_marking_kinds(hw, kind, nulls):
    L = hw.lib()
    n = ctypes.c_uint64(UNWRITTEN)
    if nulls:
        rc = L.hwbrj_join_keys_outer_nulls_device(KEYS, VALID, 4, KEYS, VALID, 4, None, kind, OUT, 8, ctypes.byref(n),
                                                  None, None, None, None)
    else:
        rc = L.hwbrj_join_keys_outer_device(KEYS, 4, KEYS, 4, None, kind, OUT, 8, ctypes.byref(n), None, None, None, None)
    assert rc == 2 and n.value == UNWRITTEN
    assert b"kind" in hw.lib().hwbrj_last_error()
