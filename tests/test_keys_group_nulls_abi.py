"""The group joins on key columns with validity bitmaps (hwbrj_join_keys_group_nulls_device,
hwbrj_join_keys_group_minmax_nulls_device, include/hwbrj.h): the exports and their prototype, the
wrappers' keywords, and every refusal that is decided before any device call, tested with pointers
that are never dereferenced. No GPU."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

KEYS, KEYS_BAD, VALID, OUT = 0x1000, 0x1004, 0x3000, 0x2000
UNWRITTEN = 0x5A5A5A5A5A5A5A5A
ENTRIES = ["hwbrj_join_keys_group_nulls_device", "hwbrj_join_keys_group_minmax_nulls_device"]
WRAPPERS = ["group_join_keys_device", "group_minmax_join_keys_device"]
BITMAPS = ["r_valid", "s_valid", "sv_valid"]  # the three positions


def _call(hw, entry, pr=KEYS, vr=None, nR=40, ps=KEYS, vs=None, pv=KEYS, vv=None, nS=40, out=None, cap=0, kind=0,
          args=None):
    """(return code, *n_out, *n_pairs, *stats' bytes) after one call of a C entry; the three start as
    UNWRITTEN / 0x5A bytes."""
    n, pairs = ctypes.c_uint64(UNWRITTEN), ctypes.c_uint64(UNWRITTEN)
    st = hw._Stats()
    ctypes.memset(ctypes.byref(st), 0x5A, ctypes.sizeof(st))
    a = ctypes.byref(args) if args is not None else None
    rc = getattr(hw.lib(), entry)(pr, vr, nR, ps, vs, pv, vv, nS, a, kind, out, cap, ctypes.byref(n), ctypes.byref(pairs),
                                  None, ctypes.byref(st), None)
    return rc, n.value, pairs.value, bytes(st)


def _unwritten(hw, n, pairs, st):
    return n == UNWRITTEN and pairs == UNWRITTEN and st == b"\x5a" * ctypes.sizeof(hw._Stats)


def _one(which, p=VALID):
    """The three bitmap arguments with `which` (a name of BITMAPS, or "all") set to p."""
    return {k: (p if which in (n, "all") else None) for k, n in (("vr", "r_valid"), ("vs", "s_valid"), ("vv", "sv_valid"))}


def _past_the_bitmap_checks(hw, entry, masks, args):
    """A call that gets past the bitmaps' checks and ends before any kernel: an unknown kind (2)."""
    rc, n, pairs, st = _call(hw, entry, out=OUT, cap=8, kind=99, args=args, **masks)
    msg = hw.lib().hwbrj_last_error()
    assert rc == 2 and b"kind" in msg and _unwritten(hw, n, pairs, st)
    return rc, msg


def test_library_exports_the_entries(hw):
    for name in ENTRIES:
        assert hasattr(hw.lib(), name)


def test_header_declares_the_prototype():
    """include/hwbrj.h: both entries with the seventeen parameters of the issue, in order."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hwbrj.h")
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    for name, row in zip(ENTRIES, ("hwbrj_group_row_t", "hwbrj_group_minmax_row_t")):
        m = re.search(r"int\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, name
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        assert params == [
            "const int32_t * d_Rkeys", "const uint8_t * d_Rvalid", "uint64_t nR", "const int32_t * d_Skeys",
            "const uint8_t * d_Svalid", "const int32_t * d_Svals", "const uint8_t * d_Svals_valid", "uint64_t nS",
            "const bloom_filter_args_t * args", "int kind", row + " * d_out", "uint64_t capacity", "uint64_t * n_out",
            "uint64_t * n_pairs", "void * stream", "hwbrj_stats_t * stats", "double * ms"]


def test_wrappers_take_the_keywords(hw):
    for name in WRAPPERS:
        p = inspect.signature(getattr(hw, name)).parameters
        for kw in BITMAPS:
            assert p[kw].kind is inspect.Parameter.KEYWORD_ONLY and p[kw].default is None


@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("which", BITMAPS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_misaligned_bitmap_is_refused_without_a_device(hw, entry, which, off):
    """One bitmap at an address = 1, 2 or 3 (mod 4), the other two aligned: 2, "align", nothing written."""
    masks = {k: v if v is not None else VALID for k, v in _one(which, VALID + off).items()}
    rc, n, pairs, st = _call(hw, entry, out=OUT, cap=8, **masks)
    assert rc == 2
    assert b"align" in hw.lib().hwbrj_last_error() and b"bitmap" in hw.lib().hwbrj_last_error()
    assert _unwritten(hw, n, pairs, st)
    # and alone
    rc, n, pairs, st = _call(hw, entry, out=OUT, cap=8, **_one(which, VALID + off))
    assert rc == 2 and b"align" in hw.lib().hwbrj_last_error() and _unwritten(hw, n, pairs, st)


@pytest.mark.parametrize("entry", ENTRIES)
def test_misaligned_bitmap_of_an_empty_column_is_not_refused(hw, entry):
    """n = 0 with bitmaps at odd addresses passes the alignment check (each side alone, and both): the
    call ends at the unknown kind instead."""
    for nR, nS in ((0, 0), (0, 40), (40, 0)):
        masks = dict(vr=VALID + 1 if nR == 0 else VALID, vs=VALID + 3 if nS == 0 else VALID,
                     vv=VALID + 2 if nS == 0 else VALID)
        rc, n, pairs, st = _call(hw, entry, nR=nR, nS=nS, out=OUT, cap=8, kind=99, **masks)
        assert rc == 2
        assert b"kind" in hw.lib().hwbrj_last_error() and b"align" not in hw.lib().hwbrj_last_error()
        assert _unwritten(hw, n, pairs, st)


def _unsupported(hw):
    return {"global_b4": hw._BloomArgs(hw.BLOCKED, 1 << 20, 1, 4), "basic_k3": hw._BloomArgs(hw.BASIC, 1 << 22, 3, 0),
            "basic_k0": hw._BloomArgs(hw.BASIC, 1 << 22, 0, 0)}


@pytest.mark.parametrize("which", BITMAPS + ["all"])
@pytest.mark.parametrize("cfg", ["global_b4", "basic_k3", "basic_k0"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_unsupported_filter_with_a_bitmap_gives_9(hw, entry, cfg, which):
    rc, n, pairs, st = _call(hw, entry, out=OUT, cap=8, args=_unsupported(hw)[cfg], **_one(which))
    assert rc == 9
    assert b"bitmap" in hw.lib().hwbrj_last_error()
    assert _unwritten(hw, n, pairs, st)


@pytest.mark.parametrize("cfg", ["global_b4", "basic_k3", "basic_k0"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_unsupported_filter_without_bitmaps_is_the_counterparts_business(hw, entry, cfg):
    """All three bitmaps NULL: not 9, the call goes on to the counterpart's own checks."""
    rc, msg = _past_the_bitmap_checks(hw, entry, _one("none"), _unsupported(hw)[cfg])
    assert rc != 9 and b"bitmap" not in msg


@pytest.mark.parametrize("cfg", [None, "blocked", "sectorized", "basic_k1"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_supported_filters_pass_the_bitmap_checks(hw, entry, cfg):
    args = {None: None, "blocked": hw._BloomArgs(hw.BLOCKED, 1 << 24, 1, 1024),
            "sectorized": hw._BloomArgs(hw.SECTORIZED, 1 << 24, 2, 1024), "basic_k1": hw._BloomArgs(hw.BASIC, 1 << 24, 1, 0)}[cfg]
    rc, msg = _past_the_bitmap_checks(hw, entry, _one("all"), args)
    assert rc != 9 and b"bitmap" not in msg


@pytest.mark.parametrize("column", ["Rkeys", "Skeys", "Svals"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_counterparts_column_alignment_still_comes_first(hw, entry, column):
    p = {c: KEYS_BAD if c == column else KEYS for c in ("Rkeys", "Skeys", "Svals")}
    rc, n, pairs, st = _call(hw, entry, pr=p["Rkeys"], ps=p["Skeys"], pv=p["Svals"], nR=4, nS=4, **_one("all", VALID + 1))
    assert rc == 2
    msg = hw.lib().hwbrj_last_error()
    assert b"align" in msg and b"column" in msg and b"bitmap" not in msg
    assert _unwritten(hw, n, pairs, st)


@pytest.mark.parametrize("entry", ENTRIES)
def test_counterparts_refusals_hold(hw, entry):
    """d_Svals NULL with nS > 0, nR >= 2^31, nS >= 2^32, an unknown kind, a misaligned d_out and a
    capacity without d_out, each with all three bitmaps set: the counterpart's code, nothing written."""
    L, m = hw.lib(), _one("all")
    cases = [
        (dict(pv=None, out=OUT, cap=8), 2, b"d_Svals"),
        (dict(nR=1 << 31), 3, b"key column R"),
        (dict(nS=1 << 32), 3, b"2^32"),
        (dict(out=OUT, cap=8, kind=-1), 2, b"kind"),
        (dict(out=OUT, cap=8, kind=2), 2, b"kind"),
        (dict(out=OUT + 8, cap=8), 2, b"d_out"),
        (dict(out=None, cap=8), 2, b"d_out"),
    ]
    for kw, code, word in cases:
        rc, n, pairs, st = _call(hw, entry, **kw, **m)
        assert rc == code, kw
        assert word in L.hwbrj_last_error()
        assert _unwritten(hw, n, pairs, st)
    # 2^31 S rows pass the row limits (S row indices are never produced)
    rc, n, pairs, st = _call(hw, entry, nS=1 << 31, out=OUT, cap=8, kind=99, **m)
    assert rc == 2 and b"kind" in L.hwbrj_last_error()


@pytest.mark.parametrize("name", WRAPPERS)
def test_wrappers_refuse_what_is_no_validity(hw, name):
    """_check_valid's ValueErrors for each of the three keywords, raised before the columns are looked
    at and before the library is called (every tensor here is on the CPU)."""
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
        for kw in BITMAPS:
            with pytest.raises(ValueError, match=kw):
                fn(keys, keys, keys, **{kw: v})
    with pytest.raises(TypeError):
        fn(keys, keys, keys, None, 0, None, None, bitmap)  # keyword-only
