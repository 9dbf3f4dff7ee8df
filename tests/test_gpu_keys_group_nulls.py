"""The group joins on key columns with validity bitmaps (r_valid / s_valid / sv_valid of
hw.group_join_keys_device and hw.group_minmax_join_keys_device).

Every expectation is test_gpu_group.reference (COUNT, SUM) or test_gpu_group_minmax.reference (COUNT,
MIN, MAX) on the compacted tuples R = {Rk[vR], original row} and S = {Sk[v], Sv[v]} with v = vS & vV;
under GROUP_ALL the identity rows of the NULL R rows are added. n_pairs is the reference's count sum
and `filtered` is orc.bpro on the compacted relations. Nothing is compared with the code under test
alone.

The data is planted so that an ignored bit cannot pass by luck: the keys under NULL key rows are live
keys of the other side (alternating with absent ones), the values under NULL value bits alternate
INT32_MIN / INT32_MAX (a leak changes COUNT, SUM, MIN and MAX), and S's two bitmaps always differ."""
import ctypes

import numpy as np
import pytest

import shapes
import test_gpu_group as g
import test_gpu_group_minmax as mm
import test_gpu_keys_group as kg
import test_gpu_keys_nulls as kn
import test_gpu_keys_pairs as kp
import test_gpu_shapes as gs
from test_gpu_materialize import _args

pytestmark = pytest.mark.gpu

INT_MIN, INT_MAX = -2**31, 2**31 - 1
FORMS = {"sum": (g, "group_join_keys_device"), "minmax": (mm, "group_minmax_join_keys_device")}
_dev, _dmask, _distinct = kg._dev, kn._dmask, kn._distinct


def _bits(n, pattern):
    """n validity bits that repeat one byte."""
    return np.unpackbits(np.full((n + 7) // 8, pattern, dtype=np.uint8), bitorder="little")[:n].astype(bool)


def _poison(Sv, vV):
    """INT32_MIN / INT32_MAX, alternating, under the NULL value bits."""
    Sv = kg._i32(Sv).copy()
    at = np.nonzero(~vV)[0]
    Sv[at[::2]], Sv[at[1::2]] = INT_MIN, INT_MAX
    return Sv


class GRef:
    """What the group joins of the columns Rk, Sk, Sv with validity vR, vS, vV (bool arrays; None: all
    valid) must return, from the host references on the compacted tuples."""

    def __init__(self, Rk, Sk, Sv, vR=None, vS=None, vV=None):
        self.Rk, self.Sk, self.Sv = kg._i32(Rk), kg._i32(Sk), kg._i32(Sv)
        self.vR = np.ones(self.Rk.size, bool) if vR is None else np.asarray(vR, bool)
        vS = np.ones(self.Sk.size, bool) if vS is None else np.asarray(vS, bool)
        vV = np.ones(self.Sk.size, bool) if vV is None else np.asarray(vV, bool)
        self.v = vS & vV
        rR = np.nonzero(self.vR)[0]
        self.R, self.S = kg._tuples(self.Rk[rR], rR), kg._tuples(self.Sk[self.v], self.Sv[self.v])
        self.nulls = np.nonzero(~self.vR)[0].astype(np.int64)
        self._rows = {}

    def rows(self, form, kind_all):
        """Sorted rows of one form: GROUP_ALL (with the NULL R rows' identity rows) or GROUP_MATCHED."""
        mod = FORMS[form][0]
        if form not in self._rows:
            ref = mod.reference(self.R, self.S)
            ident = [0, 0] if form == "sum" else [0, INT_MAX, INT_MIN]
            null_rows = np.concatenate([self.nulls[:, None], np.tile(np.array(ident, dtype=np.int64), (self.nulls.size, 1))], 1)
            both = (mod._sorted(np.concatenate([ref, null_rows])), mod._sorted(ref[ref[:, 1] > 0]))
            for a in both:
                a.setflags(write=False)
            self._rows[form] = both
        return self._rows[form][0 if kind_all else 1]

    def n_pairs(self):
        return int(self.rows("sum", False)[:, 1].sum())

    def counts(self, orc, args):
        """(filtered, matches) of the counting join on the compacted relations."""
        if self.S.shape[0] == 0:
            return (0, 0)  # (no participating S row: nothing to filter, nothing to match)
        return kp._counts(orc, self.R, self.S, args)


def check(hw, ref, cols, masks, args, counts=None, forms=("sum", "minmax"), kinds=None, skip=()):
    """Every form and kind (but the (form, kind) pairs of `skip`) against the reference; masks =
    (r_valid, s_valid, sv_valid). Returns {(form, kind): rows sorted by r_payload}."""
    kw = dict(r_valid=masks[0], s_valid=masks[1], sv_valid=masks[2])
    out = {}
    for form in forms:
        mod, fn = FORMS[form]
        for kind in kinds if kinds is not None else (hw.GROUP_MATCHED, hw.GROUP_ALL):
            if (form, kind) in skip:
                continue
            want = ref.rows(form, kind == hw.GROUP_ALL)
            st, rows, pairs, _ = getattr(hw, fn)(*cols, args, kind=kind, **kw)
            rows = mod._sorted(mod._host(rows))
            print(f"{form} kind {kind}: {rows.shape[0]} rows (host {want.shape[0]}), n_pairs {pairs} (host "
                  f"{ref.n_pairs()}), filtered {st.filtered} (oracle {counts})")
            assert rows.shape[0] == want.shape[0] == st.matches
            assert pairs == ref.n_pairs()
            assert np.array_equal(rows, want)
            if kind == hw.GROUP_ALL:
                assert rows.shape[0] == ref.Rk.size
            if counts is not None:
                assert st.filtered == counts[0] and pairs == counts[1]
            out[form, kind] = rows
    return out


# ------------------------------------------------------------------------------ 1. every mode
_MODE = {}


def _mode_case(orc, cuda):
    if not _MODE:
        R = orc.relation(400000, 2, 400000, 400000, 1.0, 1)
        S = orc.relation(3000000, 2, INT_MAX, 400000, 0.2, 2)
        rng = np.random.default_rng(20)
        Rk, Sk = R[:, 0].copy(), S[:, 0].copy()
        vR, vS, vV = rng.random(Rk.size) >= 0.2, rng.random(Sk.size) >= 0.2, rng.random(Sk.size) >= 0.2
        kn._plant(Rk, Sk, vR, vS, rng)
        Sv = _poison(rng.integers(-10**6, 10**6, size=Sk.size), vV)
        ref = GRef(Rk, Sk, Sv, vR, vS, vV)
        assert not np.array_equal(vS, vV)
        plain = GRef(Rk, Sk, Sv)
        assert 0 < ref.n_pairs() < GRef(Rk, Sk, Sv, vR, vS).n_pairs() < plain.n_pairs()  # each mask matters
        _MODE.update(ref=ref, cols=(_dev(cuda, Rk), _dev(cuda, Sk), _dev(cuda, Sv)),
                     masks=(_dmask(cuda, vR), _dmask(cuda, vS), _dmask(cuda, vV)), counts={})
    return _MODE


@pytest.mark.parametrize("form", ["sum", "minmax"])
@pytest.mark.parametrize("name", kn.SUPPORTED)
def test_every_supported_mode(hw, cuda, orc, name, form):
    """R 400,000 / S 3,000,000; a fifth of R's keys, a fifth of S's keys and an independent fifth of
    S's values NULL; both kinds."""
    M = _mode_case(orc, cuda)
    args = _args(hw)[name]
    if name not in M["counts"]:
        M["counts"][name] = M["ref"].counts(orc, args)
    check(hw, M["ref"], M["cols"], M["masks"], args, M["counts"][name], forms=(form,))


@pytest.mark.parametrize("name", kn.REFUSED)
def test_unsupported_modes_raise_9(hw, cuda, orc, name):
    M = _mode_case(orc, cuda)
    args = _args(hw)[name]
    mR, mS, mV = M["masks"]
    for kw in (dict(r_valid=mR), dict(s_valid=mS), dict(sv_valid=mV), dict(r_valid=mR, s_valid=mS, sv_valid=mV)):
        for fn in (hw.group_join_keys_device, hw.group_minmax_join_keys_device):
            with pytest.raises(RuntimeError, match=r"\(9\)"):
                fn(*M["cols"], args, **kw)


# ------------------------------------------------------------------ 2. full rounds with NULLs
_FULL = {}


def _full_case(hw, cuda):
    if not _FULL:
        G, rnd = kn._G(hw, cuda)
        n = 2 * G * rnd + 5
        e0 = kn._e0(n, G)
        # every workgroup has a full round, and the ranges start at odd nibbles and off dword boundaries
        assert np.all(np.diff(np.append(e0, n)) >= rnd)
        assert np.any(e0 % 8 == 4) and np.any(e0 % 32 != 0)
        big = _distinct(n)
        other = np.concatenate([big[::97], _distinct(500, first=n)])
        np.random.default_rng(n).shuffle(other)
        rng = np.random.default_rng(3)
        _FULL.update(n=n, big=big, other=other, cb=_dev(cuda, big), co=_dev(cuda, other),
                     vals_big=kg._i32(rng.integers(-10**6, 10**6, size=n)),
                     vals_other=kg._i32(rng.integers(-10**6, 10**6, size=other.size)),
                     all_big=_dmask(cuda, np.ones(n, bool)), all_other=_dmask(cuda, np.ones(other.size, bool)))
        _FULL["cvo"] = _dev(cuda, _FULL["vals_other"])
    return _FULL


def _full_check(hw, cuda, orc, which, vb, vb2=None):
    """The big column (R for r_valid, else S) under validity vb on bitmap `which` (and vb2 on S's value
    bitmap when given), every other bitmap present and all valid."""
    F = _full_case(hw, cuda)
    mb = _dmask(cuda, vb, tail=int(vb.sum()) & 1)  # (tail bits set and clear, by the case)
    if which == "r_valid":
        assert vb.all() or np.isin(F["big"][~vb], F["other"]).any()  # live keys under NULL rows
        ref = GRef(F["big"], F["other"], F["vals_other"], vb)
        cols, masks = (F["cb"], F["co"], F["cvo"]), (mb, F["all_other"], F["all_other"])
    else:
        vS = vb if which == "s_valid" else None
        vV = vb2 if vb2 is not None else vb if which == "sv_valid" else None
        Sv = F["vals_big"] if vV is None else _poison(F["vals_big"], vV)
        assert vb.all() or np.isin(F["big"][~vb], F["other"]).any()
        ref = GRef(F["other"], F["big"], Sv, None, vS, vV)
        mS = mb if which == "s_valid" else F["all_big"]
        mV = _dmask(cuda, vV) if vb2 is not None else mb if which == "sv_valid" else F["all_big"]
        cols, masks = (F["co"], F["cb"], _dev(cuda, Sv)), (F["all_other"], mS, mV)
    # (r_valid: GROUP_ALL returns all 4.2 M rows of the big column, so each filter takes it in one form)
    skips = {"nobloom": (("minmax", hw.GROUP_ALL),), "blocked_packed": (("sum", hw.GROUP_ALL),)}
    for name in ("nobloom", "blocked_packed"):
        args = _args(hw)[name]
        check(hw, ref, cols, masks, args, ref.counts(orc, args), skip=skips[name] if which == "r_valid" else ())
    return ref


@pytest.mark.parametrize("which", ["r_valid", "s_valid", "sv_valid"])
@pytest.mark.parametrize("pattern", kn.PATTERNS, ids=[f"0x{p:02X}" for p in kn.PATTERNS])
def test_full_rounds_with_nulls(hw, cuda, orc, pattern, which):
    """2 G round + 5 distinct keys in an exactly-sized column whose bitmap repeats one byte (0xFF: all
    valid, 0x00: all NULL), on each of the three bitmaps with the other two all valid; the other side
    holds every 97th key and 500 absent ones."""
    n = _full_case(hw, cuda)["n"]
    _full_check(hw, cuda, orc, which, _bits(n, pattern))


def test_full_rounds_with_two_different_bitmaps(hw, cuda, orc):
    """S's key bitmap 0x55 and its value bitmap 0x33: a row takes part iff both bits are set (0x11). A
    kernel that reads one of them only, or ORs them, counts more."""
    n = _full_case(hw, cuda)["n"]
    vS, vV = _bits(n, 0x55), _bits(n, 0x33)
    ref = _full_check(hw, cuda, orc, "s_valid", vS, vV)
    assert np.array_equal(ref.v, _bits(n, 0x11))
    hit = np.isin(_FULL["big"], _FULL["other"])  # (distinct keys: a participating S row with a partner is one pair)
    assert ref.n_pairs() == int(hit[ref.v].sum()) < min(int(hit[vS].sum()), int(hit[vV].sum()))


# ------------------------------------------------------------------------------- 3. edges
@pytest.mark.parametrize("which", ["r_valid", "s_valid", "sv_valid"])
@pytest.mark.parametrize("nspec", kn.EDGE_N)
def test_nulls_at_every_edge(hw, cuda, orc, nspec, which):
    """A column of exactly n distinct keys and one bitmap of exactly ceil(n / 32) * 4 bytes (the other
    two absent). Four masks: the only NULL at row 0; at row n - 1; one NULL at the last row of every
    workgroup's range (e0 - 1); one at the first row of every range (e0). Each with the bits past n all
    clear and all set: the same result. On R under GROUP_ALL, on each S bitmap under both kinds. The
    other side holds every 3rd key (n < 100) or every 97th, and absent ones."""
    n, G = kn._edge_n(hw, cuda, nspec)
    big = _distinct(n)
    other = np.concatenate([big[:: 3 if n < 100 else 97], _distinct(50, first=n)])
    np.random.default_rng(n).shuffle(other)
    rng = np.random.default_rng(n + 1)
    co, cb = _dev(cuda, other), _dev(cuda, big)
    e0 = np.unique(kn._e0(n, G))
    spots = {"row 0": [0], "row n-1": [n - 1], "every e0-1": e0[e0 > 0] - 1, "every e0": e0[e0 < n]}
    for spot, (what, null_rows) in enumerate(spots.items()):
        vb = np.ones(n, bool)
        vb[np.asarray(null_rows, dtype=np.int64)] = False
        if which == "r_valid":
            Sv = kg._i32(rng.integers(-10**6, 10**6, size=other.size))
            ref, cols, kinds = GRef(big, other, Sv, vb), (cb, co, _dev(cuda, Sv)), (hw.GROUP_ALL,)
        else:
            Sv = kg._i32(rng.integers(-10**6, 10**6, size=n))
            Sv = _poison(Sv, vb) if which == "sv_valid" else Sv
            ref = GRef(other, big, Sv, None, vb if which == "s_valid" else None, vb if which == "sv_valid" else None)
            cols, kinds = (co, cb, _dev(cuda, Sv)), None
        # (a large column: one tail value per mask, and on R, where GROUP_ALL returns n rows, one form
        # per filter; over the four masks both tails and all four filter / form pairs occur)
        large = n > 100000
        for tail in ((spot & 1,) if large else (0, 1)):
            mb = _dmask(cuda, vb, tail)
            assert mb.numel() == (n + 31) // 32 * 4
            masks = tuple(mb if which == w else None for w in ("r_valid", "s_valid", "sv_valid"))
            print(f"-- {what}, tail bits {tail}")
            for i, name in enumerate(("nobloom", "blocked_packed")):
                forms = (("sum", "minmax")[(spot // 2 + i) & 1],) if large and which == "r_valid" else ("sum", "minmax")
                check(hw, ref, cols, masks, _args(hw)[name], forms=forms, kinds=kinds)


# ------------------------------------------------------------- 4. degenerate ranges and sides
@pytest.mark.parametrize("which", ["s_valid", "sv_valid"])
def test_one_workgroups_whole_s_range_is_null(hw, cuda, orc, which):
    G, rnd = kn._G(hw, cuda)
    n = G * rnd + 12
    big, w = _distinct(n), G // 3
    lo, hi = shapes.wg_range(n, G, w)
    assert hi - lo >= rnd
    vb = np.ones(n, bool)
    vb[lo:hi] = False
    other = np.concatenate([big[::53], _distinct(300, first=n)])
    assert np.isin(big[lo:hi], other).any()
    Sv = _poison(np.random.default_rng(4).integers(-10**6, 10**6, size=n), vb)
    ref = GRef(other, big, Sv, None, vb if which == "s_valid" else None, vb if which == "sv_valid" else None)
    cols = (_dev(cuda, other), _dev(cuda, big), _dev(cuda, Sv))
    mb = _dmask(cuda, vb)
    masks = (None, mb, None) if which == "s_valid" else (None, None, mb)
    for name in ("nobloom", "blocked_packed"):
        args = _args(hw)[name]
        check(hw, ref, cols, masks, args, ref.counts(orc, args))


def test_a_partition_whose_only_r_rows_are_null(hw, cuda, orc):
    """PRO and the blocked filter partition by the code's low 10 bits: every R row of partition 5 is
    NULL, and S holds those keys as valid rows."""
    crc = shapes.Crc(orc.crc)
    assert gs.geometry(hw, cuda, None, 8, mat=True)["F"] == 1024
    Rk, Sk = _distinct(300000), np.concatenate([_distinct(300000)[::2], _distinct(200000, first=300000)])
    vR = (crc.code(Rk) & 1023) != 5
    assert (~vR).sum() > 100 and np.isin(Sk, Rk[~vR]).any()
    Sv = np.random.default_rng(6).integers(INT_MIN, INT_MAX, size=Sk.size, endpoint=True)
    ref = GRef(Rk, Sk, Sv, vR)
    cols, masks = (_dev(cuda, Rk), _dev(cuda, Sk), _dev(cuda, Sv)), (_dmask(cuda, vR), None, None)
    for name in ("nobloom", "blocked_packed"):
        args = _args(hw)[name]
        check(hw, ref, cols, masks, args, ref.counts(orc, args))


@pytest.mark.parametrize("name", ["nobloom", "blocked_packed", "basic_k1"])
def test_all_null_and_empty_sides(hw, cuda, orc, name):
    Rk, Sk = _distinct(70001), np.concatenate([_distinct(70001)[::3], _distinct(50000, first=70001)])
    nR, nS = Rk.size, Sk.size
    Sv = np.random.default_rng(8).integers(INT_MIN, INT_MAX, size=nS, endpoint=True)
    cols = (_dev(cuda, Rk), _dev(cuda, Sk), _dev(cuda, Sv))
    args = _args(hw)[name]
    none_r, none_s = _dmask(cuda, np.zeros(nR, bool)), _dmask(cuda, np.zeros(nS, bool))
    # R all NULL: GROUP_ALL gives nR identity rows, GROUP_MATCHED none; the filter is empty
    ref = GRef(Rk, Sk, Sv, np.zeros(nR, bool))
    got = check(hw, ref, cols, (none_r, None, None), args, ref.counts(orc, args))
    assert got["sum", hw.GROUP_ALL].shape[0] == nR and not got["sum", hw.GROUP_ALL][:, 1:].any()
    assert (got["minmax", hw.GROUP_ALL][:, 1:] == mm.EMPTY).all()
    assert got["sum", hw.GROUP_MATCHED].shape[0] == got["minmax", hw.GROUP_MATCHED].shape[0] == 0
    # S all NULL by value only: every R row has count 0, nothing is filtered in
    ref = GRef(Rk, Sk, Sv, None, None, np.zeros(nS, bool))
    got = check(hw, ref, cols, (None, None, none_s), args, (0, 0))
    assert got["sum", hw.GROUP_ALL].shape[0] == nR and not got["sum", hw.GROUP_ALL][:, 1:].any()
    # nS = 0 with an R bitmap: every R row, NULL or not, once, with the identity row
    vR = np.random.default_rng(9).random(nR) >= 0.5
    empty = np.empty(0, dtype=np.int32)
    ref = GRef(Rk, empty, empty, vR)
    got = check(hw, ref, (cols[0], _dev(cuda, empty), _dev(cuda, empty)), (_dmask(cuda, vR), None, None), args, (0, 0))
    assert np.array_equal(got["sum", hw.GROUP_ALL][:, 0], np.arange(nR))
    # nR = 0 with S bitmaps
    vS, vV = np.random.default_rng(10).random(nS) >= 0.5, np.arange(nS) % 3 != 0
    ref = GRef(empty, Sk, Sv, None, vS, vV)
    got = check(hw, ref, (_dev(cuda, empty), cols[1], cols[2]), (None, _dmask(cuda, vS), _dmask(cuda, vV)), args)
    assert got["sum", hw.GROUP_ALL].shape[0] == 0


# -------------------------------------------------------------------- 5. one bitmap at a time
def test_one_bitmap_at_a_time_and_none(hw, cuda, orc):
    rng = np.random.default_rng(31)
    Rk, Sk = _distinct(100003), np.concatenate([_distinct(100003)[::2], _distinct(300000, first=100003)])
    rng.shuffle(Sk)
    vR, vS, vV = rng.random(Rk.size) >= 0.3, rng.random(Sk.size) >= 0.3, rng.random(Sk.size) >= 0.3
    kn._plant(Rk, Sk, vR, vS, rng)
    Sv = _poison(rng.integers(-10**6, 10**6, size=Sk.size), vV)
    cols = (_dev(cuda, Rk), _dev(cuda, Sk), _dev(cuda, Sv))
    mR, mS, mV = _dmask(cuda, vR), _dmask(cuda, vS), _dmask(cuda, vV)
    args = _args(hw)["blocked_packed"]
    for ref, masks in ((GRef(Rk, Sk, Sv, vR), (mR, None, None)), (GRef(Rk, Sk, Sv, None, vS), (None, mS, None)),
                       (GRef(Rk, Sk, Sv, None, None, vV), (None, None, mV)), (GRef(Rk, Sk, Sv, None, vS, vV), (None, mS, mV))):
        check(hw, ref, cols, masks, args, ref.counts(orc, args))
    # an all-valid bitmap, one at a time and all three: the rows without a bitmap
    plain = GRef(Rk, Sk, Sv)
    pc = plain.counts(orc, args)
    allR, allS = _dmask(cuda, np.ones(Rk.size, bool)), _dmask(cuda, np.ones(Sk.size, bool), tail=1)
    for masks in ((allR, None, None), (None, allS, None), (None, None, allS), (allR, allS, allS), (None, None, None)):
        check(hw, plain, cols, masks, args, pc)
    # the nulls entries with three NULL bitmaps: the existing entries' rows and `filtered`
    a = args._c()
    for form, entry in (("sum", "hwbrj_join_keys_group_nulls_device"), ("minmax", "hwbrj_join_keys_group_minmax_nulls_device")):
        mod, fn = FORMS[form]
        for kind in (hw.GROUP_MATCHED, hw.GROUP_ALL):
            st0, rows0, pairs0, _ = getattr(hw, fn)(*cols, args, kind=kind)
            want = plain.rows(form, kind == hw.GROUP_ALL)
            buf = cuda.empty((want.shape[0] + 1, 4), dtype=cuda.int32, device="cuda:0")
            n, pairs, st = ctypes.c_uint64(), ctypes.c_uint64(), hw._Stats()
            rc = getattr(hw.lib(), entry)(cols[0].data_ptr(), None, Rk.size, cols[1].data_ptr(), None, cols[2].data_ptr(),
                                          None, Sk.size, ctypes.byref(a), kind, buf.data_ptr(), want.shape[0],
                                          ctypes.byref(n), ctypes.byref(pairs), None, ctypes.byref(st), None)
            assert (rc, n.value, pairs.value, st.filtered) == (0, want.shape[0], plain.n_pairs(), pc[0])
            assert (st0.filtered, pairs0, st0.matches) == (st.filtered, pairs.value, st.matches)
            raw = buf.cpu().numpy()[: n.value]
            if form == "sum":
                got = np.stack([raw[:, 0].astype(np.int64), raw[:, 1].view(np.uint32).astype(np.int64),
                                np.ascontiguousarray(raw[:, 2:]).view(np.int64).ravel()], 1)
            else:
                got = np.stack([raw[:, 0].astype(np.int64), raw[:, 1].view(np.uint32).astype(np.int64),
                                raw[:, 2].astype(np.int64), raw[:, 3].astype(np.int64)], 1)
            assert np.array_equal(mod._sorted(got), want)
            assert np.array_equal(mod._sorted(mod._host(rows0)), want)
    # torch.bool masks are packed by the wrapper
    tb = [cuda.from_numpy(v).to("cuda:0") for v in (vR, vS, vV)]
    ref = GRef(Rk, Sk, Sv, vR, vS, vV)
    check(hw, ref, cols, tuple(tb), args, ref.counts(orc, args))
    with pytest.raises(ValueError, match="sv_valid"):
        hw.group_join_keys_device(*cols, args, sv_valid=mV.cpu())  # a bitmap on another device than its column


# ------------------------------------------------------------------------------- 6. capacity
@pytest.mark.parametrize("name", ["blocked_packed", "nobloom"])
def test_capacity_with_null_r_rows(hw, cuda, orc, name):
    """GROUP_ALL through the C entries with NULL R rows at capacities 0 (count only), 1, nR - 1 and nR,
    a guard region behind d_out: *n_out == nR every time, 7 exactly below nR, the guard stays, every
    written row is a row and none twice."""
    rng = np.random.default_rng(44)
    Rk, Sk = _distinct(20011), np.concatenate([_distinct(20011)[::2], _distinct(30000, first=20011)])
    vR, vS, vV = rng.random(Rk.size) >= 0.4, rng.random(Sk.size) >= 0.4, rng.random(Sk.size) >= 0.4
    kn._plant(Rk, Sk, vR, vS, rng)
    Sv = _poison(rng.integers(-10**6, 10**6, size=Sk.size), vV)
    ref = GRef(Rk, Sk, Sv, vR, vS, vV)
    assert (~vR).sum() > 1000
    cR, cS, cV = _dev(cuda, Rk), _dev(cuda, Sk), _dev(cuda, Sv)
    mR, mS, mV = _dmask(cuda, vR), _dmask(cuda, vS), _dmask(cuda, vV)
    args = _args(hw)[name]
    a = args._c() if args is not None else None
    nR, GUARD = Rk.size, 0x5A5A5A5A
    for form, entry in (("sum", "hwbrj_join_keys_group_nulls_device"), ("minmax", "hwbrj_join_keys_group_minmax_nulls_device")):
        want = ref.rows(form, True)
        rows = set(map(tuple, want.tolist()))
        for cap in (0, 1, nR - 1, nR):
            buf = cuda.full((cap + 1024, 4), GUARD, dtype=cuda.int32, device="cuda:0")
            n, pairs, st = ctypes.c_uint64(), ctypes.c_uint64(), hw._Stats()
            rc = getattr(hw.lib(), entry)(cR.data_ptr(), mR.data_ptr(), nR, cS.data_ptr(), mS.data_ptr(), cV.data_ptr(),
                                          mV.data_ptr(), Sk.size, ctypes.byref(a) if a is not None else None, hw.GROUP_ALL,
                                          buf.data_ptr() if cap else None, cap, ctypes.byref(n), ctypes.byref(pairs), None,
                                          ctypes.byref(st), None)
            print(f"{form} capacity {cap}: rc {rc}, n_out {n.value} (expected {nR}), pairs {pairs.value}")
            assert (rc, n.value, st.matches, pairs.value) == (7 if cap < nR else 0, nR, nR, ref.n_pairs())
            host = buf.cpu().numpy()
            assert (host[cap:] == GUARD).all()  # nothing past the capacity
            raw = host[:cap]
            if form == "sum":
                first = np.stack([raw[:, 0].astype(np.int64), raw[:, 1].view(np.uint32).astype(np.int64),
                                  np.ascontiguousarray(raw[:, 2:]).view(np.int64).ravel()], 1)
            else:
                first = np.stack([raw[:, 0].astype(np.int64), raw[:, 1].view(np.uint32).astype(np.int64),
                                  raw[:, 2].astype(np.int64), raw[:, 3].astype(np.int64)], 1)
            assert np.unique(first[:, 0]).size == cap
            assert all(tuple(r) in rows for r in first.tolist())
            if cap == nR:
                assert np.array_equal(FORMS[form][0]._sorted(first), want)


# ----------------------------------------------------------------------------------- 7. skew
@pytest.mark.parametrize("name", ["blocked_packed", "basic_k1", "nobloom"])
def test_skew_with_half_of_the_hot_values_null(hw, cuda, orc, name):
    """The hot-key columns of test_gpu_keys_group.test_skewed_partitions (key 77 in a third of R, key
    88 in a tenth of S) with every other value of the hot S key NULL, every fourth hot S key NULL, and
    every other hot R row NULL: the skew path's direct stores and the split jobs."""
    rng = np.random.default_rng(9)
    Rk = np.concatenate([np.full(20000, 77), np.full(100, 88), rng.integers(-5000, 5000, size=40000),
                         [INT_MAX, -INT_MAX - 1]])
    Sk = np.concatenate([np.full(500, 77), np.full(100000, 88), rng.integers(-6000, 6000, size=900000),
                         [INT_MAX, -INT_MAX - 1, 77]])
    rng.shuffle(Rk)
    rng.shuffle(Sk)
    vR, vS, vV = np.ones(Rk.size, bool), np.ones(Sk.size, bool), np.ones(Sk.size, bool)
    vR[np.nonzero((Rk == 77) | (Rk == 88))[0][::2]] = False
    hot = np.nonzero(Sk == 88)[0]
    vV[hot[::2]] = False
    vS[hot[1::4]] = False
    Sv = _poison(rng.integers(-10**6, 10**6, size=Sk.size), vV)
    ref = GRef(Rk, Sk, Sv, vR, vS, vV)
    args = _args(hw)[name]
    got = check(hw, ref, (_dev(cuda, Rk), _dev(cuda, Sk), _dev(cuda, Sv)),
                (_dmask(cuda, vR), _dmask(cuda, vS), _dmask(cuda, vV)), args, ref.counts(orc, args))
    rows = got["sum", hw.GROUP_MATCHED]
    mine = rows[Rk[rows[:, 0]] == 88]
    assert mine.shape[0] == int(((Rk == 88) & vR).sum()) >= 40
    assert (mine[:, 1] == int(((Sk == 88) & vS & vV).sum())).all() and mine[0, 1] == hot.size // 4


# ------------------------------------------------------------------- 8. state between joins
def test_state_between_joins(hw, cuda, orc):
    """On one engine, without a filter: a masked group join, the unmasked one, a masked counting join,
    and the masked group join again. Each reports its own `filtered`: the participating S rows, |S|,
    S's valid keys, and the participating S rows again."""
    rng = np.random.default_rng(77)
    Rk, Sk = _distinct(50021), np.concatenate([_distinct(50021)[::2], _distinct(90000, first=50021)])
    vR, vS, vV = rng.random(Rk.size) >= 0.25, rng.random(Sk.size) >= 0.25, rng.random(Sk.size) >= 0.25
    kn._plant(Rk, Sk, vR, vS, rng)
    Sv = _poison(rng.integers(-10**6, 10**6, size=Sk.size), vV)
    cols = (_dev(cuda, Rk), _dev(cuda, Sk), _dev(cuda, Sv))
    masks = (_dmask(cuda, vR), _dmask(cuda, vS), _dmask(cuda, vV))
    masked, only_v, plain = GRef(Rk, Sk, Sv, vR, vS, vV), GRef(Rk, Sk, Sv, None, None, vV), GRef(Rk, Sk, Sv)
    mc, vc, pc = masked.counts(orc, None), only_v.counts(orc, None), plain.counts(orc, None)
    assert mc[0] == int((vS & vV).sum()) and vc[0] == int(vV.sum()) and pc[0] == Sk.size
    counting = kn.NRef(orc, Rk, Sk, vR, vS)
    for _ in range(2):
        check(hw, masked, cols, masks, None, mc)
        check(hw, plain, cols, (None, None, None), None, pc)
        st = hw.join_keys_device(cols[0], cols[1], None, r_valid=masks[0], s_valid=masks[1])
        assert (st.filtered, st.matches) == (int(vS.sum()), counting.pairs.shape[0])
        check(hw, only_v, cols, (None, None, masks[2]), None, vc)
        check(hw, plain, cols, (None, None, None), None, pc)
    check(hw, masked, cols, masks, None, mc)
