"""Key columns with validity bitmaps (r_valid / s_valid of hw.join_keys_device, hw.join_keys_pairs_device,
hw.semi_join_keys_device and hw.outer_join_keys_device) against the oracle and numpy.

Every expectation is computed from {key, original row} tuples of the valid rows only: pairs from
orc.join_pairs, `filtered` and the match count from orc.bpro on those compacted relations, existence
and class rows from np.isin, and the NULL rows added as the header states (anti, outer). Nothing is
compared with the code under test alone.

The keys stored under NULL rows equal live keys of the other side, mixed with keys that occur nowhere
else: a kernel that ignores a mask bit produces extra pairs or loses anti rows, it cannot pass by luck."""
import ctypes

import numpy as np
import pytest

import shapes
import test_gpu_shapes as gs
from test_gpu_keys_pairs import _counts, _u64
from test_gpu_materialize import _args

pytestmark = pytest.mark.gpu

INT_MIN, INT_MAX = -2**31, 2**31 - 1
SUPPORTED = ["blocked_packed", "blocked_code", "blocked_k3", "sectorized_k2", "basic_k1", "two_segments", "nobloom"]
REFUSED = ["global_b4", "basic_k3"]
A, C = 0x9E3779B1, 0x7F4A7C15  # i -> i * A + C mod 2^32: distinct keys


def _distinct(n, first=0):
    return ((np.arange(first, first + n, dtype=np.uint64) * A + C) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def _dcol(cuda, keys):
    """A key column in a device allocation of exactly its size."""
    keys = np.ascontiguousarray(np.asarray(keys).astype(np.int64).astype(np.int32))
    c = cuda.empty(keys.size, dtype=cuda.int32, device="cuda:0")
    c.copy_(cuda.from_numpy(keys))
    cuda.cuda.synchronize()
    return c


def _dmask(cuda, valid, tail=0):
    """The bitmap of `valid` in a device allocation of exactly ceil(n / 32) * 4 bytes; the bits past n
    in the last byte (and the padding bytes) all clear (tail = 0) or all set (tail = 1)."""
    n = valid.size
    bits = np.full((n + 31) // 32 * 32, bool(tail))
    bits[:n] = valid
    b = np.packbits(bits, bitorder="little")
    m = cuda.empty(b.size, dtype=cuda.uint8, device="cuda:0")
    m.copy_(cuda.from_numpy(b))
    cuda.cuda.synchronize()
    assert m.data_ptr() % 4 == 0
    return m


def _rows(a, b):
    return np.stack([np.asarray(a), np.asarray(b)], 1).astype(np.int32).reshape(-1, 2)


class NRef:
    """What the joins of the key columns Rk, Sk with validity vR, vS (bool arrays; None: all valid)
    must return: the tuple joins' results on {key, original row} of the valid rows, plus the NULL rows."""

    def __init__(self, orc, Rk, Sk, vR=None, vS=None):
        self.Rk = np.asarray(Rk).astype(np.int64).astype(np.int32)
        self.Sk = np.asarray(Sk).astype(np.int64).astype(np.int32)
        self.vR = np.ones(self.Rk.size, bool) if vR is None else np.asarray(vR, bool)
        self.vS = np.ones(self.Sk.size, bool) if vS is None else np.asarray(vS, bool)
        rR, rS = np.nonzero(self.vR)[0], np.nonzero(self.vS)[0]
        self.R, self.S = _rows(self.Rk[rR], rR), _rows(self.Sk[rS], rS)  # the compacted relations
        both = self.R.shape[0] and self.S.shape[0]
        self.pairs = orc.join_pairs(self.R, self.S).reshape(-1, 2) if both else np.empty((0, 2), dtype=np.int32)
        s_hit, r_hit = np.isin(self.S[:, 0], self.R[:, 0]), np.isin(self.R[:, 0], self.S[:, 0])
        self.semi = rS[s_hit]
        self.anti = np.sort(np.concatenate([rS[~s_hit], np.nonzero(~self.vS)[0]]))  # NULL S rows: no partner
        self.r_only = np.sort(np.concatenate([rR[~r_hit], np.nonzero(~self.vR)[0]]))
        self.upairs = _u64(self.pairs)

    def counts(self, orc, args):
        """(filtered, matches) of the counting join on the compacted relations."""
        if self.R.shape[0] == 0 or self.S.shape[0] == 0:
            return None  # (checked by the callers that know what an empty side gives)
        return _counts(orc, self.R, self.S, args)


def check(hw, ref, cR, cS, mR, mS, args, counts=None, outer=None, what=("count", "pairs", "semi", "anti", "outer")):
    kw = dict(r_valid=mR, s_valid=mS)
    n_pairs = ref.pairs.shape[0]
    if "count" in what:
        st = hw.join_keys_device(cR, cS, args, **kw)
        print(f"count: filtered {st.filtered} matches {st.matches} (oracle {counts}, pairs {n_pairs})")
        assert st.matches == n_pairs
        if counts is not None:
            assert (st.filtered, st.matches) == counts
    if "pairs" in what:
        st, pairs, _ = hw.join_keys_pairs_device(cR, cS, args, **kw)
        p = pairs.cpu().numpy()
        print(f"pairs: {p.shape[0]} rows (oracle {n_pairs}), filtered {st.filtered} (oracle {counts})")
        assert st.matches == p.shape[0] == n_pairs
        assert np.array_equal(ref.Rk[p[:, 0]], ref.Sk[p[:, 1]])        # every pair joins equal keys
        assert ref.vR[p[:, 0]].all() and ref.vS[p[:, 1]].all()         # of valid rows
        assert np.array_equal(_u64(p), ref.upairs)
        if counts is not None:
            assert (st.filtered, st.matches) == counts
    for anti in (False, True):
        if ("anti" if anti else "semi") not in what:
            continue
        st, rows, _ = hw.semi_join_keys_device(cR, cS, args, anti=anti, **kw)
        r = rows.cpu().numpy()
        want = ref.anti if anti else ref.semi
        print(f"anti={anti}: {r.shape[0]} rows (numpy {want.size}), filtered {st.filtered} (oracle {counts})")
        assert st.matches == r.shape[0] == want.size
        assert np.array_equal(ref.Sk[r[:, 1]], r[:, 0])  # the key field: what the column stores there
        assert np.array_equal(np.sort(r[:, 1]), want)
        if counts is not None:
            assert st.filtered == counts[0]
    if "outer" in what:
        s_rows, r_rows = _rows(np.full(ref.anti.size, -1), ref.anti), _rows(ref.r_only, np.full(ref.r_only.size, -1))
        for kind in outer if outer is not None else (hw.OUTER_S, hw.OUTER_R, hw.OUTER_FULL):
            parts = [ref.pairs] + ([s_rows] if kind != hw.OUTER_R else []) + ([r_rows] if kind != hw.OUTER_S else [])
            want_cls = (n_pairs, s_rows.shape[0] if kind != hw.OUTER_R else 0, r_rows.shape[0] if kind != hw.OUTER_S else 0)
            st, rows, cls, _ = hw.outer_join_keys_device(cR, cS, args, kind=kind, **kw)
            r = rows.cpu().numpy()
            print(f"outer {kind}: {r.shape[0]} rows, classes {cls} (numpy {want_cls}), filtered {st.filtered}")
            assert cls == want_cls
            assert st.matches == r.shape[0] == sum(cls)
            assert np.array_equal(_u64(r), _u64(np.concatenate(parts)))
            if counts is not None:
                assert st.filtered == counts[0]


def _plant(Rk, Sk, vR, vS, rng):
    """The central trick: under NULL rows, alternately a live key of the other side and an absent key."""
    nr, ns = np.nonzero(~vR)[0], np.nonzero(~vS)[0]
    liveR, liveS = Rk[vR], Sk[vS]
    absent = -(np.arange(nr.size + ns.size, dtype=np.int64) + 7) * 2654435761 % (2**31)  # (any keys; mostly absent)
    if liveS.size:
        Rk[nr[::2]] = rng.choice(liveS, size=nr[::2].size)
    Rk[nr[1::2]] = absent[: nr[1::2].size]
    if liveR.size:
        Sk[ns[::2]] = rng.choice(liveR, size=ns[::2].size)
    Sk[ns[1::2]] = absent[nr.size: nr.size + ns[1::2].size]


def _G(hw, cuda):
    """(G, round) of the scatters, counting and payload alike (one workgroup per CU each)."""
    a, b = gs.geometry(hw, cuda, None, 8), gs.geometry(hw, cuda, None, 8, mat=True)
    assert a["G"] == b["G"] and a["sc_round"] == b["sc_round"] == 1024 * 8
    return a["G"], a["sc_round"]


def _e0(n, G):
    return np.array([shapes.wg_range(n, G, w)[0] for w in range(G)], dtype=np.int64)


# ------------------------------------------------------------------------------ 1. every mode
_MODE = {}


def _mode_case(orc, cuda):
    if not _MODE:
        R = orc.relation(400000, 2, 400000, 400000, 1.0, 1)
        S = orc.relation(3000000, 2, INT_MAX, 400000, 0.2, 2)
        rng = np.random.default_rng(20)
        Rk, Sk = R[:, 0].copy(), S[:, 0].copy()
        vR, vS = rng.random(Rk.size) >= 0.2, rng.random(Sk.size) >= 0.2
        _plant(Rk, Sk, vR, vS, rng)
        ref = NRef(orc, Rk, Sk, vR, vS)
        assert 0 < ref.pairs.shape[0] < np.isin(Sk, Rk).sum()  # ignoring the masks would give more
        _MODE.update(ref=ref, cR=_dcol(cuda, Rk), cS=_dcol(cuda, Sk), mR=_dmask(cuda, vR), mS=_dmask(cuda, vS), counts={})
    return _MODE


def _mode_counts(orc, M, name, args):
    if name not in M["counts"]:
        M["counts"][name] = M["ref"].counts(orc, args)
    return M["counts"][name]


@pytest.mark.parametrize("what", ["count_pairs", "semi_anti", "outer"])
@pytest.mark.parametrize("name", SUPPORTED)
def test_every_supported_mode(hw, cuda, orc, name, what):
    """R 400,000 / S 3,000,000, about one row in five NULL on each side."""
    M = _mode_case(orc, cuda)
    args = _args(hw)[name]
    check(hw, M["ref"], M["cR"], M["cS"], M["mR"], M["mS"], args, _mode_counts(orc, M, name, args),
          what={"count_pairs": ("count", "pairs"), "semi_anti": ("semi", "anti"), "outer": ("outer",)}[what])


@pytest.mark.parametrize("name", REFUSED)
def test_unsupported_modes_raise_9(hw, cuda, orc, name):
    M = _mode_case(orc, cuda)
    args = _args(hw)[name]
    for kw in (dict(r_valid=M["mR"]), dict(s_valid=M["mS"]), dict(r_valid=M["mR"], s_valid=M["mS"])):
        for fn in (hw.join_keys_device, hw.join_keys_pairs_device, hw.semi_join_keys_device, hw.outer_join_keys_device):
            with pytest.raises(RuntimeError, match=r"\(9\)"):
                fn(M["cR"], M["cS"], args, **kw)


# ------------------------------------------------------------------ 2. full rounds with NULLs
PATTERNS = [0x55, 0xAA, 0x0F, 0xF0, 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80, 0xFF, 0x00]
_FULL = {}


def _full_case(hw, cuda, side):
    if side not in _FULL:
        G, rnd = _G(hw, cuda)
        n = 2 * G * rnd + 5
        e0 = _e0(n, G)
        # every workgroup has a full round, and the ranges start at odd nibbles and off dword boundaries
        assert np.all(np.diff(np.append(e0, n)) >= rnd)
        assert np.any(e0 % 8 == 4) and np.any(e0 % 32 != 0)
        big = _distinct(n)
        other = np.concatenate([big[::97], _distinct(500, first=n)])
        np.random.default_rng(n).shuffle(other)
        vo = np.random.default_rng(5).random(other.size) >= 0.2
        _FULL[side] = dict(big=big, other=other, vo=vo, cb=_dcol(cuda, big), co=_dcol(cuda, other), mo=_dmask(cuda, vo))
    return _FULL[side]


@pytest.mark.parametrize("side", ["R", "S"])
@pytest.mark.parametrize("pattern", PATTERNS, ids=[f"0x{p:02X}" for p in PATTERNS])
def test_full_rounds_with_nulls(hw, cuda, orc, pattern, side):
    """2 G round + 5 distinct keys whose bitmap repeats one byte (0xFF: all valid, 0x00: all NULL); the
    other side holds every 97th key, valid or not, and 500 absent ones, a fifth of its rows NULL."""
    F = _full_case(hw, cuda, side)
    n = F["big"].size
    vb = np.unpackbits(np.full((n + 7) // 8, pattern, dtype=np.uint8), bitorder="little")[:n].astype(bool)
    mb = _dmask(cuda, vb)
    if side == "R":
        ref, cols = NRef(orc, F["big"], F["other"], vb, F["vo"]), (F["cb"], F["co"], mb, F["mo"])
    else:
        ref, cols = NRef(orc, F["other"], F["big"], F["vo"], vb), (F["co"], F["cb"], F["mo"], mb)
    for name in ("nobloom", "blocked_packed"):
        args = _args(hw)[name]
        check(hw, ref, *cols, args, ref.counts(orc, args), outer=(hw.OUTER_FULL,))


# ------------------------------------------------------------------------------- 3. edges
EDGE_N = ["1", "2", "3", "4", "5", "31", "32", "33", "4G-1", "4G", "4G+1", "G*round-1", "G*round", "G*round+1"]


def _edge_n(hw, cuda, nspec):
    G, rnd = _G(hw, cuda)
    return {"4G-1": 4 * G - 1, "4G": 4 * G, "4G+1": 4 * G + 1, "G*round-1": G * rnd - 1, "G*round": G * rnd,
            "G*round+1": G * rnd + 1}.get(nspec) or int(nspec), G


@pytest.mark.parametrize("side", ["R", "S"])
@pytest.mark.parametrize("nspec", EDGE_N)
def test_nulls_at_every_edge(hw, cuda, orc, nspec, side):
    """A column of exactly n distinct keys and a bitmap of exactly ceil(n / 32) * 4 bytes. Four masks:
    the only NULL at row 0; at row n - 1; one NULL at the last row of every workgroup's range (e0 - 1);
    one at the first row of every range (e0). Each with the bits past n all clear and all set: the
    same result. The other side holds every 3rd key (n < 100) or every 97th, and absent ones."""
    n, G = _edge_n(hw, cuda, nspec)
    big = _distinct(n)
    other = np.concatenate([big[:: 3 if n < 100 else 97], _distinct(50, first=n)])
    np.random.default_rng(n).shuffle(other)
    co, cb = _dcol(cuda, other), _dcol(cuda, big)
    e0 = np.unique(_e0(n, G))
    masks = {"row 0": [0], "row n-1": [n - 1], "every e0-1": e0[e0 > 0] - 1, "every e0": e0[e0 < n]}
    for what, null_rows in masks.items():
        vb = np.ones(n, bool)
        vb[np.asarray(null_rows, dtype=np.int64)] = False
        ref = NRef(orc, big, other, vb, None) if side == "R" else NRef(orc, other, big, None, vb)
        for tail in (0, 1):
            mb = _dmask(cuda, vb, tail)
            assert mb.numel() == (n + 31) // 32 * 4
            cols = (cb, co, mb, None) if side == "R" else (co, cb, None, mb)
            print(f"-- {what}, tail bits {tail}")
            for name in ("nobloom", "blocked_packed"):
                check(hw, ref, *cols, _args(hw)[name], outer=(hw.OUTER_FULL,))


# ------------------------------------------------------------- 4. range and partition coverage
def test_one_workgroups_whole_range_is_null(hw, cuda, orc):
    G, rnd = _G(hw, cuda)
    n = G * rnd + 12
    big, w = _distinct(n), G // 3
    lo, hi = shapes.wg_range(n, G, w)
    assert hi - lo >= rnd
    vb = np.ones(n, bool)
    vb[lo:hi] = False
    other = np.concatenate([big[::53], _distinct(300, first=n)])
    for side in ("R", "S"):
        ref = NRef(orc, big, other, vb, None) if side == "R" else NRef(orc, other, big, None, vb)
        cols = (_dcol(cuda, big), _dcol(cuda, other), _dmask(cuda, vb), None)
        cols = cols if side == "R" else (cols[1], cols[0], None, cols[2])
        for name in ("nobloom", "blocked_packed"):
            args = _args(hw)[name]
            check(hw, ref, *cols, args, ref.counts(orc, args), outer=(hw.OUTER_FULL,))


def test_a_partition_whose_only_rows_are_null(hw, cuda, orc):
    """PRO and the blocked filter partition by the code's low 10 bits: every row of partition 5, on both
    sides, is NULL, and those rows hold keys that the other side has as well."""
    crc = shapes.Crc(orc.crc)
    info = gs.geometry(hw, cuda, None, 8, mat=True)
    assert info["F"] == 1024
    Rk, Sk = _distinct(300000), np.concatenate([_distinct(300000)[::2], _distinct(200000, first=300000)])
    vR, vS = (crc.code(Rk) & 1023) != 5, (crc.code(Sk) & 1023) != 5
    assert (~vR).sum() > 100 and (~vS).sum() > 100 and np.isin(Sk[~vS], Rk[~vR]).any()
    ref = NRef(orc, Rk, Sk, vR, vS)
    cols = (_dcol(cuda, Rk), _dcol(cuda, Sk), _dmask(cuda, vR), _dmask(cuda, vS))
    for name in ("nobloom", "blocked_packed"):
        args = _args(hw)[name]
        check(hw, ref, *cols, args, ref.counts(orc, args))


@pytest.mark.parametrize("name", ["nobloom", "blocked_packed", "basic_k1"])
def test_one_side_all_null(hw, cuda, orc, name):
    Rk, Sk = _distinct(70001), np.concatenate([_distinct(70001)[::3], _distinct(50000, first=70001)])
    nR, nS = Rk.size, Sk.size
    cR, cS = _dcol(cuda, Rk), _dcol(cuda, Sk)
    args = _args(hw)[name]
    none_r, none_s = _dmask(cuda, np.zeros(nR, bool)), _dmask(cuda, np.zeros(nS, bool))
    # S all NULL: no pairs, anti = all of S, OUTER_FULL = nR + nS rows
    ref = NRef(orc, Rk, Sk, None, np.zeros(nS, bool))
    assert ref.pairs.shape[0] == 0 and ref.anti.size == nS and ref.r_only.size == nR
    check(hw, ref, cR, cS, None, none_s, args)
    st = hw.join_keys_device(cR, cS, args, s_valid=none_s)
    assert (st.filtered, st.matches) == (0, 0)
    # R all NULL: the filter is empty, so it passes nothing (no filter: every S row "passes")
    ref = NRef(orc, Rk, Sk, np.zeros(nR, bool), None)
    assert ref.pairs.shape[0] == 0 and ref.anti.size == nS and ref.r_only.size == nR
    check(hw, ref, cR, cS, none_r, None, args)
    empty = np.empty((0, 2), dtype=np.int32)
    want = _counts(orc, empty, ref.S, args)
    print("R all NULL: oracle on an empty R", want)
    assert want == ((nS if args is None else 0), 0)
    st = hw.join_keys_device(cR, cS, args, r_valid=none_r)
    assert (st.filtered, st.matches) == want


# ------------------------------------------------------------------------- 5. one side only
def test_one_side_only_and_no_masks(hw, cuda, orc):
    rng = np.random.default_rng(31)
    Rk, Sk = _distinct(100003), np.concatenate([_distinct(100003)[::2], _distinct(300000, first=100003)])
    rng.shuffle(Sk)
    vR, vS = rng.random(Rk.size) >= 0.3, rng.random(Sk.size) >= 0.3
    _plant(Rk, Sk, vR, vS, rng)
    cR, cS, mR, mS = _dcol(cuda, Rk), _dcol(cuda, Sk), _dmask(cuda, vR), _dmask(cuda, vS)
    args = _args(hw)["blocked_packed"]
    for ref, mr, ms in ((NRef(orc, Rk, Sk, vR, None), mR, None), (NRef(orc, Rk, Sk, None, vS), None, mS)):
        check(hw, ref, cR, cS, mr, ms, args, ref.counts(orc, args))
    # no masks: the unmasked call's result and tables; an all-valid bitmap: its rows
    ref = NRef(orc, Rk, Sk)
    tabs = []
    for kw in ({}, dict(r_valid=None, s_valid=None)):
        st = hw.join_keys_device(cR, cS, args, **kw)
        info = hw.tables_info()
        tabs.append((st.filtered, st.matches, {k: info[k] for k in gs.GEOM}, hw.tables_read(hw.TAB_R_ELEM_START),
                     hw.tables_read(hw.TAB_S_ELEM_START)))
    assert tabs[0][:3] == tabs[1][:3] and (tabs[0][0], tabs[0][1]) == ref.counts(orc, args)
    assert np.array_equal(tabs[0][3], tabs[1][3]) and np.array_equal(tabs[0][4], tabs[1][4])
    check(hw, ref, cR, cS, None, None, args, ref.counts(orc, args))
    allR, allS = _dmask(cuda, np.ones(Rk.size, bool)), _dmask(cuda, np.ones(Sk.size, bool))
    check(hw, ref, cR, cS, allR, allS, args, ref.counts(orc, args))
    # a torch.bool tensor is packed by the wrapper
    check(hw, NRef(orc, Rk, Sk, vR, vS), cR, cS, cuda.from_numpy(vR).to("cuda:0"), cuda.from_numpy(vS).to("cuda:0"), args,
          what=("count", "pairs", "anti"))
    got = hw.pack_validity(cuda.from_numpy(vS).to("cuda:0"))
    assert got.is_cuda and np.array_equal(got.cpu().numpy()[: (Sk.size + 7) // 8], np.packbits(vS, bitorder="little"))
    with pytest.raises(ValueError, match="s_valid"):
        hw.join_keys_device(cR, cS, args, s_valid=mS.cpu())  # a bitmap on another device than its column


# ----------------------------------------------------------------------------------- 6. skew
@pytest.mark.parametrize("name", ["blocked_packed", "basic_k1", "nobloom"])
def test_skew_with_half_of_the_hot_rows_null(hw, cuda, orc, name):
    """The hot-key relations of test_gpu_keys_pairs.test_pairs_skewed_partitions (key 77 in a third of
    R, key 88 in a tenth of S) with every other hot row NULL."""
    rng = np.random.default_rng(9)
    Rk = np.concatenate([np.full(20000, 77), np.full(100, 88), rng.integers(-5000, 5000, size=40000),
                         [INT_MAX, -INT_MAX - 1]])
    Sk = np.concatenate([np.full(500, 77), np.full(100000, 88), rng.integers(-6000, 6000, size=900000),
                         [INT_MAX, -INT_MAX - 1, 77]])
    rng.shuffle(Rk)
    rng.shuffle(Sk)
    vR, vS = np.ones(Rk.size, bool), np.ones(Sk.size, bool)
    for k, v in ((Rk, vR), (Sk, vS)):
        hot = np.nonzero((k == 77) | (k == 88))[0]
        v[hot[::2]] = False
    ref = NRef(orc, Rk, Sk, vR, vS)
    args = _args(hw)[name]
    check(hw, ref, _dcol(cuda, Rk), _dcol(cuda, Sk), _dmask(cuda, vR), _dmask(cuda, vS), args, ref.counts(orc, args),
          outer=(hw.OUTER_FULL,))


# ------------------------------------------------------------------------------- 7. capacity
@pytest.mark.parametrize("name", ["blocked_packed", "nobloom"])
def test_capacity_with_null_rows(hw, cuda, orc, name):
    """Anti and OUTER_FULL through the C entries at capacities 0 (count only), 1, n - 1 and n, a guard
    region after the buffer: the guard stays, *n_out is the full count, 7 above capacity, and what is
    written is a sub-multiset of the expected rows."""
    rng = np.random.default_rng(44)
    Rk, Sk = _distinct(20011), np.concatenate([_distinct(20011)[::2], _distinct(30000, first=20011)])
    vR, vS = rng.random(Rk.size) >= 0.4, rng.random(Sk.size) >= 0.4
    _plant(Rk, Sk, vR, vS, rng)
    ref = NRef(orc, Rk, Sk, vR, vS)
    cR, cS, mR, mS = _dcol(cuda, Rk), _dcol(cuda, Sk), _dmask(cuda, vR), _dmask(cuda, vS)
    args = _args(hw)[name]
    a = args._c() if args is not None else None
    L = hw.lib()
    ptrs = (cR.data_ptr(), mR.data_ptr(), cR.shape[0], cS.data_ptr(), mS.data_ptr(), cS.shape[0],
            ctypes.byref(a) if a is not None else None)
    anti_rows = _rows(Sk[ref.anti], ref.anti)
    full_rows = np.concatenate([ref.pairs, _rows(np.full(ref.anti.size, -1), ref.anti),
                                _rows(ref.r_only, np.full(ref.r_only.size, -1))])
    assert (~vS).sum() > 1000 and (~vR).sum() > 1000
    GUARD = 64
    for entry, want in (("anti", anti_rows), ("full", full_rows)):
        n_all, uwant = want.shape[0], _u64(want)
        for cap in (0, 1, n_all - 1, n_all):
            out = cuda.full((cap + GUARD, 2), 0x5A5A5A5A, dtype=cuda.int32, device="cuda:0")
            n = ctypes.c_uint64()
            op = out.data_ptr() if cap else None
            if entry == "anti":
                rc = L.hwbrj_join_keys_semi_nulls_device(*ptrs, hw.JOIN_ANTI, op, cap, ctypes.byref(n), None, None, None)
            else:
                cls = (ctypes.c_uint64 * 3)()
                rc = L.hwbrj_join_keys_outer_nulls_device(*ptrs, hw.OUTER_FULL, op, cap, ctypes.byref(n), cls, None,
                                                          None, None)
                assert tuple(cls) == (ref.pairs.shape[0], ref.anti.size, ref.r_only.size)
            got = out.cpu().numpy()
            print(f"{entry} capacity {cap}: rc {rc}, n_out {n.value} (expected {n_all})")
            assert (rc, n.value) == (7 if cap < n_all else 0, n_all)
            assert np.all(got[cap:] == 0x5A5A5A5A)  # nothing beyond the capacity
            ugot = _u64(got[:cap])
            if cap == n_all:
                assert np.array_equal(ugot, uwant)
            else:  # a sub-multiset: no row more often than expected
                vals, cnt = np.unique(ugot, return_counts=True)
                wv, wc = np.unique(uwant, return_counts=True)
                pos = np.searchsorted(wv, vals)
                assert np.all(pos < wv.size) and np.array_equal(wv[np.minimum(pos, wv.size - 1)], vals)
                assert np.all(cnt <= wc[pos])


# ----------------------------------------------------------------------------- 8. neighbours
def test_masked_and_unmasked_joins_side_by_side(hw, cuda, orc):
    """A masked join, an unmasked join of other columns, and the masked one again: each its own result."""
    rng = np.random.default_rng(77)
    Rk, Sk = _distinct(50021), np.concatenate([_distinct(50021)[::2], _distinct(90000, first=50021)])
    vR, vS = rng.random(Rk.size) >= 0.25, rng.random(Sk.size) >= 0.25
    _plant(Rk, Sk, vR, vS, rng)
    Rk2, Sk2 = _distinct(33333, first=10**6), np.concatenate([_distinct(33333, first=10**6)[::3], _distinct(70000, first=2 * 10**6)])
    masked, plain = NRef(orc, Rk, Sk, vR, vS), NRef(orc, Rk2, Sk2)
    m_cols = (_dcol(cuda, Rk), _dcol(cuda, Sk), _dmask(cuda, vR), _dmask(cuda, vS))
    p_cols = (_dcol(cuda, Rk2), _dcol(cuda, Sk2), None, None)
    args = _args(hw)["blocked_packed"]
    mc, pc = masked.counts(orc, args), plain.counts(orc, args)
    for what in (("count",), ("pairs",), ("anti",), ("outer",)):
        check(hw, masked, *m_cols, args, mc, outer=(hw.OUTER_FULL,), what=what)
        check(hw, plain, *p_cols, args, pc, outer=(hw.OUTER_FULL,), what=what)
        check(hw, masked, *m_cols, args, mc, outer=(hw.OUTER_FULL,), what=what)
