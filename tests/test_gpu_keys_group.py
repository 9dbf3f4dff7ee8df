"""The group joins on key columns with an S value column (hw.group_join_keys_device,
hw.group_minmax_join_keys_device).

Every expectation is test_gpu_group.reference (COUNT, SUM) or test_gpu_group_minmax.reference
(COUNT, MIN, MAX), the host references of the tuple entries, applied to R = stack(Rk, arange) and
S = stack(Sk, Sv): the tuples a caller without these entries would have had to write. Rows are
compared exactly after sorting by r_payload, both kinds in every case. Every case also checks n_pairs
and `filtered` against join_keys_device of the same columns, and that the tuple entry on the
interleaved tensors returns the column entry's rows. Columns live in allocations of exactly their
size, so a load past a column's end is not covered by padding."""
import ctypes

import numpy as np
import pytest

import shapes
import test_gpu_group as g
import test_gpu_group_minmax as mm
import test_gpu_keys_pairs as kp
import test_gpu_outer as t
from test_gpu_materialize import _args

pytestmark = pytest.mark.gpu

INT_MIN, INT_MAX = -2**31, 2**31 - 1
FORMS = {
    "sum": (g, "group_join_keys_device", "group_join_device"),
    "minmax": (mm, "group_minmax_join_keys_device", "group_minmax_join_device"),
}


def _i32(a):
    return np.asarray(a).astype(np.int64).astype(np.int32).ravel()


def _tuples(keys, pay):
    return np.stack([_i32(keys), _i32(pay)], 1).reshape(-1, 2)


def _dev(cuda, a):
    """A 1-D int32 column in a device allocation of exactly its size."""
    a = _i32(a)
    c = cuda.empty(a.size, dtype=cuda.int32, device="cuda:0")
    c.copy_(cuda.from_numpy(np.ascontiguousarray(a)))
    cuda.cuda.synchronize()
    return c


_REF = {}


def _reference(mod, R, S, tag):
    if tag is not None and tag in _REF:
        return _REF[tag]
    ref = mod._sorted(mod.reference(R, S))
    ref.setflags(write=False)
    if tag is not None:
        _REF[tag] = ref
    return ref


def check(hw, cuda, Rk, Sk, Sv, args, forms=("sum", "minmax"), tag=None, cols=None, **kw):
    """Both kinds of every form against the host reference of the interleaved tuples; returns
    {form: {kind: rows sorted by r_payload}}."""
    Rk, Sk, Sv = _i32(Rk), _i32(Sk), _i32(Sv)
    R, S = _tuples(Rk, np.arange(Rk.size)), _tuples(Sk, Sv)
    cR, cS, cV = cols if cols is not None else (_dev(cuda, Rk), _dev(cuda, Sk), _dev(cuda, Sv))
    dR, dS = t.to_dev(cuda, R), t.to_dev(cuda, S)
    cj = hw.join_keys_device(cR, cS, args)
    out = {}
    for form in forms:
        mod, col_fn, tup_fn = FORMS[form]
        ref = _reference(mod, R, S, None if tag is None else (tag, form))
        got = {}
        for kind in (hw.GROUP_MATCHED, hw.GROUP_ALL):
            want = ref if kind == hw.GROUP_ALL else ref[ref[:, 1] > 0]
            st, rows, pairs, _ = getattr(hw, col_fn)(cR, cS, cV, args, kind=kind, **kw)
            rows = mod._sorted(mod._host(rows))
            print(f"{form} kind {kind}: {rows.shape[0]} rows (host {want.shape[0]}), n_pairs {pairs} (host "
                  f"{int(ref[:, 1].sum())}, counting join {cj.matches}), filtered {st.filtered} (counting join "
                  f"{cj.filtered})")
            assert rows.shape[0] == want.shape[0] == st.matches
            assert pairs == cj.matches == int(ref[:, 1].sum())
            assert st.filtered == cj.filtered
            assert np.array_equal(rows, want)
            _, trows, tpairs, _ = getattr(hw, tup_fn)(dR, dS, args, kind=kind)
            assert tpairs == pairs and np.array_equal(mod._sorted(mod._host(trows)), rows)
            got[kind] = rows
        assert got[hw.GROUP_ALL].shape[0] == Rk.size
        assert np.array_equal(got[hw.GROUP_MATCHED], got[hw.GROUP_ALL][got[hw.GROUP_ALL][:, 1] > 0])
        out[form] = got
    return out


@pytest.fixture(scope="module")
def crc(orc):
    return shapes.Crc(orc.crc)


# ------------------------------------------------------------------------------ 1. every mode
_MODE = {}


def _mode_case(orc, cuda):
    """The relations of test_gpu_keys_pairs._mode_case (|R| = 400,000, |S| = 3,000,000: at G = 256
    every S scatter workgroup gets one full round and a partial one) with random values."""
    if not _MODE:
        R = orc.relation(400000, 2, 400000, 400000, 1.0, 1)
        S = orc.relation(3000000, 2, INT_MAX, 400000, 0.2, 2)
        Sv = np.random.default_rng(17).integers(INT_MIN, INT_MAX, size=S.shape[0], endpoint=True)
        Rk, Sk, Sv = _i32(R[:, 0]), _i32(S[:, 0]), _i32(Sv)
        _MODE.update(Rk=Rk, Sk=Sk, Sv=Sv, cols=(_dev(cuda, Rk), _dev(cuda, Sk), _dev(cuda, Sv)))
    return _MODE


@pytest.mark.parametrize("form", ["sum", "minmax"])
@pytest.mark.parametrize("name", kp.MODES)
def test_every_mode(hw, cuda, orc, name, form):
    c = _mode_case(orc, cuda)
    got = check(hw, cuda, c["Rk"], c["Sk"], c["Sv"], _args(hw)[name], forms=(form,), tag="every_mode", cols=c["cols"])
    assert got[form][hw.GROUP_MATCHED].shape[0] == int(np.isin(c["Rk"], c["Sk"]).sum()) >= 1000


# ------------------------------------------------------- 2. the value at every range edge
A, C = kp.A, kp.C
A2, C2 = 0x85EBCA6B, 0x27D4EB2F


def _edge_keys(n):
    """n + 500 distinct keys; the first n (the big column) end in INT32_MIN, INT32_MAX, 0 and -1."""
    k = ((np.arange(n + 500, dtype=np.uint64) * A + C) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    big = k[:n].copy()
    special = np.array([INT_MIN, INT_MAX, 0, -1], dtype=np.int32)
    big[-min(n, 4):] = np.roll(special, n)[-min(n, 4):]
    return big, k[n:]


def _edge_values(n):
    """An injective i -> value (a bijection of 2^32 restricted to [0, n)), with INT32_MAX at the last
    position and INT32_MIN at the one before it (swapped in, so it stays injective)."""
    v = ((np.arange(n, dtype=np.uint64) * A2 + C2) & 0xFFFFFFFF).astype(np.uint32).view(np.int32).copy()
    for pos, val in ((n - 1, INT_MAX), (n - 2, INT_MIN)):
        if pos < 0:
            continue
        at = np.nonzero(v == val)[0]
        if at.size and at[0] != pos:
            v[at[0]] = v[pos]
        v[pos] = val
    assert np.unique(v).size == n
    return v


@pytest.mark.parametrize("side", ["S", "R"])
@pytest.mark.parametrize("nspec", kp.EDGE_N)
def test_value_at_every_range_edge(hw, cuda, nspec, side):
    """A column of exactly n distinct keys ending in INT32_MIN, INT32_MAX, 0 and -1; the other side
    holds every 97th of them and 500 absent keys, so every matched group has one member. side S: the
    big column is S with an injective value column; every matched R row's sum, min and max must be
    the one value at its key's position in S: what goes wrong if the value load's base, round offset
    or four-per-load index shape differs from the key load's. side R: the big column is R, and
    r_payload must name the position of the row's key. PRO and a blocked filter with packed words."""
    n = kp._edge_n(hw, cuda, nspec)
    big, absent = _edge_keys(n)
    other = np.concatenate([big[::97], absent])
    np.random.default_rng(n).shuffle(other)
    if side == "S":
        Rk, Sk, Sv = other, big, _edge_values(n)
    else:
        Rk, Sk, Sv = big, other, _edge_values(other.size)
    assert np.unique(Sk).size == Sk.size and np.unique(Rk).size == Rk.size
    if Sv.size >= 2:
        assert {INT_MIN, INT_MAX} <= set(Sv[-4:].tolist())
    order = np.argsort(Sk, kind="stable")
    n_hit = int(np.isin(Rk, Sk).sum())
    assert n_hit >= (n + 96) // 97
    cols = (_dev(cuda, Rk), _dev(cuda, Sk), _dev(cuda, Sv))
    for name in ("nobloom", "blocked_packed"):
        got = check(hw, cuda, Rk, Sk, Sv, _args(hw)[name], tag=("edge", nspec, side), cols=cols)
        s, m = got["sum"][hw.GROUP_MATCHED], got["minmax"][hw.GROUP_MATCHED]
        assert s.shape[0] == m.shape[0] == n_hit
        keys = Rk[s[:, 0]]  # (r_payload = R row)
        at = order[np.searchsorted(Sk[order], keys)]
        assert np.array_equal(Sk[at], keys)
        want = Sv[at].astype(np.int64)  # the one value at the key's position in S
        assert np.array_equal(s[:, 0], m[:, 0])
        assert (s[:, 1] == 1).all() and (m[:, 1] == 1).all()
        assert np.array_equal(s[:, 2], want) and np.array_equal(m[:, 2], want) and np.array_equal(m[:, 3], want)


# ------------------------------------------------------------------------------------ 3. skew
@pytest.mark.parametrize("name", ["blocked_packed", "basic_k1", "nobloom"])
def test_skewed_partitions(hw, cuda, name):
    """The hot-key columns of test_gpu_keys_pairs.test_pairs_skewed_partitions (key 77 in a third of
    R, key 88 in a tenth of S) with random values: the skew path's direct half stores and the
    pending words carry the value that belongs to their key."""
    rng = np.random.default_rng(9)
    Rk = np.concatenate([np.full(20000, 77), np.full(100, 88), rng.integers(-5000, 5000, size=40000),
                         [INT_MAX, -INT_MAX - 1]])
    Sk = np.concatenate([np.full(500, 77), np.full(100000, 88), rng.integers(-6000, 6000, size=900000),
                         [INT_MAX, -INT_MAX - 1, 77]])
    rng.shuffle(Rk)
    rng.shuffle(Sk)
    Sv = rng.integers(INT_MIN, INT_MAX, size=Sk.size, endpoint=True)
    got = check(hw, cuda, Rk, Sk, Sv, _args(hw)[name], tag="skew")
    rows = got["sum"][hw.GROUP_MATCHED]
    mine = rows[Rk[rows[:, 0]] == 88]
    assert mine.shape[0] == int((Rk == 88).sum()) >= 100 and (mine[:, 1] == int((Sk == 88).sum())).all()
    assert (mine[:, 2] == int(Sv[Sk == 88].astype(np.int64).sum())).all()


# ------------------------------------------------------ 4. hot S keys and 64-bit sums
@pytest.mark.parametrize("name", ["nobloom", "blocked_packed", "basic_k1"])
def test_hot_s_keys_and_64_bit_sums(hw, cuda, crc, name):
    """The S groups of test_gpu_group.test_hot_s_keys_and_64_bit_sums: three R keys with 200,000 S
    values of INT_MAX (the sum passes 2^32), 70,000 of INT_MIN and 100,001 alternating, beside
    filler; once with each of the three keys once in R (the bitmap path) and once twice (the hash
    table). The min/max form runs on the values of test_gpu_group_minmax's counterpart: each group's
    extremes occur once, at random positions, among values strictly between them."""
    rng = np.random.default_rng(66)
    args = _args(hw)[name]
    nR = 20000
    info = t.geometry(hw, cuda, args, name, nR)
    if info["sub_shift"] > 0:
        q0 = 9
        k3 = crc.key_of(shapes.job_codes(info, q0, 1, [5, 6, 7])).astype(np.int64)
        fill = crc.key_of(shapes.filler_codes(info, nR + 3000, {q0}, 1)).astype(np.int64)
    else:  # (basic filters: the partition is no code digit; three plain keys)
        k3 = np.array([-3, 123456, INT_MAX], dtype=np.int64)
        fill = 10**6 + rng.permutation(nR + 3000).astype(np.int64)
    sizes = (200000, 70000, 100001)
    alt = np.where(np.arange(100001) % 2 == 0, INT_MAX, INT_MIN)
    v_sum = [np.full(200000, INT_MAX), np.full(70000, INT_MIN), alt]
    want_sum = [200000 * INT_MAX, 70000 * INT_MIN, 50001 * INT_MAX + 50000 * INT_MIN]
    assert want_sum[0] > 2**32 and want_sum[1] < -2**32
    ends = ((INT_MIN, INT_MAX), (-1234567, 7654321), (-5000001, 5000002))
    v_mm = []
    for n, (lo, hi) in zip(sizes, ends):
        p = rng.integers(-10**6, 10**6, size=n, endpoint=True)
        a, b = rng.choice(n, 2, replace=False)
        p[a], p[b] = lo, hi
        v_mm.append(p)
    fill_s = fill[nR - 3000:]  # 3,000 of R's filler keys, 3,000 R lacks
    Sk = np.concatenate([np.repeat(k3, sizes), fill_s])
    fv = rng.integers(INT_MIN, INT_MAX, size=fill_s.size, endpoint=True)
    perm = rng.permutation(Sk.size)
    Sk = Sk[perm]
    Sv = {"sum": np.concatenate(v_sum + [fv])[perm], "minmax": np.concatenate(v_mm + [fv])[perm]}
    for copies in (1, 2):
        Rk = np.concatenate([np.repeat(k3, copies), fill[:nR - 3 * copies]])
        rng.shuffle(Rk)
        if info["sub_shift"] > 0:
            t.same_geometry(hw, cuda, _tuples(Rk, np.arange(Rk.size)), args, info)
        for form in ("sum", "minmax"):
            got = check(hw, cuda, Rk, Sk, Sv[form], args, forms=(form,))[form]
            for kind in (hw.GROUP_MATCHED, hw.GROUP_ALL):
                for i, k in enumerate(k3):
                    mine = got[kind][Rk[got[kind][:, 0]] == k]
                    assert mine.shape[0] == copies and (mine[:, 1] == sizes[i]).all()
                    if form == "sum":
                        assert (mine[:, 2] == want_sum[i]).all()
                    else:
                        assert (mine[:, 2:] == list(ends[i])).all()


# --------------------------------------------------------------- 5. duplicates on both sides
@pytest.mark.parametrize("name", ["blocked_packed", "basic_k1", "nobloom"])
def test_duplicates_on_both_sides(hw, cuda, crc, name):
    """The relations of test_gpu_group.test_duplicates_on_both_sides: 5,000 R keys three times each
    (INT_MAX, INT_MIN, 0, -1 and the key whose code is the kernels' empty-slot value among them), S
    key i (i mod 5) times and 7,000 keys R lacks. The three R rows of a key carry three different row
    indices and the same aggregates."""
    rng = np.random.default_rng(21)
    special = np.array([INT_MAX, INT_MIN, 0, -1, int(crc.key_of(0xFFFFFFFF))], dtype=np.int64)
    rest = np.setdiff1d(rng.choice(np.arange(-10**6, 10**6), 6000, replace=False), special)[:5000 - special.size]
    keys = np.concatenate([special, rest])
    assert np.unique(keys).size == 5000
    hits = np.concatenate([[0, 1, 2, 3, 4], np.arange(keys.size - 5) % 5])
    Rk = np.repeat(keys, 3)
    Sk = np.concatenate([np.repeat(keys, hits), rng.integers(2 * 10**6, 3 * 10**6, size=7000)])
    rng.shuffle(Rk)
    rng.shuffle(Sk)
    Sv = rng.integers(INT_MIN, INT_MAX, size=Sk.size, endpoint=True)
    got = check(hw, cuda, Rk, Sk, Sv, _args(hw)[name], tag="duplicates")
    for form in ("sum", "minmax"):
        rows = got[form][hw.GROUP_ALL]
        assert got[form][hw.GROUP_MATCHED].shape[0] == 3 * int((hits > 0).sum())
        for key, h in zip(keys[:50], hits[:50]):
            mine = rows[Rk[rows[:, 0]] == key]
            assert mine.shape[0] == 3 and np.unique(mine[:, 0]).size == 3 and (mine[:, 1] == h).all()
            assert (mine[:, 1:] == mine[0, 1:]).all()


# ------------------------------------------------------------------------------ 6. empty sides
@pytest.mark.parametrize("name", ["blocked_packed", "global_b4", "nobloom"])
def test_empty_sides(hw, cuda, name):
    """nR = 0; nS = 0 with an empty value column; and S rows none of which has a key of R, so that
    every job with R rows has no survivor that matches: |R| rows of count 0 under GROUP_ALL."""
    rng = np.random.default_rng(13)
    args = _args(hw)[name]
    some = rng.permutation(5000) + 1
    vals = rng.integers(INT_MIN, INT_MAX, size=5000, endpoint=True)
    empty = np.empty(0, dtype=np.int32)
    for Rk, Sk, Sv in ((empty, some, vals), (some, empty, empty), (some, some + 10000, vals)):
        got = check(hw, cuda, Rk, Sk, Sv, args)
        assert got["sum"][hw.GROUP_MATCHED].shape[0] == 0 and not got["sum"][hw.GROUP_ALL][:, 1:].any()
        assert got["minmax"][hw.GROUP_MATCHED].shape[0] == 0
        assert (got["minmax"][hw.GROUP_ALL][:, 1:] == mm.EMPTY).all()


# ---------------------------------------------------------------------- 7. capacity contract
@pytest.mark.parametrize("name", ["blocked_packed", "global_b4"])
def test_capacity_contract(hw, cuda, orc, name):
    """Capacities 0 (count only, d_out NULL), 1, n - 1 and n with a guard region behind d_out: 7 and
    the full count below n, nothing written past the capacity, every written row a row."""
    rng = np.random.default_rng(77)
    R = orc.relation(10000, 2, 10000, 10000, 1.0, 3)
    S = orc.relation(100000, 2, INT_MAX, 10000, 0.05, 4)
    Rk, Sk = _i32(R[:, 0]), _i32(S[:, 0])
    Sv = _i32(rng.integers(INT_MIN, INT_MAX, size=Sk.size, endpoint=True))
    args = _args(hw)[name]
    cols = (_dev(cuda, Rk), _dev(cuda, Sk), _dev(cuda, Sv))
    check(hw, cuda, Rk, Sk, Sv, args, cols=cols, capacity=10)  # (the wrapper runs again at the exact size)
    Rt, St = _tuples(Rk, np.arange(Rk.size)), _tuples(Sk, Sv)
    a = args._c()
    cR, cS, cV = cols
    GUARD = 0x5A5A5A5A
    for mod, entry in ((g, "hwbrj_join_keys_group_device"), (mm, "hwbrj_join_keys_group_minmax_device")):
        ref = mod._sorted(mod.reference(Rt, St))
        assert 1000 < int((ref[:, 1] > 0).sum()) < Rk.size - 1000

        def call(kind, buf, cap, n, pairs=None, st=None):
            return getattr(hw.lib(), entry)(cR.data_ptr(), cR.shape[0], cS.data_ptr(), cV.data_ptr(), cS.shape[0],
                                            ctypes.byref(a), kind, buf, cap, ctypes.byref(n), pairs, None, st, None)

        for kind, want in ((hw.GROUP_MATCHED, ref[ref[:, 1] > 0]), (hw.GROUP_ALL, ref)):
            nrows, total = want.shape[0], int(ref[:, 1].sum())
            rows = set(map(tuple, want.tolist()))
            n0 = ctypes.c_uint64()
            assert (call(kind, None, 0, n0), n0.value) == (7, nrows)  # count only
            for cap in (1, nrows - 1, nrows):
                buf = cuda.full((cap + 1024, 4), GUARD, dtype=cuda.int32, device="cuda:0")
                n, pairs, st = ctypes.c_uint64(), ctypes.c_uint64(), hw._Stats()
                rc = call(kind, buf.data_ptr(), cap, n, ctypes.byref(pairs), ctypes.byref(st))
                assert (rc, n.value, st.matches, pairs.value) == (7 if cap < nrows else 0, nrows, nrows, total)
                host = buf.cpu().numpy()
                assert (host[cap:] == GUARD).all()  # nothing past the capacity
                raw = host[:cap]
                if mod is g:  # {r_payload, count, sum as two words}
                    first = np.stack([raw[:, 0].astype(np.int64), raw[:, 1].view(np.uint32).astype(np.int64),
                                      np.ascontiguousarray(raw[:, 2:]).view(np.int64).ravel()], 1)
                else:
                    first = np.stack([raw[:, 0].astype(np.int64), raw[:, 1].view(np.uint32).astype(np.int64),
                                      raw[:, 2].astype(np.int64), raw[:, 3].astype(np.int64)], 1)
                assert np.unique(first[:, 0]).size == cap
                assert all(tuple(r) in rows for r in first.tolist())  # the first `capacity` rows are rows


# ---------------------------------------------------------------------------- 8. stream rule
def test_columns_cut_in_the_same_expression(hw, cuda, orc):
    """The three columns cut from 2M-row tensors with .contiguous() in the same expression as the
    call, stream=None: the wrappers wait for torch's current stream (the cutting kernels)."""
    R = orc.relation(200000, 2, 200000, 200000, 1.0, 5)
    S = orc.relation(2000000, 2, INT_MAX, 200000, 0.3, 6)
    S[:, 1] = _i32(np.random.default_rng(8).integers(INT_MIN, INT_MAX, size=S.shape[0], endpoint=True))
    R[:, 1] = np.arange(R.shape[0])
    dR, dS = t.to_dev(cuda, R), t.to_dev(cuda, S)
    args = _args(hw)["blocked_packed"]
    for mod, fn in ((g, hw.group_join_keys_device), (mm, hw.group_minmax_join_keys_device)):
        ref = mod._sorted(mod.reference(R, S))
        for kind in (hw.GROUP_MATCHED, hw.GROUP_ALL):
            _, rows, pairs, _ = fn(dR[:, 0].contiguous(), dS[:, 0].contiguous(), dS[:, 1].contiguous(), args, kind=kind)
            want = ref if kind == hw.GROUP_ALL else ref[ref[:, 1] > 0]
            assert pairs == int(ref[:, 1].sum())
            assert np.array_equal(mod._sorted(mod._host(rows)), want)


# ----------------------------------------------------------------------------- 9. neighbours
def test_neighbours_still_work(hw, cuda, orc):
    """tables_info answers 13 directly after a column group join (partitioned and side pass); the
    tuple group join, join_keys_pairs_device and join_device on the same data then still return
    their expected results, and a second column group join the first one's rows."""
    rng = np.random.default_rng(101)
    Rk = _i32(rng.choice(np.arange(1, 60000), 20000, replace=False))
    Sk = _i32(rng.integers(1, 90000, size=120000))
    Sv = _i32(rng.integers(INT_MIN, INT_MAX, size=Sk.size, endpoint=True))
    R, S = _tuples(Rk, np.arange(Rk.size)), _tuples(Sk, Sv)
    cols = (_dev(cuda, Rk), _dev(cuda, Sk), _dev(cuda, Sv))
    dR, dS = t.to_dev(cuda, R), t.to_dev(cuda, S)
    args = _args(hw)["blocked_packed"]
    for a in (args, _args(hw)["global_b4"]):
        for fn in (hw.group_join_keys_device, hw.group_minmax_join_keys_device):
            fn(*cols, a, kind=hw.GROUP_ALL)
            with pytest.raises(hw.TablesError) as ei:
                hw.tables_info()
            assert ei.value.code == 13
        first = check(hw, cuda, Rk, Sk, Sv, a, cols=cols)
        again = check(hw, cuda, Rk, Sk, Sv, a, cols=cols)
        for form in first:
            for kind in first[form]:
                assert np.array_equal(first[form][kind], again[form][kind])
    hw.group_join_keys_device(*cols, args)
    g.check(hw, cuda, R, S, args)  # (the tuple group join against its host reference)
    hw.group_join_keys_device(*cols, args)
    Ri, Si = kp._rel(Rk), kp._rel(Sk)
    kp.check_pairs(hw, kp.Ref(orc, Ri, Si), cols[0], cols[1], args, kp._counts(orc, Ri, Si, args))
    hw.group_minmax_join_keys_device(*cols, args)
    assert hw.join_device(dR, dS, args).matches == orc.join_pairs(R, S).shape[0]


# ------------------------------------------------------------------------ Python refusals
def test_python_refusals_on_the_device(hw, cuda):
    c = _dev(cuda, np.arange(1000))
    T = cuda.zeros((1000, 2), dtype=cuda.int32, device="cuda:0")
    bad = {"(N, 2) tensor": T, "int64 column": c.to(cuda.int64), "CPU tensor": c.cpu(), "strided view": T[:, 0],
           "misaligned slice": c[1:]}
    for fn in (hw.group_join_keys_device, hw.group_minmax_join_keys_device):
        for what, x in bad.items():
            for cols in ((x, c, c), (c, x, c), (c, c, x)):
                with pytest.raises(ValueError):
                    fn(*cols)
        with pytest.raises(ValueError):
            fn(c, c, c[:996])  # (aligned, but not Sk's length)
