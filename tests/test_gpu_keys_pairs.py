"""The row-index joins on key columns (hw.join_keys_pairs_device, hw.semi_join_keys_device,
hw.outer_join_keys_device) against the oracle and numpy.

Every test builds (N, 2) relations with payload = arange(N), as a caller without these entries
would have had to, and joins their key columns. Pairs come from orc.join_pairs on the tuples,
existence rows from np.isin, `filtered` and the match count from orc.bpro: nothing is compared with
the code under test alone. The tuple joins run beside the key-column ones only where the point is
that both layouts leave the same tables."""
import ctypes

import numpy as np
import pytest

import test_gpu_shapes as gs
from test_gpu_materialize import _args

pytestmark = pytest.mark.gpu

INT_MIN, INT_MAX = -2**31, 2**31 - 1
MODES = ["blocked_packed", "blocked_code", "blocked_k3", "sectorized_k2", "basic_k1", "basic_k3", "two_segments",
         "global_b4", "nobloom"]


def _rel(keys):
    """(N, 2) int32 {key, row index}."""
    keys = np.asarray(keys).astype(np.int64).astype(np.int32)
    return np.stack([keys, np.arange(keys.size, dtype=np.int32)], 1).reshape(-1, 2)


def _col(cuda, T):
    """The key column of T in a device allocation of exactly its size."""
    c = cuda.empty(T.shape[0], dtype=cuda.int32, device="cuda:0")
    c.copy_(cuda.from_numpy(np.ascontiguousarray(T[:, 0])))
    cuda.cuda.synchronize()
    return c


def _u64(rows):
    """Sorted rows, each as one 64-bit word (an exact multiset comparison)."""
    rows = np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1, 2))
    return np.sort(rows.view(np.uint64).ravel())


class Ref:
    """What the joins of R and S (payload = row index) must return, from the oracle and numpy."""

    def __init__(self, orc, R, S):
        self.R, self.S = R, S
        both = R.shape[0] and S.shape[0]
        self.pairs = orc.join_pairs(R, S).reshape(-1, 2) if both else np.empty((0, 2), dtype=np.int32)
        self.mask = np.isin(S[:, 0], R[:, 0])      # S rows with a partner
        self.r_hit = np.isin(R[:, 0], S[:, 0])     # R rows with a partner
        self.upairs = _u64(self.pairs)

    def outer_parts(self):
        s_only = np.nonzero(~self.mask)[0]
        r_only = np.nonzero(~self.r_hit)[0]
        s_rows = np.stack([np.full(s_only.size, -1), s_only], 1).astype(np.int32).reshape(-1, 2)
        r_rows = np.stack([r_only, np.full(r_only.size, -1)], 1).astype(np.int32).reshape(-1, 2)
        return s_rows, r_rows


def _counts(orc, R, S, args):
    """(filtered, matches) of the counting join, from the oracle."""
    if args is None:
        res, filt, _ = orc.bpro(R, S, 8, 0, 0, 0, 0, use_bloom=False)
    else:
        res, filt, _ = orc.bpro(R, S, 8, args.variant, args.m, args.k, args.B)
    return filt, res


def check_pairs(hw, ref, cR, cS, args, counts=None, **kw):
    st, pairs, _ = hw.join_keys_pairs_device(cR, cS, args, **kw)
    p = pairs.cpu().numpy()
    print(f"pairs: {p.shape[0]} rows (oracle {ref.pairs.shape[0]}), filtered {st.filtered} (oracle {counts})")
    assert st.matches == p.shape[0] == ref.pairs.shape[0]
    assert np.array_equal(ref.R[p[:, 0], 0], ref.S[p[:, 1], 0])  # every pair joins equal keys
    assert np.array_equal(_u64(p), ref.upairs)
    if counts is not None:
        assert (st.filtered, st.matches) == counts
    return st


def check_semi(hw, ref, cR, cS, args, counts=None, kinds=(False, True), **kw):
    for anti in kinds:
        st, rows, _ = hw.semi_join_keys_device(cR, cS, args, anti=anti, **kw)
        r = rows.cpu().numpy()
        want = np.nonzero(~ref.mask if anti else ref.mask)[0]
        print(f"anti={anti}: {r.shape[0]} rows (numpy {want.size}), filtered {st.filtered} (oracle {counts})")
        assert st.matches == r.shape[0] == want.size
        assert np.array_equal(ref.S[r[:, 1], 0], r[:, 0])  # each row names the position of its key
        assert np.array_equal(np.sort(r[:, 1]), want)
        if counts is not None:
            assert st.filtered == counts[0]


def check_outer(hw, ref, cR, cS, args, counts=None, kinds=None, **kw):
    s_rows, r_rows = ref.outer_parts()
    for kind in kinds if kinds is not None else (hw.OUTER_S, hw.OUTER_R, hw.OUTER_FULL):
        parts = [ref.pairs] + ([s_rows] if kind != hw.OUTER_R else []) + ([r_rows] if kind != hw.OUTER_S else [])
        want_cls = (ref.pairs.shape[0], s_rows.shape[0] if kind != hw.OUTER_R else 0,
                    r_rows.shape[0] if kind != hw.OUTER_S else 0)
        st, rows, cls, _ = hw.outer_join_keys_device(cR, cS, args, kind=kind, **kw)
        r = rows.cpu().numpy()
        print(f"kind {kind}: {r.shape[0]} rows, classes {cls} (numpy {want_cls}), filtered {st.filtered} "
              f"(oracle {counts})")
        assert cls == want_cls
        assert st.matches == r.shape[0] == sum(cls)
        assert np.array_equal(_u64(r), _u64(np.concatenate(parts)))  # (-1 on the missing side)
        if counts is not None:
            assert st.filtered == counts[0] and cls[0] == counts[1]


# ------------------------------------------------------------------------------ 1. every mode
_MODE = {}


def _mode_case(orc, cuda):
    """The relations of test_gpu_materialize.test_pairs_every_mode with payload = row index; at
    G = 256 every scatter workgroup of S gets one full round and a partial one."""
    if not _MODE:
        R = orc.relation(400000, 2, 400000, 400000, 1.0, 1)
        S = orc.relation(3000000, 2, INT_MAX, 400000, 0.2, 2)
        assert np.array_equal(R[:, 1], np.arange(R.shape[0])) and np.array_equal(S[:, 1], np.arange(S.shape[0]))
        _MODE.update(ref=Ref(orc, R, S), cR=_col(cuda, R), cS=_col(cuda, S))
    return _MODE["ref"], _MODE["cR"], _MODE["cS"]


@pytest.mark.parametrize("name", MODES)
def test_pairs_every_mode(hw, cuda, orc, name):
    ref, cR, cS = _mode_case(orc, cuda)
    args = _args(hw)[name]
    check_pairs(hw, ref, cR, cS, args, _counts(orc, ref.R, ref.S, args))


@pytest.mark.parametrize("name", MODES)
def test_semi_and_anti_every_mode(hw, cuda, orc, name):
    ref, cR, cS = _mode_case(orc, cuda)
    args = _args(hw)[name]
    check_semi(hw, ref, cR, cS, args, _counts(orc, ref.R, ref.S, args))


@pytest.mark.parametrize("name", MODES)
def test_outer_every_mode(hw, cuda, orc, name):
    ref, cR, cS = _mode_case(orc, cuda)
    args = _args(hw)[name]
    check_outer(hw, ref, cR, cS, args, _counts(orc, ref.R, ref.S, args))


# ------------------------------------------------------------- 2. row index at every range edge
EDGE_N = ["1", "2", "3", "4", "5", "4G-1", "4G", "4G+1", "G*round-1", "G*round", "G*round+1", "2*G*round+5"]
A, C = 0x9E3779B1, 0x7F4A7C15  # i -> i * A + C mod 2^32: distinct keys


def _edge_n(hw, cuda, nspec):
    info = gs.geometry(hw, cuda, None, 8, mat=True)
    G, rnd = info["G"], info["sc_round"]
    assert rnd == 1024 * 8  # the payload scatter's round
    return {"4G-1": 4 * G - 1, "4G": 4 * G, "4G+1": 4 * G + 1, "G*round-1": G * rnd - 1, "G*round": G * rnd,
            "G*round+1": G * rnd + 1, "2*G*round+5": 2 * G * rnd + 5}.get(nspec) or int(nspec)


@pytest.mark.parametrize("side", ["R", "S"])
@pytest.mark.parametrize("nspec", EDGE_N)
def test_row_index_at_every_range_edge(hw, cuda, orc, nspec, side):
    """A column of exactly n distinct keys (torch.empty(n), no padding) that ends in INT32_MIN,
    INT32_MAX, 0 and -1; the other side holds every 97th key and 500 absent ones. Every row must name
    the position of its key: what goes wrong if the workgroup's first row, the round base or the
    four-keys-per-load index shape is off by one. PRO and a blocked filter with packed words."""
    n = _edge_n(hw, cuda, nspec)
    k = ((np.arange(n + 500, dtype=np.uint64) * A + C) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    big = k[:n].copy()
    special = np.array([INT_MIN, INT_MAX, 0, -1], dtype=np.int32)
    big[-min(n, 4):] = np.roll(special, n)[-min(n, 4):]
    other = np.concatenate([big[::97], k[n:]])
    np.random.default_rng(n).shuffle(other)
    R, S = (_rel(big), _rel(other)) if side == "R" else (_rel(other), _rel(big))
    ref = Ref(orc, R, S)
    assert ref.pairs.shape[0] >= (n + 96) // 97
    cR, cS = _col(cuda, R), _col(cuda, S)
    for name in ("nobloom", "blocked_packed"):
        args = _args(hw)[name]
        check_pairs(hw, ref, cR, cS, args)
        check_semi(hw, ref, cR, cS, args)
        check_outer(hw, ref, cR, cS, args, kinds=(hw.OUTER_FULL,))


# ------------------------------------------------------------------------------------ 3. skew
@pytest.mark.parametrize("name", ["blocked_packed", "basic_k1", "nobloom"])
def test_pairs_skewed_partitions(hw, cuda, orc, name):
    """The hot-key relations of test_gpu_materialize.test_pairs_skewed_partitions (key 77 in a third
    of R, key 88 in a tenth of S): the direct halves and the pending words carry the right rows."""
    rng = np.random.default_rng(9)
    Rk = np.concatenate([np.full(20000, 77), np.full(100, 88), rng.integers(-5000, 5000, size=40000),
                         [INT_MAX, -INT_MAX - 1]])
    Sk = np.concatenate([np.full(500, 77), np.full(100000, 88), rng.integers(-6000, 6000, size=900000),
                         [INT_MAX, -INT_MAX - 1, 77]])
    rng.shuffle(Rk)
    rng.shuffle(Sk)
    R, S = _rel(Rk), _rel(Sk)
    ref = Ref(orc, R, S)
    cR, cS = _col(cuda, R), _col(cuda, S)
    args = _args(hw)[name]
    check_pairs(hw, ref, cR, cS, args, _counts(orc, R, S, args))
    check_semi(hw, ref, cR, cS, args)
    check_outer(hw, ref, cR, cS, args, kinds=(hw.OUTER_FULL,))


# ------------------------------------------------------------- 4. same tables as the tuples
@pytest.mark.parametrize("cfg", [None, gs.BLK512])
def test_same_tables_as_the_tuple_join(hw, cuda, orc, cfg):
    """join_materialize_device on the tuples and join_keys_pairs_device on their columns leave the
    same geometry words and the same element starts on both sides (PRO, and F = 512)."""
    R = orc.relation(100003, 2, 100003, 100003, 1.0, 3)
    S = orc.relation(400009, 2, INT_MAX, 100003, 0.5, 4)
    ref = Ref(orc, R, S)
    dR, dS = gs.to_dev(cuda, R), gs.to_dev(cuda, S)
    st_t, pairs_t, _ = hw.join_materialize_device(dR, dS, gs.mk(hw, cfg))
    info_t = hw.tables_info()
    T_t = (hw.tables_read(hw.TAB_R_ELEM_START), hw.tables_read(hw.TAB_S_ELEM_START))
    assert np.array_equal(_u64(pairs_t.cpu().numpy()), ref.upairs)
    check_pairs(hw, ref, _col(cuda, R), _col(cuda, S), gs.mk(hw, cfg), gs.ref_counts(orc, hw, R, S, cfg))
    info_k = hw.tables_info()
    assert info_k["mat"] == info_t["mat"] == 1
    assert {k: info_k[k] for k in gs.GEOM} == {k: info_t[k] for k in gs.GEOM}
    assert np.array_equal(hw.tables_read(hw.TAB_R_ELEM_START), T_t[0])
    assert np.array_equal(hw.tables_read(hw.TAB_S_ELEM_START), T_t[1])


# ------------------------------------------------------------------------------- 5. capacity
def test_capacity_contract(hw, cuda, orc):
    """capacity=1000 on 500,000 pairs: the wrapper runs again at size; the C entry returns 7 with
    the full count; the count-only form of the semi and outer entries gives the full count."""
    R = orc.relation(100000, 2, 100000, 100000, 1.0, 3)
    S = orc.relation(1000000, 2, INT_MAX, 100000, 0.5, 4)
    ref = Ref(orc, R, S)
    assert ref.pairs.shape[0] == 500000
    cR, cS = _col(cuda, R), _col(cuda, S)
    args = _args(hw)["blocked_packed"]
    check_pairs(hw, ref, cR, cS, args, capacity=1000)
    check_semi(hw, ref, cR, cS, args, capacity=1000)
    check_outer(hw, ref, cR, cS, args, kinds=(hw.OUTER_FULL,), capacity=1000)

    L, a = hw.lib(), args._c()
    out = cuda.full((1001, 2), 0x5A5A5A5A, dtype=cuda.int32, device="cuda:0")
    n = ctypes.c_uint64()
    ptrs = (cR.data_ptr(), cR.shape[0], cS.data_ptr(), cS.shape[0], ctypes.byref(a))
    rc = L.hwbrj_join_keys_pairs_device(*ptrs, out.data_ptr(), 1000, ctypes.byref(n), None, None, None)
    assert (rc, n.value) == (7, 500000)
    got = out.cpu().numpy()
    assert np.all(got[1000] == 0x5A5A5A5A)  # nothing beyond the capacity
    assert np.all(np.isin(_u64(got[:1000]), ref.upairs))
    rc = L.hwbrj_join_keys_pairs_device(*ptrs, None, 0, ctypes.byref(n), None, None, None)
    assert (rc, n.value) == (7, 500000)
    for kind, want in ((hw.JOIN_SEMI, int(ref.mask.sum())), (hw.JOIN_ANTI, int((~ref.mask).sum()))):
        rc = L.hwbrj_join_keys_semi_device(*ptrs, kind, None, 0, ctypes.byref(n), None, None, None)
        assert (rc, n.value) == (7 if want else 0, want)
    s_rows, r_rows = ref.outer_parts()
    for kind, want in ((hw.OUTER_S, 500000 + s_rows.shape[0]), (hw.OUTER_R, 500000 + r_rows.shape[0]),
                       (hw.OUTER_FULL, 500000 + s_rows.shape[0] + r_rows.shape[0])):
        cls = (ctypes.c_uint64 * 3)()
        rc = L.hwbrj_join_keys_outer_device(*ptrs, kind, None, 0, ctypes.byref(n), cls, None, None, None)
        assert (rc, n.value) == (7, want)
        assert sum(cls) == want and cls[0] == 500000


# ---------------------------------------------------------------------------- 6. stream rule
def test_columns_cut_in_the_same_expression(hw, cuda, orc):
    """A 2M-key column cut with T[:, 0].contiguous() and joined in the same expression, stream=None:
    the wrappers wait for torch's current stream (the cutting kernel) before the library's own."""
    R = orc.relation(200000, 2, 200000, 200000, 1.0, 5)
    S = orc.relation(2000000, 2, INT_MAX, 200000, 0.3, 6)
    ref = Ref(orc, R, S)
    dR, dS = gs.to_dev(cuda, R), gs.to_dev(cuda, S)
    args = _args(hw)["blocked_packed"]
    counts = _counts(orc, R, S, args)
    st, pairs, _ = hw.join_keys_pairs_device(dR[:, 0].contiguous(), dS[:, 0].contiguous(), args)
    assert (st.filtered, st.matches) == counts
    assert np.array_equal(_u64(pairs.cpu().numpy()), ref.upairs)
    st, rows, _ = hw.semi_join_keys_device(dR[:, 0].contiguous(), dS[:, 0].contiguous(), args)
    assert (st.filtered, st.matches) == (counts[0], int(ref.mask.sum()))
    assert np.array_equal(np.sort(rows.cpu().numpy()[:, 1]), np.nonzero(ref.mask)[0])
    st, rows, cls, _ = hw.outer_join_keys_device(dR[:, 0].contiguous(), dS[:, 0].contiguous(), args, kind=hw.OUTER_S)
    assert (st.filtered, cls) == (counts[0], (counts[1], int((~ref.mask).sum()), 0))


# ------------------------------------------------------------------------ 7. Python refusals
def test_python_refusals_on_the_device(hw, cuda, orc):
    R = orc.relation(1000, 2, 1000, 1000, 1.0, 7)
    dR = gs.to_dev(cuda, R)
    c = _col(cuda, R)
    bad = {"(N, 2) tensor": dR, "int64 column": c.to(cuda.int64), "CPU tensor": c.cpu(), "strided view": dR[:, 0],
           "misaligned slice": c[1:]}
    for what, t in bad.items():
        for fn in (hw.join_keys_pairs_device, hw.semi_join_keys_device, hw.outer_join_keys_device):
            with pytest.raises(ValueError):
                fn(t, c)
            with pytest.raises(ValueError):
                fn(c, t)
    check_pairs(hw, Ref(orc, R, R), c, c, None)
