"""The existence joins (hwbrj_join_semi_device: k_join_semi, k_semi_emit, the global-mode side pass).

The reference of every check is plain numpy on the host inputs: mask = isin(S.key, R.key), SEMI =
S[mask], ANTI = S[~mask], compared as exact multisets of {key, payload} rows (lexsort over both
columns). Every case runs both kinds and also checks n_semi + n_anti = |S| and that `filtered` is
the counting join's. Crafted shapes take their sizes from the kernel constants (hwbrj_tables_info
after a materializing join of the same |R| and filter: the existence join runs on its geometry)."""
import ctypes

import numpy as np
import pytest

import shapes

pytestmark = pytest.mark.gpu
INT_MAX, INT_MIN = 2**31 - 1, -2**31


def to_dev(cuda, a):
    return cuda.from_numpy(np.ascontiguousarray(a, dtype=np.int32).reshape(-1, 2)).to("cuda:0")


def _args(hw):
    """The modes of tests/test_gpu_materialize.py::_args, and a filter with F = 256 partitions whose
    job keys (18 bits) take k_join_semi's hash set although the partition is a code digit."""
    return {
        "blocked_packed": hw.BloomFilterArgs(hw.BLOCKED, 1 << 24, 1, 1024),
        "blocked_code": hw.BloomFilterArgs(hw.BLOCKED, 1 << 24, 1, 2048),
        "blocked_k3": hw.BloomFilterArgs(hw.BLOCKED, 1 << 24, 3, 512),
        "sectorized_k2": hw.BloomFilterArgs(hw.SECTORIZED, 1 << 24, 2, 1024),
        "basic_k1": hw.BloomFilterArgs(hw.BASIC, 1 << 24, 1),
        "basic_k3": hw.BloomFilterArgs(hw.BASIC, 1 << 22, 3),
        "two_segments": hw.BloomFilterArgs(hw.BLOCKED, 1 << 31, 1, 1024),
        "global_b4": hw.BloomFilterArgs(hw.BLOCKED, 1 << 20, 1, 4),
        "nobloom": None,
        "blocked_f256": hw.BloomFilterArgs(hw.BLOCKED, 1 << 18, 1, 1024),
    }


@pytest.fixture(scope="module")
def crc(orc):
    return shapes.Crc(orc.crc)


def _sorted(rows):
    rows = np.asarray(rows).reshape(-1, 2)
    return rows[np.lexsort((rows[:, 1], rows[:, 0]))]


def _rel(keys, rng):
    keys = np.asarray(keys).astype(np.int64)
    return np.stack([keys, rng.integers(-2**31, 2**31, size=keys.size)], 1).astype(np.int32).reshape(-1, 2)


def check(hw, cuda, R, S, args, **kw):
    """Both kinds against numpy; returns {anti: rows} (host)."""
    dR, dS = to_dev(cuda, R), to_dev(cuda, S)
    mask = np.isin(S[:, 0], R[:, 0])
    filtered = hw.join_device(dR, dS, args).filtered
    got = {}
    for anti in (False, True):
        st, rows, _ = hw.semi_join_device(dR, dS, args, anti=anti, **kw)
        want = S[~mask] if anti else S[mask]
        rows = rows.cpu().numpy()
        print(f"{'anti' if anti else 'semi'}: {rows.shape[0]} rows (numpy {want.shape[0]}), filtered "
              f"{st.filtered} (counting join {filtered})")
        assert st.matches == rows.shape[0] == want.shape[0]
        assert np.array_equal(_sorted(rows), _sorted(want))
        assert st.filtered == filtered
        got[anti] = rows
    assert got[False].shape[0] + got[True].shape[0] == S.shape[0]
    return got


_GEOM = {}


def geometry(hw, cuda, args, name, nR):
    """tables_info of a materializing join of |R| = nR under args (throw-away keys)."""
    if (name, nR) not in _GEOM:
        R = np.stack([np.arange(nR, dtype=np.int32), np.zeros(nR, dtype=np.int32)], 1)
        hw.join_materialize_device(to_dev(cuda, R), to_dev(cuda, R[:8]), args, capacity=64)
        _GEOM[(name, nR)] = hw.tables_info()
    return dict(_GEOM[(name, nR)])


def same_geometry(hw, cuda, R, args, info):
    """A materializing join of this R and args reports the geometry the keys were crafted for."""
    hw.join_materialize_device(to_dev(cuda, R), to_dev(cuda, R[:8]), args, capacity=64)
    now = hw.tables_info()
    keys = ("mode", "format", "F", "NSUB", "sub_shift", "hash_shift", "nseg", "bitmap", "G", "CH", "BSW", "slot")
    assert {k: now[k] for k in keys} == {k: info[k] for k in keys}


# ------------------------------------------------------------------------------ 1: every mode
@pytest.mark.parametrize("name", ["blocked_packed", "blocked_code", "blocked_k3", "sectorized_k2",
                                  "basic_k1", "basic_k3", "two_segments", "global_b4", "nobloom"])
def test_every_mode(hw, cuda, orc, name):
    """|R| = 40,000 distinct keys, |S| = 300,000 at selectivity 0.2, random payloads, 1,000 S rows
    twice."""
    rng = np.random.default_rng(5)
    R = orc.relation(40000, 2, 40000, 40000, 1.0, 1)
    S = orc.relation(299000, 2, INT_MAX, 40000, 0.2, 2)
    R[:, 1] = rng.integers(-2**31, 2**31, size=R.shape[0])
    S[:, 1] = rng.integers(-2**31, 2**31, size=S.shape[0])
    S = np.concatenate([S, S[rng.choice(S.shape[0], 1000, replace=False)]])
    assert np.unique(R[:, 0]).size == 40000 and S.shape[0] == 300000
    check(hw, cuda, R, S, _args(hw)[name])


# ------------------------------------------------------------------------ 2: duplicate R keys
@pytest.mark.parametrize("name", ["blocked_packed", "basic_k1", "nobloom"])
def test_duplicate_r_keys(hw, cuda, crc, name):
    """5,000 R keys three times each, with INT_MAX, INT_MIN, 0, -1 and the key whose code is the
    kernels' empty-slot value; S hits key i (i mod 5) times: SEMI lists each S row once."""
    rng = np.random.default_rng(21)
    special = np.array([INT_MAX, INT_MIN, 0, -1, int(crc.key_of(0xFFFFFFFF))], dtype=np.int64)
    rest = np.setdiff1d(rng.choice(np.arange(-10**6, 10**6), 6000, replace=False), special)[:5000 - special.size]
    keys = np.concatenate([special, rest])
    assert np.unique(keys).size == 5000
    # (the special keys are hit 0..4 times: the empty-slot code's key four times)
    hits = np.concatenate([[0, 1, 2, 3, 4], np.arange(keys.size - 5) % 5])
    Rk = np.repeat(keys, 3)
    Sk = np.concatenate([np.repeat(keys, hits), rng.integers(2 * 10**6, 3 * 10**6, size=7000)])
    rng.shuffle(Rk)
    rng.shuffle(Sk)
    R, S = _rel(Rk, rng), _rel(Sk, rng)
    got = check(hw, cuda, R, S, _args(hw)[name])
    assert got[False].shape[0] == int(hits.sum())  # (not three times as many)


# -------------------------------------------------------------- 3: a hot R key across pieces
@pytest.mark.parametrize("name", ["nobloom", "blocked_packed"])
def test_hot_r_key_across_pieces(hw, cuda, crc, name):
    """One job holds an R key 2 kMatPiece + 5 times and three other keys, more than kMatRCap tuples:
    its survivors (40 of the hot key, 10 of each other, 50 of keys R lacks) are each listed once."""
    rng = np.random.default_rng(33)
    args = _args(hw)[name]
    nR = 20000
    info = geometry(hw, cuda, args, name, nR)
    q0, sub0 = 17, 1
    hot = 2 * info["m_piece"] + 5
    rv = np.concatenate([np.full(hot, 7), [11, 12, 13]])
    assert rv.size >= info["m_rcap"] + 1
    nf = nR - rv.size
    fill = shapes.filler_codes(info, nf + 3000, {q0}, 1)  # distinct: R takes the first nf
    Rc = np.concatenate([shapes.job_codes(info, q0, sub0, rv), fill[:nf]])
    sv = np.concatenate([np.full(40, 7), np.repeat([11, 12, 13], 10), 1000 + np.arange(50)])
    Sc = np.concatenate([shapes.job_codes(info, q0, sub0, sv), fill[nf - 3000:]])  # 3,000 of R's, 3,000 not
    rng.shuffle(Rc)
    rng.shuffle(Sc)
    R, S = _rel(crc.key_of(Rc), rng), _rel(crc.key_of(Sc), rng)
    same_geometry(hw, cuda, R, args, info)
    got = check(hw, cuda, R, S, args)
    jobk = crc.key_of(shapes.job_codes(info, q0, sub0, np.arange(2000)))
    assert np.isin(got[False][:, 0], jobk).sum() == 70 and np.isin(got[True][:, 0], jobk).sum() == 50


# ----------------------------------------------------------------- 4: partitions with no R
def test_partition_without_r(hw, cuda, crc):
    """No R tuple in partition q0, 100 S rows there: ANTI holds them, SEMI none of them."""
    rng = np.random.default_rng(44)
    nR, q0 = 20000, 300
    info = geometry(hw, cuda, None, "nobloom", nR)
    Rc = shapes.filler_codes(info, nR, {q0}, 1)
    inq = np.uint64(q0) | ((np.arange(100, dtype=np.uint64) * np.uint64(977)) << np.uint64(info["F"].bit_length() - 1))
    Sc = np.concatenate([inq.astype(np.uint32), Rc[:3000], shapes.filler_codes(info, 3000, {q0}, 999)])
    rng.shuffle(Sc)
    R, S = _rel(crc.key_of(Rc), rng), _rel(crc.key_of(Sc), rng)
    same_geometry(hw, cuda, R, None, info)
    got = check(hw, cuda, R, S, None)
    q_keys = crc.key_of(inq.astype(np.uint32))
    assert np.isin(got[True][:, 0], q_keys).sum() == 100 and not np.isin(got[False][:, 0], q_keys).any()


# ------------------------------------------------------------- 5: more than kMatDesc descriptors
@pytest.mark.parametrize("name", ["nobloom", "blocked_f256"])
def test_more_descriptors_than_a_batch(hw, cuda, crc, name):
    """A partition of kMatDesc * BSW * 32 + 1 R tuples: more than kMatDesc * BSW chunks (a chunk holds
    at most 32), so more than kMatDesc build sweeps, the R run descriptors of each of its jobs.
    60,000 distinct keys, repeated all over it. nobloom: the bitmap path; blocked_f256: the hash set
    in several pieces per descriptor batch."""
    rng = np.random.default_rng(55)
    args = _args(hw)[name]
    q0, fill = 5, 20000
    probe = geometry(hw, cuda, args, name, 8)
    n_q = probe["m_desc"] * probe["BSW"] * 32 + 1
    nR = n_q + fill
    info = geometry(hw, cuda, args, name, nR)
    assert (info["m_desc"], info["BSW"]) == (probe["m_desc"], probe["BSW"])
    assert info["bitmap"] == (1 if name == "nobloom" else 0)
    lf = info["F"].bit_length() - 1
    hi = rng.choice(1 << min(32 - lf, 24), 66000, replace=False).astype(np.uint64)
    qcodes = (np.uint64(q0) | (hi << np.uint64(lf))).astype(np.uint32)
    member, absent = qcodes[:60000], qcodes[60000:]
    Rc = np.concatenate([member[rng.integers(0, member.size, size=n_q)], shapes.filler_codes(info, fill, {q0}, 1)])
    Sc = np.concatenate([member[rng.integers(0, member.size, size=3000)], absent[rng.integers(0, absent.size, size=3000)],
                         Rc[n_q:n_q + 3000], shapes.filler_codes(info, 3000, {q0}, 777)])
    rng.shuffle(Rc)
    rng.shuffle(Sc)
    R, S = _rel(crc.key_of(Rc), rng), _rel(crc.key_of(Sc), rng)
    check(hw, cuda, R, S, args)


# ----------------------------------------------------------------------------- 6: edge sizes
@pytest.mark.parametrize("name", ["blocked_packed", "nobloom"])
def test_edge_sizes(hw, cuda, name):
    rng = np.random.default_rng(13)
    for nR, nS in [(0, 1000), (1000, 0), (1, 1), (7, 33), (4097, 4099)]:
        R = _rel(rng.permutation(nR) + 1, rng)
        S = _rel(rng.integers(0, 2 * max(nR, 1) + 2, size=nS), rng)
        got = check(hw, cuda, R, S, _args(hw)[name])
        if nR == 0:
            assert got[False].shape[0] == 0 and got[True].shape[0] == nS


# ---------------------------------------------------------------------- 7: capacity contract
def test_capacity_contract(hw, cuda, orc):
    rng = np.random.default_rng(77)
    R = orc.relation(10000, 2, 10000, 10000, 1.0, 3)
    S = orc.relation(100000, 2, INT_MAX, 10000, 0.5, 4)
    S[:, 1] = rng.integers(-2**31, 2**31, size=S.shape[0])
    args = _args(hw)["blocked_packed"]
    check(hw, cuda, R, S, args, capacity=10)  # (the wrapper runs again at the exact size)
    dR, dS = to_dev(cuda, R), to_dev(cuda, S)
    a = args._c()
    mask = np.isin(S[:, 0], R[:, 0])
    for kind, want in ((hw.JOIN_SEMI, S[mask]), (hw.JOIN_ANTI, S[~mask])):
        cap, guard = 1000, 4096
        buf = cuda.full((cap + guard, 2), 0x5A5A5A5A, dtype=cuda.int32, device="cuda:0")
        n, st = ctypes.c_uint64(), hw._Stats()
        rc = hw.lib().hwbrj_join_semi_device(dR.data_ptr(), dR.shape[0], dS.data_ptr(), dS.shape[0], ctypes.byref(a),
                                             kind, buf.data_ptr(), cap, ctypes.byref(n), None, ctypes.byref(st), None)
        assert (rc, n.value, st.matches) == (7, want.shape[0], want.shape[0])
        host = buf.cpu().numpy()
        assert (host[cap:] == 0x5A5A5A5A).all()  # nothing past capacity
        rows = set(map(tuple, want.tolist()))
        assert all(tuple(r) in rows for r in host[:cap].tolist())  # the first `capacity` rows are rows
        n0 = ctypes.c_uint64()
        rc = hw.lib().hwbrj_join_semi_device(dR.data_ptr(), dR.shape[0], dS.data_ptr(), dS.shape[0], ctypes.byref(a),
                                             kind, None, 0, ctypes.byref(n0), None, None, None)
        assert (rc, n0.value) == (7, want.shape[0])  # count only


# ------------------------------------------------------------------------------ 8: skewed S
@pytest.mark.parametrize("name", ["blocked_packed", "basic_k1", "nobloom"])
def test_skewed_partitions(hw, cuda, name):
    """The hot-key relations of test_pairs_skewed_partitions (key 88 in a tenth of S, key 77 in a
    third of R): the scatter's skew path together with the emission."""
    rng = np.random.default_rng(9)
    Rk = np.concatenate([np.full(20000, 77), np.full(100, 88), rng.integers(-5000, 5000, size=40000),
                         [INT_MAX, -INT_MAX - 1]])
    Sk = np.concatenate([np.full(500, 77), np.full(100000, 88), rng.integers(-6000, 6000, size=900000),
                         [INT_MAX, -INT_MAX - 1, 77]])
    rng.shuffle(Rk)
    rng.shuffle(Sk)
    R = np.stack([Rk, rng.integers(-2**31, 2**31, size=Rk.size)], 1).astype(np.int32)
    S = np.stack([Sk, rng.integers(-2**31, 2**31, size=Sk.size)], 1).astype(np.int32)
    check(hw, cuda, R, S, _args(hw)[name])
