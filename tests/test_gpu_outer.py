"""The outer joins (hwbrj_join_outer_device: k_join_outer, k_outer_emit, the global-mode side pass).

The reference of every check is computed on the host from the inputs: the inner pairs are
orc.join_pairs(R, S), the S-only rows S[~isin(S.key, R.key)] as {null, S.payload}, the R-only rows
R[~isin(R.key, S.key)] as {R.payload, null}; the rows of a kind are compared with the concatenation
as exact sorted multisets (a row is compared as one 64-bit word). Every case runs the three kinds and
also checks the class counts, `filtered` and the inner count against the counting join, and that
OUTER_FULL is OUTER_S plus OUTER_R's R-only rows. Payloads are random over the int32 range, distinct
within a relation and never the default marker, so that a row's class and its tuples can be told from
the row. Crafted shapes take their sizes from the kernel constants (hwbrj_tables_info after a
materializing join of the same |R| and filter: the outer join runs on its geometry)."""
import ctypes

import numpy as np
import pytest

import shapes

pytestmark = pytest.mark.gpu
INT_MAX, INT_MIN = 2**31 - 1, -2**31
NULL = -2**31  # outer_join_device's default marker


def to_dev(cuda, a):
    return cuda.from_numpy(np.ascontiguousarray(a, dtype=np.int32).reshape(-1, 2)).to("cuda:0")


def _args(hw):
    """The ten modes of tests/test_gpu_semi.py::_args."""
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


MODES = ["blocked_packed", "blocked_code", "blocked_k3", "sectorized_k2", "basic_k1", "basic_k3",
         "two_segments", "global_b4", "nobloom", "blocked_f256"]


@pytest.fixture(scope="module")
def crc(orc):
    return shapes.Crc(orc.crc)


def _u64(rows):
    """Sorted rows, each as one 64-bit word (an exact multiset comparison)."""
    rows = np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1, 2))
    return np.sort(rows.view(np.uint64).ravel())


_payloads, _rel = shapes.payloads, shapes.rel  # (distinct random payloads, none of them NULL)


def _col(pay, null, left):
    """Rows {null, pay} (left) or {pay, null}."""
    pay = np.asarray(pay, dtype=np.int64)
    nul = np.full(pay.size, null, dtype=np.int64)
    return np.stack([nul, pay] if left else [pay, nul], 1).astype(np.int32).reshape(-1, 2)


_REF = {}


def reference(orc, R, S, null=NULL, tag=None):
    """(inner, S-only, R-only) rows on the host; shared between the cases of a test under `tag`."""
    if tag is not None and tag in _REF:
        return _REF[tag]
    inner = orc.join_pairs(R, S) if R.shape[0] and S.shape[0] else np.empty((0, 2), dtype=np.int32)
    s_only = _col(S[~np.isin(S[:, 0], R[:, 0]), 1], null, True)
    r_only = _col(R[~np.isin(R[:, 0], S[:, 0]), 1], null, False)
    ref = (np.asarray(inner, dtype=np.int32).reshape(-1, 2), s_only, r_only)
    if tag is not None:
        _REF[tag] = ref
    return ref


def check(hw, cuda, orc, R, S, args, null=NULL, tag=None, **kw):
    """The three kinds against the host reference; returns ({kind: rows}, Stats of OUTER_S)."""
    dR, dS = to_dev(cuda, R), to_dev(cuda, S)
    inner, s_only, r_only = reference(orc, R, S, null, tag)
    cj = hw.join_device(dR, dS, args)
    got, st_s = {}, None
    for kind in (hw.OUTER_S, hw.OUTER_R, hw.OUTER_FULL):
        parts = [inner] + ([s_only] if kind != hw.OUTER_R else []) + ([r_only] if kind != hw.OUTER_S else [])
        want_cls = (inner.shape[0], s_only.shape[0] if kind != hw.OUTER_R else 0,
                    r_only.shape[0] if kind != hw.OUTER_S else 0)
        st, rows, cls, _ = hw.outer_join_device(dR, dS, args, kind=kind, null_payload=null, **kw)
        rows = rows.cpu().numpy()
        print(f"kind {kind}: {rows.shape[0]} rows, classes {cls} (host {want_cls}), filtered {st.filtered} "
              f"(counting join {cj.filtered}), inner vs counting join {cj.matches}")
        assert cls == want_cls
        assert cls[0] == cj.matches
        assert st.filtered == cj.filtered
        assert st.matches == rows.shape[0] == sum(cls)
        assert np.array_equal(_u64(rows), _u64(np.concatenate(parts)))
        got[kind] = rows
        if kind == hw.OUTER_S:
            st_s = st
    # FULL = OUTER_S + OUTER_R's R-only rows, i.e. FULL + inner = OUTER_S + OUTER_R (as multisets)
    assert np.array_equal(_u64(np.concatenate([got[hw.OUTER_FULL], inner])),
                          _u64(np.concatenate([got[hw.OUTER_S], got[hw.OUTER_R]])))
    return got, st_s


def job_counts(hw, rows, R, S, jobk, null=NULL):
    """(inner, S-only, R-only) rows of `rows` whose tuples have a key in jobk (payloads are distinct
    within a relation and never null)."""
    rp, sp = R[np.isin(R[:, 0], jobk), 1], S[np.isin(S[:, 0], jobk), 1]
    in_r, in_s = np.isin(rows[:, 0], rp), np.isin(rows[:, 1], sp)
    return (int((in_r & in_s).sum()), int((in_s & (rows[:, 0] == null)).sum()),
            int((in_r & (rows[:, 1] == null)).sum()))


def geometry(hw, cuda, args, name, nR):
    """tables_info of a materializing join of |R| = nR under args (throw-away keys)."""
    return shapes.mat_geometry(hw, lambda a: to_dev(cuda, a), args, name, nR)


def same_geometry(hw, cuda, R, args, info):
    """A materializing join of this R and args reports the geometry the keys were crafted for."""
    shapes.same_geometry(hw, lambda a: to_dev(cuda, a), R, args, info)


# ------------------------------------------------------------------------------ 1: every mode
MODE_SEED = 5


def mode_relations(orc, seed=MODE_SEED):
    """|R| = 40,000 distinct keys; |S| = 300,000: 60,000 rows draw from 30,000 of R's keys, 239,000
    have keys R lacks, and 1,000 rows appear twice. So 10,000 R keys have no partner. Under every
    filter of _args some of the 239,000 survive it (tests/test_outer_abi.py checks this seed against
    the oracle's counting join on the CPU)."""
    rng = np.random.default_rng(seed)
    R = orc.relation(40000, 2, 40000, 40000, 1.0, 1)
    assert np.unique(R[:, 0]).size == 40000
    hit = rng.choice(R[:, 0], 30000, replace=False)
    Sk = np.concatenate([hit[rng.integers(0, hit.size, size=60000)],
                         rng.integers(40001, INT_MAX, size=239000, endpoint=True)])
    rng.shuffle(Sk)
    R[:, 1] = _payloads(R.shape[0], rng)
    S = _rel(Sk, rng)
    S = np.concatenate([S, S[rng.choice(S.shape[0], 1000, replace=False)]])
    # (the 1,000 repeated rows repeat a payload: the only equal S payloads of this test)
    return R, S


@pytest.mark.parametrize("name", MODES)
def test_every_mode(hw, cuda, orc, name):
    R, S = mode_relations(orc)
    assert S.shape[0] == 300000
    got, st = check(hw, cuda, orc, R, S, _args(hw)[name], tag="every_mode")
    inner, s_only, r_only = _REF["every_mode"]
    assert min(inner.shape[0], s_only.shape[0], r_only.shape[0]) >= 1000
    if name != "nobloom":  # false-positive survivors are present: each comes out S-only, once
        partnered = int(np.isin(S[:, 0], R[:, 0]).sum())
        print(f"filtered {st.filtered}, S rows with a partner {partnered}")
        assert st.filtered > partnered


# --------------------------------------------------------------- 2: duplicates on both sides
@pytest.mark.parametrize("name", ["blocked_packed", "basic_k1", "nobloom"])
def test_duplicates_on_both_sides(hw, cuda, orc, crc, name):
    """5,000 R keys three times each, with INT_MAX, INT_MIN, 0, -1 and the key whose code is the
    kernels' empty-slot value; S holds key i (i mod 5) times (the special keys 0 to 4 times) and
    7,000 keys R lacks: inner = 3 x the hits, R-only = 3 rows for every key hit 0 times."""
    R, S, args, info = shapes.duplicates_on_both_sides(crc, _args(hw)[name])
    special, hits = info["special"], info["hits"]
    got, _ = check(hw, cuda, orc, R, S, args, tag="duplicates")
    inner, s_only, r_only = _REF["duplicates"]
    assert inner.shape[0] == 3 * int(hits.sum())
    assert r_only.shape[0] == 3 * int((hits == 0).sum())
    assert s_only.shape[0] == 7000
    # the first special key (hit 0 times): its three R rows are R-only rows of OUTER_R
    assert job_counts(hw, got[hw.OUTER_R], R, S, special[:1]) == (0, 0, 3)
    assert job_counts(hw, got[hw.OUTER_FULL], R, S, special[4:5]) == (12, 0, 0)


# -------------------------------------------------------------- 3: a hot R key across pieces
@pytest.mark.parametrize("name", ["nobloom", "blocked_packed"])
def test_hot_r_key_across_pieces(hw, cuda, orc, crc, name):
    """One job holds an R key 2 kMatPiece + 5 times, keys 11, 12, 13 and six keys no S row has (three
    at the head of R, three at its tail: the job's first and last pieces), more than kMatRCap tuples.
    Its survivors: 40 of the hot key, 10 of 11, 10 of 12, none of 13, 50 of keys R lacks. A flag or a
    mark decided per piece instead of per job gives other counts."""
    R, S, args, info = shapes.hot_r_key_across_pieces(
        crc, _args(hw)[name], lambda nR: geometry(hw, cuda, _args(hw)[name], name, nR))
    q0, sub0, hot = info["q0"], info["sub0"], info["hot"]
    same_geometry(hw, cuda, R, args, info)
    got, _ = check(hw, cuda, orc, R, S, args)
    jobk = crc.key_of(shapes.job_codes(info, q0, sub0, np.arange(3000)))
    assert job_counts(hw, got[hw.OUTER_FULL], R, S, jobk) == (40 * hot + 20, 50, 7)
    assert job_counts(hw, got[hw.OUTER_S], R, S, jobk) == (40 * hot + 20, 50, 0)
    assert job_counts(hw, got[hw.OUTER_R], R, S, jobk) == (40 * hot + 20, 0, 7)


# ------------------------------------------------------------------- 4: empty sides of a job
def test_empty_sides_of_a_job(hw, cuda, orc, crc):
    """Without a filter, crafted codes: (a) partition qa holds 100 S rows and no R: S-only, none
    inner; (b) partition qb holds 100 R rows and no S row at all (no probe items: k_join_mat's
    early return): R-only; (c) in partition qc sub s1 holds 100 R rows and no survivors, sub s2 holds
    R and S: s1's R rows are R-only."""
    rng = np.random.default_rng(44)
    nR, qa, qb, qc = 20000, 300, 301, 302
    info = geometry(hw, cuda, None, "nobloom", nR)
    assert info["F"] > qc and info["NSUB"] >= 2
    s1, s2 = (1, 2) if info["NSUB"] > 2 else (0, 1)
    v = np.arange(100, dtype=np.uint64) * np.uint64(3) + np.uint64(1)
    a_s = shapes.job_codes(info, qa, 0, v)
    b_r = shapes.job_codes(info, qb, s1 % info["NSUB"], v)
    c1_r = shapes.job_codes(info, qc, s1, v)
    c2_r = shapes.job_codes(info, qc, s2, v)
    c2_s = shapes.job_codes(info, qc, s2, np.concatenate([v[:60], v[:20], 1000 + np.arange(30)]))
    nf = nR - 300
    fill = shapes.filler_codes(info, nf + 3000, {qa, qb, qc}, 1)
    Rc = np.concatenate([b_r, c1_r, c2_r, fill[:nf]])
    Sc = np.concatenate([a_s, c2_s, fill[nf - 3000:]])
    rng.shuffle(Rc)
    rng.shuffle(Sc)
    R, S = _rel(crc.key_of(Rc), rng), _rel(crc.key_of(Sc), rng)
    same_geometry(hw, cuda, R, None, info)
    got, _ = check(hw, cuda, orc, R, S, None)
    full = got[hw.OUTER_FULL]
    assert job_counts(hw, full, R, S, crc.key_of(a_s)) == (0, 100, 0)
    assert job_counts(hw, full, R, S, crc.key_of(b_r)) == (0, 0, 100)
    assert job_counts(hw, full, R, S, crc.key_of(c1_r)) == (0, 0, 100)
    assert job_counts(hw, full, R, S, crc.key_of(np.concatenate([c2_r, c2_s]))) == (80, 30, 40)
    assert job_counts(hw, got[hw.OUTER_R], R, S, crc.key_of(b_r)) == (0, 0, 100)
    assert job_counts(hw, got[hw.OUTER_S], R, S, crc.key_of(a_s)) == (0, 100, 0)


# ------------------------------------------------------------- 5: more than kMatDesc descriptors
@pytest.mark.parametrize("name", ["nobloom", "blocked_f256"])
def test_more_descriptors_than_a_batch(hw, cuda, orc, crc, name):
    """A partition of kMatDesc * BSW * 32 + 1 R tuples (more than kMatDesc build sweeps: several R
    descriptor batches per job), 60,000 distinct keys repeated all over it; S has rows of 50,000 of
    them only, so R-only rows come from every descriptor batch."""
    R, S, args, info = shapes.more_descriptors_than_a_batch(
        crc, _args(hw)[name], lambda nR: geometry(hw, cuda, _args(hw)[name], name, nR))
    n_q, member, Rc, Sc = info["n_q"], info["member"], info["Rc"], info["Sc"]
    got, _ = check(hw, cuda, orc, R, S, args)
    n_lone = int((~np.isin(Rc[np.isin(Rc, member)], Sc)).sum())
    assert n_lone > n_q // 2
    assert job_counts(hw, got[hw.OUTER_R], R, S, crc.key_of(member))[2] == n_lone


# ----------------------------------------------------------------------------- 6: edge sizes
@pytest.mark.parametrize("name", ["blocked_packed", "nobloom"])
def test_edge_sizes(hw, cuda, orc, name):
    rng = np.random.default_rng(13)
    for nR, nS in [(0, 1000), (1000, 0), (1, 1), (7, 33), (4097, 4099)]:
        R = _rel(rng.permutation(nR) + 1, rng)
        S = _rel(rng.integers(0, 2 * max(nR, 1) + 2, size=nS), rng)
        got, _ = check(hw, cuda, orc, R, S, _args(hw)[name])
        if nR == 0:  # every S row is S-only
            assert np.array_equal(_u64(got[hw.OUTER_S]), _u64(_col(S[:, 1], NULL, True)))
            assert got[hw.OUTER_R].shape[0] == 0
        if nS == 0:  # every R row is R-only
            assert np.array_equal(_u64(got[hw.OUTER_R]), _u64(_col(R[:, 1], NULL, False)))
            assert got[hw.OUTER_S].shape[0] == 0


# ---------------------------------------------------------------------- 7: capacity contract
def test_capacity_contract(hw, cuda, orc):
    rng = np.random.default_rng(77)
    R = orc.relation(10000, 2, 10000, 10000, 1.0, 3)
    S = orc.relation(100000, 2, INT_MAX, 10000, 0.05, 4)
    R[:, 1] = _payloads(R.shape[0], rng)
    S[:, 1] = _payloads(S.shape[0], rng)
    args = _args(hw)["blocked_packed"]
    check(hw, cuda, orc, R, S, args, capacity=10)  # (the wrapper runs again at the exact size)
    dR, dS = to_dev(cuda, R), to_dev(cuda, S)
    a = args._c()
    inner, s_only, r_only = reference(orc, R, S)
    assert min(inner.shape[0], s_only.shape[0], r_only.shape[0]) > 1000
    for kind in (hw.OUTER_S, hw.OUTER_R, hw.OUTER_FULL):
        want = np.concatenate([inner] + ([s_only] if kind != hw.OUTER_R else []) +
                              ([r_only] if kind != hw.OUTER_S else []))
        cap, guard = 1000, 4096
        buf = cuda.full((cap + guard, 2), 0x5A5A5A5A, dtype=cuda.int32, device="cuda:0")
        n, st, cls = ctypes.c_uint64(), hw._Stats(), (ctypes.c_uint64 * 3)()
        rc = hw.lib().hwbrj_join_outer_device(dR.data_ptr(), dR.shape[0], dS.data_ptr(), dS.shape[0],
                                              ctypes.byref(a), kind, NULL, buf.data_ptr(), cap, ctypes.byref(n),
                                              cls, None, ctypes.byref(st), None)
        assert (rc, n.value, st.matches, sum(cls)) == (7, want.shape[0], want.shape[0], want.shape[0])
        host = buf.cpu().numpy()
        assert (host[cap:] == 0x5A5A5A5A).all()  # nothing past capacity
        rows = set(map(tuple, want.tolist()))
        assert all(tuple(r) in rows for r in host[:cap].tolist())  # the first `capacity` rows are rows
        n0 = ctypes.c_uint64()
        rc = hw.lib().hwbrj_join_outer_device(dR.data_ptr(), dR.shape[0], dS.data_ptr(), dS.shape[0],
                                              ctypes.byref(a), kind, NULL, None, 0, ctypes.byref(n0), None, None,
                                              None, None)
        assert (rc, n0.value) == (7, want.shape[0])  # count only


# ------------------------------------------------------------------ 8: a colliding null marker
@pytest.mark.parametrize("name", ["blocked_packed", "global_b4"])
def test_colliding_null_marker(hw, cuda, orc, name):
    """The marker is a value that 100 R payloads and 100 S payloads carry too (matched and unmatched
    rows among them): the library writes it and never reads it, so the multisets stay exact."""
    rng = np.random.default_rng(88)
    null = 123456789
    Rk = rng.choice(np.arange(1, 40000), 8000, replace=False)
    Sk = rng.integers(1, 60000, size=50000)
    R, S = _rel(Rk, rng), _rel(Sk, rng)
    R[rng.choice(R.shape[0], 100, replace=False), 1] = null
    S[rng.choice(S.shape[0], 100, replace=False), 1] = null
    check(hw, cuda, orc, R, S, _args(hw)[name], null=null)


# ------------------------------------------------------------------------ 9: skewed relations
@pytest.mark.parametrize("name", ["blocked_packed", "basic_k1", "nobloom"])
def test_skewed_partitions(hw, cuda, orc, name):
    """The hot-key relations of test_gpu_semi.py::test_skewed_partitions (key 88 in a tenth of S, key
    77 in a third of R): the scatters' skew path with both payloads, and the emission."""
    rng = np.random.default_rng(9)
    Rk = np.concatenate([np.full(20000, 77), np.full(100, 88), rng.integers(-5000, 5000, size=40000),
                         [INT_MAX, -INT_MAX - 1]])
    Sk = np.concatenate([np.full(500, 77), np.full(100000, 88), rng.integers(-6000, 6000, size=900000),
                         [INT_MAX, -INT_MAX - 1, 77]])
    rng.shuffle(Rk)
    rng.shuffle(Sk)
    R, S = _rel(Rk, rng), _rel(Sk, rng)
    check(hw, cuda, orc, R, S, _args(hw)[name], tag="skew")


# --------------------------------------------------------------- 10: neighbours still work
def test_neighbours_still_work(hw, cuda, orc):
    """After an outer join the table readback answers 13, and a materializing join and a semi-join of
    the same inputs still equal their references (they share the marks and the result slot)."""
    rng = np.random.default_rng(101)
    R = _rel(rng.choice(np.arange(1, 60000), 20000, replace=False), rng)
    S = _rel(rng.integers(1, 90000, size=120000), rng)
    args = _args(hw)["blocked_packed"]
    dR, dS = to_dev(cuda, R), to_dev(cuda, S)
    for a in (args, _args(hw)["global_b4"]):
        hw.outer_join_device(dR, dS, a, kind=hw.OUTER_FULL)
        with pytest.raises(hw.TablesError) as ei:
            hw.tables_info()
        assert ei.value.code == 13
    check(hw, cuda, orc, R, S, args)
    _, pairs, _ = hw.join_materialize_device(dR, dS, args)
    assert np.array_equal(_u64(pairs.cpu().numpy()), _u64(orc.join_pairs(R, S)))
    mask = np.isin(S[:, 0], R[:, 0])
    for anti in (False, True):
        _, rows, _ = hw.semi_join_device(dR, dS, args, anti=anti)
        assert np.array_equal(_u64(rows.cpu().numpy()), _u64(S[~mask] if anti else S[mask]))
