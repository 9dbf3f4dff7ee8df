"""The group join (hwbrj_join_group_device: k_join_group, the global-mode side pass).

The reference of every check is computed on the host in numpy from the inputs: the unique S keys with
their counts and int64 payload sums, looked up per R row (`reference`; tests/test_group_abi.py pins
it to the oracle's pairs on the CPU). R payloads are distinct, so the rows of a kind are compared
exactly after sorting by r_payload. Every case runs both kinds and also checks that GROUP_MATCHED is
GROUP_ALL's rows with count > 0, that GROUP_ALL has |R| rows, n_pairs and `filtered` against the
counting join, and stats.matches against the row count. S payloads are random over the int32 range
unless a case says otherwise. Relations, filter modes and the crafted shapes are those of
tests/test_gpu_outer.py (sizes from the kernel constants: hwbrj_tables_info after a materializing
join of the same |R| and filter, on whose geometry the group join runs)."""
import ctypes

import numpy as np
import pytest

import shapes
import test_gpu_outer as t

pytestmark = pytest.mark.gpu
INT_MAX, INT_MIN = 2**31 - 1, -2**31


def reference(R, S):
    """(|R|, 3) int64 rows {r_payload, count, sum} in R's order: per R row the number of S rows with
    its key and the int64 sum of their payloads."""
    R, S = np.asarray(R).reshape(-1, 2), np.asarray(S).reshape(-1, 2)
    cnt, sm = np.zeros(R.shape[0], dtype=np.int64), np.zeros(R.shape[0], dtype=np.int64)
    if R.shape[0] and S.shape[0]:
        order = np.argsort(S[:, 0], kind="stable")
        uk, start, n = np.unique(S[order, 0], return_index=True, return_counts=True)
        sums = np.add.reduceat(S[order, 1].astype(np.int64), start)
        i = np.minimum(np.searchsorted(uk, R[:, 0]), uk.size - 1)
        hit = uk[i] == R[:, 0]
        cnt, sm = np.where(hit, n[i], 0).astype(np.int64), np.where(hit, sums[i], 0).astype(np.int64)
    return np.stack([R[:, 1].astype(np.int64), cnt, sm], 1)


def _sorted(rows):
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    return rows[np.argsort(rows[:, 0], kind="stable")]


def _host(rows):
    """GroupRows -> (n, 3) int64 {r_payload, count, sum}, checking the views against raw."""
    raw = rows.raw.cpu().numpy()
    out = np.stack([rows.r_payload.cpu().numpy().astype(np.int64), rows.count.cpu().numpy(),
                    rows.sum.cpu().numpy()], 1).reshape(-1, 3)
    assert raw.dtype == np.int64 and raw.shape == (out.shape[0], 2)
    w0 = raw[:, 0].view(np.uint64)
    assert np.array_equal(out[:, 0], (w0 & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32))
    assert np.array_equal(out[:, 1], (w0 >> np.uint64(32)).astype(np.int64))
    assert np.array_equal(out[:, 2], raw[:, 1])
    return out


_REF = {}


def check(hw, cuda, R, S, args, tag=None, **kw):
    """Both kinds against the host reference; returns {kind: rows sorted by r_payload}."""
    dR, dS = t.to_dev(cuda, R), t.to_dev(cuda, S)
    if tag is None or tag not in _REF:
        ref = _sorted(reference(R, S))
        ref.setflags(write=False)
        if tag is not None:
            _REF[tag] = ref
    else:
        ref = _REF[tag]
    assert np.unique(R[:, 1]).size == R.shape[0]  # (distinct R payloads: rows are told apart)
    cj = hw.join_device(dR, dS, args)
    got = {}
    for kind in (hw.GROUP_MATCHED, hw.GROUP_ALL):
        want = ref if kind == hw.GROUP_ALL else ref[ref[:, 1] > 0]
        st, rows, pairs, _ = hw.group_join_device(dR, dS, args, kind=kind, **kw)
        rows = _sorted(_host(rows))
        print(f"kind {kind}: {rows.shape[0]} rows (host {want.shape[0]}), n_pairs {pairs} (host {int(ref[:, 1].sum())}, "
              f"counting join {cj.matches}), filtered {st.filtered} (counting join {cj.filtered})")
        assert rows.shape[0] == want.shape[0] == st.matches
        assert pairs == cj.matches == int(ref[:, 1].sum())
        assert st.filtered == cj.filtered
        assert np.array_equal(rows, want)
        got[kind] = rows
    assert got[hw.GROUP_ALL].shape[0] == R.shape[0]
    assert np.array_equal(got[hw.GROUP_MATCHED], got[hw.GROUP_ALL][got[hw.GROUP_ALL][:, 1] > 0])
    return got


def rows_of(rows, R, keys):
    """The rows of the R tuples whose key is in `keys`."""
    return rows[np.isin(rows[:, 0], R[np.isin(R[:, 0], keys), 1])]


@pytest.fixture(scope="module")
def crc(orc):
    return shapes.Crc(orc.crc)


# ------------------------------------------------------------------------------ 1: every mode
@pytest.mark.parametrize("name", t.MODES)
def test_every_mode(hw, cuda, orc, name):
    R, S = t.mode_relations(orc)
    got = check(hw, cuda, R, S, t._args(hw)[name], tag="every_mode")
    assert got[hw.GROUP_MATCHED].shape[0] == int(np.isin(R[:, 0], S[:, 0]).sum()) >= 1000
    assert got[hw.GROUP_ALL].shape[0] - got[hw.GROUP_MATCHED].shape[0] >= 1000


# --------------------------------------------------------------- 2: duplicates on both sides
@pytest.mark.parametrize("name", ["blocked_packed", "basic_k1", "nobloom"])
def test_duplicates_on_both_sides(hw, cuda, crc, name):
    """5,000 R keys three times each, with INT_MAX, INT_MIN, 0, -1 and the key whose code is the
    kernels' empty-slot value; S holds key i (i mod 5) times (the special keys 0 to 4 times) and
    7,000 keys R lacks. The three copies of a key carry the same count and sum; the keys hit 0 times
    appear only under GROUP_ALL."""
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
    R, S = t._rel(Rk, rng), t._rel(Sk, rng)
    got = check(hw, cuda, R, S, t._args(hw)[name], tag="duplicates")
    rows = got[hw.GROUP_ALL]
    assert got[hw.GROUP_MATCHED].shape[0] == 3 * int((hits > 0).sum())
    for key, h in zip(keys[:50], hits[:50]):
        mine = rows_of(rows, R, [key])
        assert mine.shape[0] == 3 and (mine[:, 1] == h).all() and np.unique(mine[:, 2]).size == 1
        assert rows_of(got[hw.GROUP_MATCHED], R, [key]).shape[0] == (3 if h else 0)


# -------------------------------------------------------------- 3: a hot R key across pieces
@pytest.mark.parametrize("name", ["nobloom", "blocked_packed"])
def test_hot_r_key_across_pieces(hw, cuda, crc, name):
    """One job holds an R key 2 kMatPiece + 5 times, keys 11, 12, 13 and six keys no S row has (three
    at the head of R, three at its tail: the job's first and last pieces), more than kMatRCap tuples.
    Its survivors: 40 of the hot key, 10 of 11, 10 of 12, none of 13, 50 of keys R lacks. Every hot
    copy, in whichever piece, has count 40 and the same sum: accumulators cleared per survivor batch
    instead of per piece, or written before the last batch, give other numbers."""
    rng = np.random.default_rng(33)
    args = t._args(hw)[name]
    nR = 20000
    info = t.geometry(hw, cuda, args, name, nR)
    q0, sub0 = 17, 1
    hot = 2 * info["m_piece"] + 5
    rv = np.concatenate([np.full(hot, 7), [11, 12, 13]])
    lone = 2000 + np.arange(6)
    assert rv.size + lone.size >= info["m_rcap"] + 1
    nf = nR - rv.size - lone.size
    fill = shapes.filler_codes(info, nf + 3000, {q0}, 1)  # distinct: R takes the first nf
    mid = np.concatenate([shapes.job_codes(info, q0, sub0, rv), fill[:nf]])
    rng.shuffle(mid)
    lc = shapes.job_codes(info, q0, sub0, lone)
    Rc = np.concatenate([lc[:3], mid, lc[3:]])
    sv = np.concatenate([np.full(40, 7), np.repeat([11, 12], 10), 1000 + np.arange(50)])
    Sc = np.concatenate([shapes.job_codes(info, q0, sub0, sv), fill[nf - 3000:]])  # 3,000 of R's, 3,000 not
    rng.shuffle(Sc)
    R, S = t._rel(crc.key_of(Rc), rng), t._rel(crc.key_of(Sc), rng)
    t.same_geometry(hw, cuda, R, args, info)
    got = check(hw, cuda, R, S, args)
    key = lambda v: crc.key_of(shapes.job_codes(info, q0, sub0, np.atleast_1d(v)))
    for kind in (hw.GROUP_MATCHED, hw.GROUP_ALL):
        mine = rows_of(got[kind], R, key(7))
        want_sum = int(S[np.isin(S[:, 0], key(7)), 1].astype(np.int64).sum())
        assert mine.shape[0] == hot and (mine[:, 1] == 40).all() and (mine[:, 2] == want_sum).all()
        assert (rows_of(got[kind], R, key([11, 12]))[:, 1] == 10).all()
    jobk = key(np.arange(3000))
    assert rows_of(got[hw.GROUP_MATCHED], R, jobk).shape[0] == hot + 2
    mine = rows_of(got[hw.GROUP_ALL], R, jobk)
    assert mine.shape[0] == hot + 9 and int((mine[:, 1] == 0).sum()) == 7 and int(mine[:, 1].sum()) == 40 * hot + 20


# ------------------------------------------------------ 4: hot S keys and 64-bit sums
@pytest.mark.parametrize("name", ["nobloom", "blocked_packed", "basic_k1"])
def test_hot_s_keys_and_64_bit_sums(hw, cuda, crc, name):
    """Three R keys (in one job where the partition is a code digit) with 200,000 S rows of payload
    INT_MAX (the sum passes 2^32: the carry into the high word), 70,000 of INT_MIN (sign extension)
    and 100,001 alternating INT_MAX / INT_MIN: more than kMatPiece survivors over many batches on
    one accumulator, beside ordinary filler. Then the same with every one of the three keys twice in
    R, which takes the hash table."""
    rng = np.random.default_rng(66)
    args = t._args(hw)[name]
    nR = 20000
    info = t.geometry(hw, cuda, args, name, nR)
    if info["sub_shift"] > 0:
        q0 = 9
        k3 = crc.key_of(shapes.job_codes(info, q0, 1, [5, 6, 7])).astype(np.int64)
        fill = crc.key_of(shapes.filler_codes(info, nR + 3000, {q0}, 1)).astype(np.int64)
    else:  # (basic filters: the partition is no code digit; three plain keys)
        k3 = np.array([-3, 123456, INT_MAX], dtype=np.int64)
        fill = 10**6 + rng.permutation(nR + 3000).astype(np.int64)
    alt = np.where(np.arange(100001) % 2 == 0, INT_MAX, INT_MIN)
    hot_k = np.concatenate([np.full(200000, k3[0]), np.full(70000, k3[1]), np.full(100001, k3[2])])
    hot_p = np.concatenate([np.full(200000, INT_MAX), np.full(70000, INT_MIN), alt])
    Sf = t._rel(fill[nR - 3000:], rng)  # 3,000 of R's filler keys, 3,000 R lacks
    S = np.concatenate([np.stack([hot_k, hot_p], 1).astype(np.int32), Sf])
    S = S[rng.permutation(S.shape[0])]
    want = {int(k3[0]): (200000, 200000 * INT_MAX), int(k3[1]): (70000, 70000 * INT_MIN),
            int(k3[2]): (100001, 50001 * INT_MAX + 50000 * INT_MIN)}
    assert want[int(k3[0])][1] > 2**32 and want[int(k3[1])][1] < -2**32
    for copies in (1, 2):
        Rk = np.concatenate([np.repeat(k3, copies), fill[:nR - 3 * copies]])
        rng.shuffle(Rk)
        R = t._rel(Rk, rng)
        if info["sub_shift"] > 0:
            t.same_geometry(hw, cuda, R, args, info)
        got = check(hw, cuda, R, S, args)
        for kind in (hw.GROUP_MATCHED, hw.GROUP_ALL):
            for k, (c, s) in want.items():
                mine = rows_of(got[kind], R, [k])
                assert mine.shape[0] == copies and (mine[:, 1] == c).all() and (mine[:, 2] == s).all()


# ------------------------------------------------------------------- 5: empty sides of a job
def test_empty_sides_of_a_job(hw, cuda, crc):
    """Without a filter, crafted codes: (a) partition qa holds 100 S rows and no R: no rows; (b)
    partition qb holds 100 R rows and no S row at all (no probe items): GROUP_ALL rows with count 0,
    no GROUP_MATCHED row; (c) in partition qc sub s1 holds 100 R rows and no survivors, beside sub s2
    with R and S."""
    rng = np.random.default_rng(44)
    nR, qa, qb, qc = 20000, 300, 301, 302
    info = t.geometry(hw, cuda, None, "nobloom", nR)
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
    R, S = t._rel(crc.key_of(Rc), rng), t._rel(crc.key_of(Sc), rng)
    t.same_geometry(hw, cuda, R, None, info)
    got = check(hw, cuda, R, S, None)
    m, a = got[hw.GROUP_MATCHED], got[hw.GROUP_ALL]
    for codes in (b_r, c1_r):
        mine = rows_of(a, R, crc.key_of(codes))
        assert mine.shape[0] == 100 and not mine[:, 1:].any()
        assert rows_of(m, R, crc.key_of(codes)).shape[0] == 0
    mine = rows_of(a, R, crc.key_of(c2_r))
    assert mine.shape[0] == 100 and int(mine[:, 1].sum()) == 80 and int((mine[:, 1] == 2).sum()) == 20
    assert rows_of(m, R, crc.key_of(c2_r)).shape[0] == 60


# ------------------------------------------------------------- 6: more than kMatDesc descriptors
@pytest.mark.parametrize("name", ["nobloom", "blocked_f256"])
def test_more_descriptors_than_a_batch(hw, cuda, crc, name):
    """A partition of kMatDesc * BSW * 32 + 1 R tuples (more than kMatDesc build sweeps: several R
    descriptor batches per job), 60,000 distinct keys repeated all over it; S has rows of 50,000 of
    them only, so rows with and without partners come from every descriptor batch."""
    rng = np.random.default_rng(55)
    args = t._args(hw)[name]
    q0, fill = 5, 20000
    probe = t.geometry(hw, cuda, args, name, 8)
    n_q = probe["m_desc"] * probe["BSW"] * 32 + 1
    nR = n_q + fill
    info = t.geometry(hw, cuda, args, name, nR)
    assert (info["m_desc"], info["BSW"]) == (probe["m_desc"], probe["BSW"])
    lf = info["F"].bit_length() - 1
    hi = rng.choice(1 << min(32 - lf, 24), 66000, replace=False).astype(np.uint64)
    qcodes = (np.uint64(q0) | (hi << np.uint64(lf))).astype(np.uint32)
    member, absent = qcodes[:60000], qcodes[60000:]
    Rc = np.concatenate([member[rng.integers(0, member.size, size=n_q)], shapes.filler_codes(info, fill, {q0}, 1)])
    Sc = np.concatenate([member[rng.integers(0, 50000, size=3000)], absent[rng.integers(0, absent.size, size=3000)],
                         Rc[n_q:n_q + 3000], shapes.filler_codes(info, 3000, {q0}, 777)])
    rng.shuffle(Rc)
    rng.shuffle(Sc)
    R, S = t._rel(crc.key_of(Rc), rng), t._rel(crc.key_of(Sc), rng)
    got = check(hw, cuda, R, S, args)
    n_lone = int((~np.isin(Rc[np.isin(Rc, member)], Sc)).sum())
    mine = rows_of(got[hw.GROUP_ALL], R, crc.key_of(member))
    assert n_lone > n_q // 2 and mine.shape[0] == n_q and int((mine[:, 1] == 0).sum()) == n_lone


# ----------------------------------------------------------------------------- 7: edge sizes
@pytest.mark.parametrize("name", ["blocked_packed", "nobloom"])
def test_edge_sizes(hw, cuda, name):
    rng = np.random.default_rng(13)
    for nR, nS in [(0, 1000), (1000, 0), (1, 1), (7, 33), (4097, 4099)]:
        R = t._rel(rng.permutation(nR) + 1, rng)
        S = t._rel(rng.integers(0, 2 * max(nR, 1) + 2, size=nS), rng)
        got = check(hw, cuda, R, S, t._args(hw)[name])
        if nR == 0 or nS == 0:
            assert got[hw.GROUP_MATCHED].shape[0] == 0 and not got[hw.GROUP_ALL][:, 1:].any()


# ---------------------------------------------------------------------- 8: capacity contract
@pytest.mark.parametrize("name", ["blocked_packed", "global_b4"])
def test_capacity_contract(hw, cuda, orc, name):
    rng = np.random.default_rng(77)
    R = orc.relation(10000, 2, 10000, 10000, 1.0, 3)
    S = orc.relation(100000, 2, INT_MAX, 10000, 0.05, 4)
    R[:, 1] = t._payloads(R.shape[0], rng)
    S[:, 1] = t._payloads(S.shape[0], rng)
    args = t._args(hw)[name]
    check(hw, cuda, R, S, args, capacity=10)  # (the wrapper runs again at the exact size)
    dR, dS = t.to_dev(cuda, R), t.to_dev(cuda, S)
    a = args._c()
    ref = _sorted(reference(R, S))
    n_matched = int((ref[:, 1] > 0).sum())
    assert 1000 < n_matched < R.shape[0] - 1000

    def call(kind, buf, cap, n, pairs=None, st=None):
        return hw.lib().hwbrj_join_group_device(dR.data_ptr(), dR.shape[0], dS.data_ptr(), dS.shape[0], ctypes.byref(a),
                                                kind, buf, cap, ctypes.byref(n), pairs, None, st, None)

    for kind, want in ((hw.GROUP_MATCHED, ref[ref[:, 1] > 0]), (hw.GROUP_ALL, ref)):
        cap, guard = 1000, 4096
        buf = cuda.full((cap + guard, 2), 0x5A5A5A5A5A5A5A5A, dtype=cuda.int64, device="cuda:0")
        n, pairs, st = ctypes.c_uint64(), ctypes.c_uint64(), hw._Stats()
        rc = call(kind, buf.data_ptr(), cap, n, ctypes.byref(pairs), ctypes.byref(st))
        assert (rc, n.value, st.matches, pairs.value) == (7, want.shape[0], want.shape[0], int(ref[:, 1].sum()))
        host = buf.cpu().numpy()
        assert (host[cap:] == 0x5A5A5A5A5A5A5A5A).all()  # nothing past capacity
        w0 = host[:cap, 0].view(np.uint64)
        first = np.stack([(w0 & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32).astype(np.int64),
                          (w0 >> np.uint64(32)).astype(np.int64), host[:cap, 1]], 1)
        rows = set(map(tuple, want.tolist()))
        assert len(set(map(tuple, first.tolist()))) == cap
        assert all(tuple(r) in rows for r in first.tolist())  # the first `capacity` rows are rows
        n0 = ctypes.c_uint64()
        assert (call(kind, None, 0, n0), n0.value) == (7, want.shape[0])  # count only
        exact = cuda.empty((want.shape[0], 2), dtype=cuda.int64, device="cuda:0")
        assert (call(kind, exact.data_ptr(), want.shape[0], n0), n0.value) == (0, want.shape[0])


# ------------------------------------------------------------------------ 9: skewed relations
@pytest.mark.parametrize("name", ["blocked_packed", "basic_k1", "nobloom"])
def test_skewed_partitions(hw, cuda, name):
    """The hot-key relations of test_gpu_outer.py::test_skewed_partitions (key 88 in a tenth of S, key
    77 in a third of R): the scatters' skew path, a hot S key on a hundred-odd accumulators, and
    20,000 copies of an R key over many pieces."""
    rng = np.random.default_rng(9)
    Rk = np.concatenate([np.full(20000, 77), np.full(100, 88), rng.integers(-5000, 5000, size=40000),
                         [INT_MAX, -INT_MAX - 1]])
    Sk = np.concatenate([np.full(500, 77), np.full(100000, 88), rng.integers(-6000, 6000, size=900000),
                         [INT_MAX, -INT_MAX - 1, 77]])
    rng.shuffle(Rk)
    rng.shuffle(Sk)
    R, S = t._rel(Rk, rng), t._rel(Sk, rng)
    got = check(hw, cuda, R, S, t._args(hw)[name], tag="skew")
    mine = rows_of(got[hw.GROUP_MATCHED], R, [88])
    n88 = int((Rk == 88).sum())  # (the random keys add a few copies to the 100)
    assert mine.shape[0] == n88 >= 100 and (mine[:, 1] == int((Sk == 88).sum())).all()
    assert mine[0, 1] >= 100000 and np.unique(mine[:, 2]).size == 1


# --------------------------------------------------------------- 10: neighbours still work
def test_neighbours_still_work(hw, cuda, orc):
    """After a group join the table readback answers 13; a counting join, a materializing join and an
    OUTER_FULL of the same inputs still give their own results, and a second group join the first
    one's rows (accumulators and counters are zeroed per call)."""
    rng = np.random.default_rng(101)
    R = t._rel(rng.choice(np.arange(1, 60000), 20000, replace=False), rng)
    S = t._rel(rng.integers(1, 90000, size=120000), rng)
    args = t._args(hw)["blocked_packed"]
    dR, dS = t.to_dev(cuda, R), t.to_dev(cuda, S)
    for a in (args, t._args(hw)["global_b4"]):
        first = check(hw, cuda, R, S, a)
        with pytest.raises(hw.TablesError) as ei:
            hw.tables_info()
        assert ei.value.code == 13
        again = check(hw, cuda, R, S, a)
        for kind in first:
            assert np.array_equal(first[kind], again[kind])
    pairs_ref = orc.join_pairs(R, S)
    assert hw.join_device(dR, dS, args).matches == pairs_ref.shape[0]
    hw.group_join_device(dR, dS, args, kind=hw.GROUP_ALL)
    _, pairs, _ = hw.join_materialize_device(dR, dS, args)
    assert np.array_equal(t._u64(pairs.cpu().numpy()), t._u64(pairs_ref))
    hw.group_join_device(dR, dS, args, kind=hw.GROUP_MATCHED)
    t.check(hw, cuda, orc, R, S, args)  # (the three outer kinds against their host reference)
