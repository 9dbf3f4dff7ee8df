"""The group join's MIN / MAX form (hwbrj_join_group_minmax_device: k_join_group<., GRP_COUNT_MINMAX>,
the global-mode side pass's min/max kernels).

The reference of every check is computed on the host in numpy from the inputs: the unique S keys with
their counts and the smallest and largest payload as signed int32, looked up per R row, and the
identities INT32_MAX / INT32_MIN where an R row has no partner (`reference`;
tests/test_group_minmax_abi.py pins it to the oracle's pairs on the CPU). R payloads are distinct, so
the rows of a kind are compared exactly after sorting by r_payload. Every case runs both kinds and
also checks that GROUP_MATCHED is GROUP_ALL's rows with count > 0, that GROUP_ALL has |R| rows,
n_pairs and `filtered` against the counting join, stats.matches against the row count, and the count
column against group_join_device's for the same inputs. Relations, filter modes and the crafted
shapes are those of tests/test_gpu_outer.py and tests/test_gpu_group.py."""
import ctypes

import numpy as np
import pytest

import shapes
import test_gpu_group as g
import test_gpu_outer as t

pytestmark = pytest.mark.gpu
INT_MAX, INT_MIN = 2**31 - 1, -2**31
EMPTY = [0, INT_MAX, INT_MIN]  # {count, min, max} of an R row without a partner


def reference(R, S):
    """(|R|, 4) int64 rows {r_payload, count, min, max} in R's order: per R row the number of S rows
    with its key and the smallest and the largest of their payloads (signed); without one, count 0
    and the identities min = INT32_MAX, max = INT32_MIN."""
    R, S = np.asarray(R).reshape(-1, 2), np.asarray(S).reshape(-1, 2)
    cnt = np.zeros(R.shape[0], dtype=np.int64)
    mn, mx = np.full(R.shape[0], INT_MAX, dtype=np.int64), np.full(R.shape[0], INT_MIN, dtype=np.int64)
    if R.shape[0] and S.shape[0]:
        order = np.argsort(S[:, 0], kind="stable")
        uk, start, n = np.unique(S[order, 0], return_index=True, return_counts=True)
        pay = S[order, 1].astype(np.int64)
        lo, hi = np.minimum.reduceat(pay, start), np.maximum.reduceat(pay, start)
        i = np.minimum(np.searchsorted(uk, R[:, 0]), uk.size - 1)
        hit = uk[i] == R[:, 0]
        cnt, mn, mx = np.where(hit, n[i], 0).astype(np.int64), np.where(hit, lo[i], mn), np.where(hit, hi[i], mx)
    return np.stack([R[:, 1].astype(np.int64), cnt, mn, mx], 1)


def _sorted(rows):
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 4)
    return rows[np.argsort(rows[:, 0], kind="stable")]


def _host(rows):
    """GroupMinMaxRows -> (n, 4) int64 {r_payload, count, min, max}, checking the views against raw."""
    raw = rows.raw.cpu().numpy()
    out = np.stack([rows.r_payload.cpu().numpy().astype(np.int64), rows.count.cpu().numpy(),
                    rows.min.cpu().numpy().astype(np.int64), rows.max.cpu().numpy().astype(np.int64)], 1).reshape(-1, 4)
    assert raw.dtype == np.int32 and raw.shape == (out.shape[0], 4)
    assert rows.count.cpu().numpy().dtype == np.int64
    assert np.array_equal(out[:, [0, 2, 3]], raw[:, [0, 2, 3]].astype(np.int64))
    assert np.array_equal(out[:, 1], raw[:, 1].view(np.uint32).astype(np.int64))
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
        st, rows, pairs, _ = hw.group_minmax_join_device(dR, dS, args, kind=kind, **kw)
        rows = _sorted(_host(rows))
        print(f"kind {kind}: {rows.shape[0]} rows (host {want.shape[0]}), n_pairs {pairs} (host {int(ref[:, 1].sum())}, "
              f"counting join {cj.matches}), filtered {st.filtered} (counting join {cj.filtered})")
        assert rows.shape[0] == want.shape[0] == st.matches
        assert pairs == cj.matches == int(ref[:, 1].sum())
        assert st.filtered == cj.filtered
        assert np.array_equal(rows, want)
        _, srows, spairs, _ = hw.group_join_device(dR, dS, args, kind=kind)
        srows = g._sorted(g._host(srows))
        assert spairs == pairs and np.array_equal(srows[:, :2], rows[:, :2])  # (the sum form's counts)
        got[kind] = rows
    assert got[hw.GROUP_ALL].shape[0] == R.shape[0]
    assert np.array_equal(got[hw.GROUP_MATCHED], got[hw.GROUP_ALL][got[hw.GROUP_ALL][:, 1] > 0])
    return got


rows_of = g.rows_of


@pytest.fixture(scope="module")
def crc(orc):
    return shapes.Crc(orc.crc)


# ------------------------------------------------------------------------------ 1: every mode
@pytest.mark.parametrize("name", t.MODES)
def test_every_mode(hw, cuda, orc, name):
    R, S = t.mode_relations(orc)
    got = check(hw, cuda, R, S, t._args(hw)[name], tag="every_mode")
    assert got[hw.GROUP_MATCHED].shape[0] == int(np.isin(R[:, 0], S[:, 0]).sum()) >= 1000
    lone = got[hw.GROUP_ALL][got[hw.GROUP_ALL][:, 1] == 0]
    assert lone.shape[0] >= 1000 and (lone[:, 1:] == EMPTY).all()


# ------------------------------------------------------------- 2: signedness and identities
@pytest.mark.parametrize("name", ["blocked_packed", "basic_k1", "nobloom"])
def test_signedness_and_identities(hw, cuda, crc, name):
    """5,000 R keys three times each, with INT_MAX, INT_MIN, 0, -1 and the key whose code is the
    kernels' empty-slot value. Key i's S group is of kind (i + 1) mod 6: 0 no row (GROUP_ALL's rows
    carry the identities), 1 one row (min == max), 2 three positive payloads (a max that starts at 0
    under unsigned handling, or a min cleared to 0), 3 three negative payloads (a max cleared to 0),
    4 exactly {-1, 1} (unsigned compares give min 1, max -1), 5 INT32_MIN, INT32_MAX and one more.
    S also holds 7,000 keys R lacks. The three copies of a key carry equal rows."""
    rng = np.random.default_rng(21)
    special = np.array([INT_MAX, INT_MIN, 0, -1, int(crc.key_of(0xFFFFFFFF))], dtype=np.int64)
    rest = np.setdiff1d(rng.choice(np.arange(-10**6, 10**6), 6000, replace=False), special)[:5000 - special.size]
    keys = np.concatenate([special, rest])
    assert np.unique(keys).size == 5000
    kinds = (np.arange(keys.size) + 1) % 6
    hits = np.array([0, 1, 3, 3, 2, 3])[kinds]
    Sk = np.repeat(keys, hits)
    Sp = np.empty(Sk.size, dtype=np.int64)
    want = {}
    o = 0
    for key, kd, h in zip(keys, kinds, hits):
        if kd == 1:
            p = rng.integers(INT_MIN, INT_MAX, size=1, endpoint=True)
        elif kd == 2:
            p = rng.integers(1, INT_MAX, size=3, endpoint=True)
        elif kd == 3:
            p = rng.integers(INT_MIN, -1, size=3, endpoint=True)
        elif kd == 4:
            p = rng.permutation([-1, 1])
        else:
            p = rng.permutation([INT_MIN, INT_MAX, int(rng.integers(-1000, 1000))])[:h]
        Sp[o:o + h] = p
        o += h
        want[int(key)] = [h, int(p.min()), int(p.max())] if h else EMPTY
    assert o == Sk.size
    extra = rng.integers(2 * 10**6, 3 * 10**6, size=7000)
    S = np.stack([np.concatenate([Sk, extra]), np.concatenate([Sp, t._payloads(7000, rng)])], 1).astype(np.int32)
    S = S[rng.permutation(S.shape[0])]
    Rk = np.repeat(keys, 3)
    rng.shuffle(Rk)
    R = t._rel(Rk, rng)
    got = check(hw, cuda, R, S, t._args(hw)[name], tag="signedness")
    rows = got[hw.GROUP_ALL]
    assert got[hw.GROUP_MATCHED].shape[0] == 3 * int((hits > 0).sum())
    for key in keys[:60]:  # (the special keys and every kind of group)
        mine = rows_of(rows, R, [key])
        assert mine.shape[0] == 3 and (mine[:, 1:] == want[int(key)]).all(), (key, mine, want[int(key)])
        assert rows_of(got[hw.GROUP_MATCHED], R, [key]).shape[0] == (3 if want[int(key)][0] else 0)
    k4, k1 = keys[kinds == 4], keys[kinds == 1]
    assert (rows_of(rows, R, k4)[:, 1:] == [2, -1, 1]).all()
    one = rows_of(rows, R, k1)
    assert one.shape[0] == 3 * k1.size and (one[:, 2] == one[:, 3]).all()
    assert (rows_of(rows, R, keys[kinds == 0])[:, 1:] == EMPTY).all()
    assert (rows_of(rows, R, keys[kinds == 5])[:, 2:] == [INT_MIN, INT_MAX]).all()
    assert (rows_of(rows, R, keys[kinds == 2])[:, 2] > 0).all() and (rows_of(rows, R, keys[kinds == 3])[:, 3] < 0).all()


# -------------------------------------------------------------- 3: a hot R key across pieces
@pytest.mark.parametrize("name", ["nobloom", "blocked_packed"])
def test_hot_r_key_across_pieces(hw, cuda, crc, name):
    """The crafted job of tests/test_gpu_group.py::test_hot_r_key_across_pieces: one job holds an R key
    2 kMatPiece + 5 times, keys 11, 12, 13 and six keys no S row has (three at the head of R, three at
    its tail: the job's first and last pieces), more than kMatRCap tuples. The hot key's 40 survivors
    have the minimum -123456789 and the maximum 987654321 at different positions, the others in
    [-1000, 1000]. Every hot copy, in whichever piece, has count 40 and that min and max; the keys
    without S rows carry the identities: accumulators that are not reinitialised per piece, or that
    are cleared to zero, give other numbers."""
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
    key = lambda v: crc.key_of(shapes.job_codes(info, q0, sub0, np.atleast_1d(v)))
    at = np.flatnonzero(np.isin(S[:, 0], key(7)))
    assert at.size == 40
    S[at, 1] = rng.integers(-1000, 1000, size=40, endpoint=True)
    S[at[13], 1], S[at[31], 1] = -123456789, 987654321
    t.same_geometry(hw, cuda, R, args, info)
    got = check(hw, cuda, R, S, args)
    for kind in (hw.GROUP_MATCHED, hw.GROUP_ALL):
        mine = rows_of(got[kind], R, key(7))
        assert mine.shape[0] == hot and (mine[:, 1:] == [40, -123456789, 987654321]).all()
        assert (rows_of(got[kind], R, key([11, 12]))[:, 1] == 10).all()
    jobk = key(np.arange(3000))
    assert rows_of(got[hw.GROUP_MATCHED], R, jobk).shape[0] == hot + 2
    mine = rows_of(got[hw.GROUP_ALL], R, jobk)
    assert mine.shape[0] == hot + 9 and int((mine[:, 1] == 0).sum()) == 7
    for codes in (lc[:3], lc[3:]):  # the first and the last piece
        mine = rows_of(got[hw.GROUP_ALL], R, crc.key_of(codes))
        assert mine.shape[0] == 3 and (mine[:, 1:] == EMPTY).all()


# ---------------------------------------------------------- 4: hot S keys over many batches
@pytest.mark.parametrize("name", ["nobloom", "blocked_packed", "basic_k1"])
def test_hot_s_keys_over_many_batches(hw, cuda, crc, name):
    """Three R keys (in one job where the partition is a code digit) with 200,000, 70,000 and 100,001
    S rows: more than kMatPiece survivors over many batches on one accumulator, beside ordinary
    filler. Each group's minimum and maximum occur exactly once, at random positions; its other
    payloads lie strictly between them, in [-10^6, 10^6] with both signs. Then the same with every
    one of the three keys twice in R, which takes the hash table."""
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
    sizes = (200000, 70000, 100001)
    ends = ((INT_MIN, INT_MAX), (-1234567, 7654321), (-5000001, 5000002))
    hot_k, hot_p, want = [], [], {}
    for k, n, (lo, hi) in zip(k3, sizes, ends):
        p = rng.integers(-10**6, 10**6, size=n, endpoint=True)
        assert (p < 0).any() and (p > 0).any()
        a, b = rng.choice(n, 2, replace=False)
        p[a], p[b] = lo, hi
        hot_k.append(np.full(n, k))
        hot_p.append(p)
        want[int(k)] = [n, lo, hi]
    Sf = t._rel(fill[nR - 3000:], rng)  # 3,000 of R's filler keys, 3,000 R lacks
    S = np.concatenate([np.stack([np.concatenate(hot_k), np.concatenate(hot_p)], 1).astype(np.int32), Sf])
    S = S[rng.permutation(S.shape[0])]
    for copies in (1, 2):
        Rk = np.concatenate([np.repeat(k3, copies), fill[:nR - 3 * copies]])
        rng.shuffle(Rk)
        R = t._rel(Rk, rng)
        if info["sub_shift"] > 0:
            t.same_geometry(hw, cuda, R, args, info)
        got = check(hw, cuda, R, S, args)
        for kind in (hw.GROUP_MATCHED, hw.GROUP_ALL):
            for k, w in want.items():
                mine = rows_of(got[kind], R, [k])
                assert mine.shape[0] == copies and (mine[:, 1:] == w).all()


# ------------------------------------------------------------------- 5: empty sides of a job
def test_empty_sides_of_a_job(hw, cuda, crc):
    """The crafted partitions of tests/test_gpu_group.py::test_empty_sides_of_a_job, without a filter:
    (a) partition qa holds 100 S rows and no R: no rows; (b) partition qb holds 100 R rows and no S
    row at all (no probe items): GROUP_ALL rows {0, INT32_MAX, INT32_MIN}, no GROUP_MATCHED row; (c)
    in partition qc sub s1 holds 100 R rows and no survivors, beside sub s2 with R and S."""
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
        assert mine.shape[0] == 100 and (mine[:, 1:] == EMPTY).all()
        assert rows_of(m, R, crc.key_of(codes)).shape[0] == 0
    mine = rows_of(a, R, crc.key_of(c2_r))
    assert mine.shape[0] == 100 and int(mine[:, 1].sum()) == 80 and int((mine[:, 1] == 2).sum()) == 20
    assert (mine[mine[:, 1] == 0, 1:] == EMPTY).all() and (mine[mine[:, 1] == 1, 2] == mine[mine[:, 1] == 1, 3]).all()
    assert rows_of(m, R, crc.key_of(c2_r)).shape[0] == 60
    assert not np.isin(crc.key_of(a_s), R[:, 0]).any() and a.shape[0] == nR  # (qa: S and no R, no row)


# ------------------------------------------------------------- 6: more than kMatDesc descriptors
@pytest.mark.parametrize("name", ["nobloom", "blocked_f256"])
def test_more_descriptors_than_a_batch(hw, cuda, crc, name):
    """The shape of tests/test_gpu_group.py::test_more_descriptors_than_a_batch: a partition of
    kMatDesc * BSW * 32 + 1 R tuples (several R descriptor batches per job), 60,000 distinct keys
    repeated all over it; S has rows of 50,000 of them only, so rows with and without partners come
    from every descriptor batch."""
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
    assert (mine[mine[:, 1] == 0, 1:] == EMPTY).all()


# ----------------------------------------------------------------------------- 7: edge sizes
@pytest.mark.parametrize("name", ["blocked_packed", "nobloom", "global_b4"])
def test_edge_sizes(hw, cuda, name):
    rng = np.random.default_rng(13)
    for nR, nS in [(0, 1000), (1000, 0), (1, 1), (7, 33), (4097, 4099)]:
        R = t._rel(rng.permutation(nR) + 1, rng)
        S = t._rel(rng.integers(0, 2 * max(nR, 1) + 2, size=nS), rng)
        got = check(hw, cuda, R, S, t._args(hw)[name])
        if nR == 0 or nS == 0:
            assert got[hw.GROUP_MATCHED].shape[0] == 0 and (got[hw.GROUP_ALL][:, 1:] == EMPTY).all()


# ---------------------------------------------------------------------- 8: capacity contract
@pytest.mark.parametrize("name", ["blocked_packed", "global_b4"])
def test_capacity_contract(hw, cuda, orc, name):
    """Capacities 0, 1, n - 1 and n: rows go into a buffer with a guard region behind `capacity` rows
    that stays untouched, *n_out is the full count, the return code 7 or 0; an unaligned d_out is
    refused with 2."""
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
        return hw.lib().hwbrj_join_group_minmax_device(dR.data_ptr(), dR.shape[0], dS.data_ptr(), dS.shape[0],
                                                       ctypes.byref(a), kind, buf, cap, ctypes.byref(n), pairs, None,
                                                       st, None)

    GUARD, guard = 0x5A5A5A5A, 4096
    for kind, want in ((hw.GROUP_MATCHED, ref[ref[:, 1] > 0]), (hw.GROUP_ALL, ref)):
        n_rows = want.shape[0]
        rows = set(map(tuple, want.tolist()))
        for cap in (0, 1, n_rows - 1, n_rows):
            buf = cuda.full((cap + guard, 4), GUARD, dtype=cuda.int32, device="cuda:0")
            n, pairs, st = ctypes.c_uint64(), ctypes.c_uint64(), hw._Stats()
            rc = call(kind, buf.data_ptr(), cap, n, ctypes.byref(pairs), ctypes.byref(st))
            assert (rc, n.value, st.matches, pairs.value) == (7 if cap < n_rows else 0, n_rows, n_rows,
                                                              int(ref[:, 1].sum()))
            host = buf.cpu().numpy()
            assert (host[cap:] == GUARD).all()  # nothing past capacity
            first = host[:cap].astype(np.int64)
            first[:, 1] = host[:cap, 1].view(np.uint32)
            assert len(set(map(tuple, first.tolist()))) == cap
            assert all(tuple(r) in rows for r in first.tolist())  # the first `capacity` rows are rows
        n0 = ctypes.c_uint64()
        assert (call(kind, None, 0, n0), n0.value) == (7, n_rows)  # count only
        n1 = ctypes.c_uint64(123)
        buf = cuda.empty((n_rows + 1, 4), dtype=cuda.int32, device="cuda:0")
        assert buf.data_ptr() % 16 == 0
        assert (call(kind, buf.data_ptr() + 8, n_rows, n1), n1.value) == (2, 123)  # unaligned d_out
        assert b"aligned" in hw.lib().hwbrj_last_error()


# --------------------------------------------------------------------------- 9: neighbours
def test_neighbours(hw, cuda, orc):
    """group_join_device, outer_join_device(OUTER_R), join_materialize_device and join_device give,
    after a min/max join of the same inputs, what they gave before it (the kernels share the LDS code
    and the engine state); one more min/max join gives the first one's rows, and the table readback
    answers 13 after it. Under a blocked filter and in the global-bitmap mode."""
    rng = np.random.default_rng(101)
    R = t._rel(rng.choice(np.arange(1, 60000), 20000, replace=False), rng)
    S = t._rel(rng.integers(1, 90000, size=120000), rng)
    dR, dS = t.to_dev(cuda, R), t.to_dev(cuda, S)

    def others(a):
        _, grp, gp, _ = hw.group_join_device(dR, dS, a, kind=hw.GROUP_ALL)
        _, outer, cls, _ = hw.outer_join_device(dR, dS, a, kind=hw.OUTER_R)
        _, pairs, _ = hw.join_materialize_device(dR, dS, a)
        cj = hw.join_device(dR, dS, a)
        return (g._sorted(g._host(grp)), gp, t._u64(outer.cpu().numpy()), cls, t._u64(pairs.cpu().numpy()),
                (cj.matches, cj.filtered))

    for a in (t._args(hw)["blocked_packed"], t._args(hw)["global_b4"]):
        before = others(a)
        assert np.array_equal(before[4], t._u64(orc.join_pairs(R, S))) and before[1] == before[5][0]
        first = check(hw, cuda, R, S, a)
        with pytest.raises(hw.TablesError) as ei:
            hw.tables_info()
        assert ei.value.code == 13
        after = others(a)
        for x, y in zip(before, after):
            assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y
        again = check(hw, cuda, R, S, a)
        for kind in first:
            assert np.array_equal(first[kind], again[kind])
