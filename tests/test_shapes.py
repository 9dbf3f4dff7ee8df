"""CPU tests of tests/shapes.py: the numpy references the path tests (test_gpu_shapes.py) rely on
are themselves checked against the oracle's scalar hash, the reference KATs and tiny hand-made
tables. The `info` dicts here are toy geometries with made-up constants (not the kernels'): they
pin the rules of shapes.py, and the GPU tests feed it the library's own constants."""
import json
import os

import numpy as np
import pytest

import shapes

HERE = os.path.dirname(os.path.abspath(__file__))
KATS = json.load(open(os.path.join(HERE, "golden", "ref_kats.json")))

# a toy launch: 8 partitions of 4 subs, 18-bit packing irrelevant here
TOY = dict(F=8, NSUB=4, sub_shift=3, hash_shift=5, jobs=32, bitmap=1, jkind=0, G=4,
           j_fused=4, j_desc=6, j_waves=2, j_fs=1, j_fw=2, j_rw=1, j_sw=1, j_piece=100, j_tail_u=2,
           j_tail_s=1, m_desc=3, m_piece=50, m_rcap=80)


@pytest.fixture(scope="module")
def crc(orc):
    return shapes.Crc(orc.crc)


def test_crc_matches_reference_kats(crc):
    keys = np.array([r["key"] for r in KATS["kats"]], dtype=np.int64)
    want = np.array([r["crc32c"] for r in KATS["kats"]], dtype=np.uint32)
    assert len(keys) > 500
    assert np.array_equal(crc.code(keys.astype(np.int32)), want)
    assert np.array_equal(crc.key_of(want), keys.astype(np.int32))


def test_crc_inverse_roundtrip(crc, orc):
    rng = np.random.default_rng(1)
    x = rng.integers(-2**31, 2**31, size=100000).astype(np.int32)
    x[:4] = [0, -1, -2**31, 2**31 - 1]
    c = crc.code(x)
    assert np.array_equal(crc.key_of(c), x)
    for k in x[:200].tolist():  # and the codes are the oracle's
        assert int(crc.code(np.array([k], dtype=np.int32))[0]) == orc.crc(42, k)
    codes = rng.integers(0, 2**32, size=100000).astype(np.uint32)  # any chosen bits
    assert np.array_equal(crc.code(crc.key_of(codes)), codes)


def test_crapwow_and_basic_jobs(orc):
    """shapes.crapwow against the reference KATs; job_of_basic = the basic filter's first bit slice
    (CrapWow mod m mod F) and the mixed word's digits."""
    keys = np.array([r["key"] for r in KATS["kats"]], dtype=np.int64).astype(np.int32)
    want = np.array([r["crapwow"] for r in KATS["kats"]], dtype=np.uint32)
    assert np.array_equal(shapes.crapwow(keys), want)
    info = dict(F=32, NSUB=8, sub_shift=0, hash_shift=3)
    q, sub, v = shapes.job_of_basic(keys, info, 1 << 10)
    assert np.array_equal(q, (want & 1023) & 31)
    h = (keys.astype(np.int64).astype(np.uint32).astype(np.uint64) * 0x9E3779B1 & 0xFFFFFFFF).astype(np.uint32)
    w = h ^ (h >> np.uint32(16))
    assert np.array_equal(sub, w & 7) and np.array_equal(v, w >> np.uint32(3))
    with pytest.raises(ValueError):
        shapes.job_of(w, info)


def test_craft_lands_keys_in_their_jobs(crc, orc):
    info = dict(TOY, F=1024, NSUB=16, sub_shift=10, hash_shift=14, jobs=1 << 14, G=8)
    a = shapes.job_codes(info, 5, 3, np.arange(70))
    b = shapes.job_codes(info, 1023, 15, np.array([0, 7, 7, (1 << 18) - 1]))  # a duplicate, the extremes
    n = 4000
    rel = shapes.craft(crc, info, dict(n=n, place=[(2, a), (2, b), (7, a[:5])], avoid_q={5, 1023}))
    assert rel.shape == (n, 2) and np.array_equal(rel[:, 1], np.arange(n))
    codes = np.array([orc.crc(42, int(k)) for k in rel[:, 0]], dtype=np.uint32)  # the oracle's hash
    q, sub, v = shapes.job_of(codes, info)
    lo, hi = shapes.wg_range(n, 8, 2)
    assert (lo, hi) == (1000, 1500)
    sl = slice(lo, lo + 70)
    assert (q[sl] == 5).all() and (sub[sl] == 3).all() and np.array_equal(v[sl], np.arange(70))
    sl = slice(lo + 70, lo + 74)
    assert (q[sl] == 1023).all() and (sub[sl] == 15).all() and v[sl].tolist() == [0, 7, 7, (1 << 18) - 1]
    lo7, _ = shapes.wg_range(n, 8, 7)
    assert (q[lo7:lo7 + 5] == 5).all() and np.array_equal(v[lo7:lo7 + 5], np.arange(5))
    # the filler stays out of the partitions under test and holds no key twice
    mask = np.ones(n, dtype=bool)
    mask[lo:lo + 74] = False
    mask[lo7:lo7 + 5] = False
    assert not np.isin(q[mask], [5, 1023]).any()
    assert np.unique(rel[mask, 0]).size == mask.sum()
    # workgroup ranges tile the input in units of 4 tuples, for ragged sizes too
    for nn, G in ((0, 4), (1, 4), (9, 4), (4 * 256 + 1, 256), (12345, 7)):
        r = [shapes.wg_range(nn, G, w) for w in range(G)]
        assert r[0][0] == 0 and r[-1][1] == nn and all(r[i][1] == r[i + 1][0] for i in range(G - 1))
        assert all(lo % 4 == 0 for lo, _ in r)


@pytest.mark.parametrize("kbits", [18, 24, 32])
def test_decode_runs_against_packer(kbits):
    """Runs of every length 0..9 and longer ones, so that packed runs start at key offsets of every
    residue mod 4 (18-bit keys: bit offsets 0, 2, 4, 6 within a byte)."""
    rng = np.random.default_rng(kbits)
    hs = 14 if kbits == 18 else 8 if kbits == 24 else 9
    vmax = 1 << min(kbits, 32 - hs)
    lens = [1, 2, 3, 0, 4, 5, 66, 7, 129, 0, 8, 9]
    runs = [rng.integers(0, vmax, size=n).tolist() for n in lens]
    runs[0][0], runs[2][-1] = vmax - 1, 0
    off = np.cumsum([0] + lens[:-1])
    assert {int(o) % 4 for o in off} == {0, 1, 2, 3}
    raw = shapes.pack_runs(runs, kbits, hs, 512, low=(1 << hs) - 1)
    got = shapes.decode_runs(raw, lens, off, kbits, hs)
    assert [g.tolist() for g in got] == runs
    # the survivor side: bit 31 of the offset selects the packed format, else 32-bit codes
    flag = 0x80000000 if kbits != 32 else 0
    got = shapes.decode_runs(raw, lens, off | flag, kbits, hs, surv=True)
    assert [g.tolist() for g in got] == runs
    codes = shapes.pack_runs(runs, 32, hs, 512)
    got = shapes.decode_runs(codes, lens, off, kbits, hs, surv=True)
    assert [g.tolist() for g in got] == runs
    with pytest.raises(AssertionError):  # a run that leaves its slot
        shapes.decode_runs(raw[:4], [9], [0], kbits, hs)


def _tables(r_sweeps, s_items, nparts=None, packed=1):
    """Toy tables: r_sweeps / s_items = per partition, a list of per-sweep / per-item [NSUB] counts."""
    F, NSUB = TOY["F"], TOY["NSUB"]
    rs, rc, its, sc = [0], [], [0], []
    for q in range(F):
        rc += r_sweeps.get(q, [])
        rs.append(len(rc))
        sc += s_items.get(q, [])
        its.append(len(sc))
    sc = np.array(sc, dtype=np.uint32).reshape(-1, NSUB)
    return dict(r_sweep_start=np.array(rs), r_cnt=np.array(rc, dtype=np.uint32).reshape(-1, NSUB),
                s_item_start=np.array(its), surv_cnt=sc,
                surv_off=np.full(sc.shape, packed << 31, dtype=np.uint32),
                nparts=np.ones(F * NSUB, dtype=np.uint32) if nparts is None else nparts)


def test_classify_one_table_per_class():
    NSUB = TOY["NSUB"]
    nodup = np.zeros(TOY["jobs"], dtype=bool)
    row = lambda s0: [s0, 0, 0, 0]
    # q0: fused (2 sweeps, 1 item); q1: batched by sweeps (5 > j_fused); q2: batched by items (7 > j_desc)
    t = _tables({0: [row(3), row(4)], 1: [row(1)] * 5, 2: [row(2)], 3: [row(1)], 4: []},
                {0: [row(9)], 1: [row(1)], 2: [row(1)] * 7, 3: [], 4: [row(5)]})
    c = shapes.classify(t, TOY, nodup)
    assert c[(0, 0)]["cls"] == "fused" and c[(0, 0)]["r_keys"] == 7 and c[(0, 0)]["s_keys"] == 9
    assert c[(1 * NSUB, 0)]["cls"] == "batched" and c[(1 * NSUB, 0)]["r_batches"] == 1
    assert c[(2 * NSUB, 0)]["cls"] == "batched" and c[(2 * NSUB, 0)]["s_batches"] == 2
    assert c[(3 * NSUB, 0)]["cls"] == "empty" and c[(4 * NSUB, 0)]["cls"] == "empty"
    assert c[(0, 0)]["formats"] == {1} and not c[(0, 0)]["s_walk"]
    # a duplicate R key: the bitmap gives up, from the fused and from the batched path
    dup = nodup.copy()
    dup[[0, NSUB]] = True
    c = shapes.classify(t, TOY, dup)
    assert (c[(0, 0)]["cls"], c[(0, 0)]["start"], c[(0, 0)]["pieces"]) == ("hash", "dup_fused", [7])
    assert (c[(NSUB, 0)]["cls"], c[(NSUB, 0)]["start"]) == ("hash", "dup_batched")
    assert c[(2 * NSUB, 0)]["cls"] == "batched"
    # hash from the start (keys too wide for the bitmap, or PRH / PRHO)
    c = shapes.classify(t, dict(TOY, bitmap=0), nodup)
    assert (c[(0, 0)]["cls"], c[(0, 0)]["start"]) == ("hash", "hash")
    c = shapes.classify(t, dict(TOY, jkind=2), nodup, jobs=[0])
    assert list(c) == [(0, 0)] and c[(0, 0)]["start"] == "hash" and c[(0, 0)]["nh"] == [4]


def test_classify_pieces_batches_tails_and_parts():
    NSUB = TOY["NSUB"]
    nodup = np.zeros(TOY["jobs"], dtype=bool)
    info = dict(TOY, bitmap=0)
    row = lambda s0: [s0, 0, 0, 0]
    # pieces (j_piece 100): 60 + 40 | 70 | 150 (a long run alone) | 10, then a second R batch (j_desc 6)
    t = _tables({0: [row(60), row(40), row(70), row(150), row(10), row(1), row(98), row(2)]}, {0: [row(1)]})
    c = shapes.classify(t, info, nodup, jobs=[0])[(0, 0)]
    assert c["pieces"] == [100, 70, 150, 11, 98 + 2] and c["r_batches"] == 2
    assert shapes.hash_pieces([101], info) == [101] and shapes.hash_pieces([100, 1], info) == [100, 1]
    assert shapes.hash_pieces([0, 0], info) == [0]
    # PRH: NH = 4 up to 16 keys, doubling at 17 (NH * 4 < n)
    cc = shapes.classify(_tables({0: [row(16)], 1: [row(17)], 2: [row(65)]}, {q: [row(1)] for q in range(3)}),
                         dict(TOY, jkind=1), nodup)
    assert [cc[(q * NSUB, 0)]["nh"] for q in range(3)] == [[4], [8], [32]]
    # tails (walk: 64 j_rw = 64 first, rounds of 64 j_tail_u = 128): none, rest only, loop only, both
    T = shapes._tail
    assert T(64, 1, TOY) == (False, False) and T(65, 1, TOY) == (False, True)
    assert T(64 + 128, 1, TOY) == (True, False) and T(64 + 129, 1, TOY) == (True, True)
    assert T(64 + 127, 1, TOY) == (False, True)
    # the fused path takes 64 j_fw words first, the batched one 64 j_rw
    t = _tables({0: [row(129)], 1: [row(129)] * 5}, {0: [row(300)], 1: [row(1)]})
    c = shapes.classify(t, TOY, nodup)
    assert c[(0, 0)]["cls"] == "fused" and c[(0, 0)]["r_tail"] == (False, True)
    assert c[(0, 0)]["s_tail"] == (True, True)
    assert c[(NSUB, 0)]["cls"] == "batched" and c[(NSUB, 0)]["r_tail"] == (False, True)
    # fused with more survivor runs than the fused loads take (j_waves * j_fs = 2): the walk after them
    t = _tables({0: [row(1)]}, {0: [row(1)] * 3})
    assert shapes.classify(t, TOY, nodup)[(0, 0)]["s_walk"]
    # parts: 7 items over 3 parts, the kernel's split; a part with no item of its own is empty
    assert [shapes.part_items(10, 17, p, 3) for p in range(3)] == [(10, 12), (12, 14), (14, 17)]
    npt = np.ones(TOY["jobs"], dtype=np.uint32)
    npt[0] = 3
    t = _tables({0: [row(1)]}, {0: [row(1), row(2), row(4), row(8), row(16), row(32), row(64)]}, nparts=npt)
    c = shapes.classify(t, TOY, nodup, jobs=[0])
    assert [c[(0, p)]["s_keys"] for p in range(3)] == [3, 12, 112]
    # mixed formats: an unstaged item (bit 31 clear) among staged ones
    t["surv_off"][2, 0] = 5
    assert shapes.classify(t, TOY, nodup, jobs=[0])[(0, 1)]["formats"] == {0, 1}


def test_classify_mat_one_table_per_class():
    NSUB = TOY["NSUB"]
    nodup = np.zeros(TOY["jobs"], dtype=bool)
    row = lambda s0: [s0, 0, 0, 0]
    t = _tables({0: [row(30), row(40)], 1: [row(30)], 2: [row(81)], 3: [row(20)] * 4, 4: [row(10)], 5: [row(1)]},
                {0: [row(200)], 1: [row(10)], 2: [row(10)], 3: [row(1)], 4: [row(30), row(30)], 5: []})
    c = shapes.classify_mat(t, TOY, nodup)
    assert (c[0]["cls"], c[0]["s_batches"]) == ("bitmap", 3)  # 200 survivors, batches of m_rcap = 80
    dup = nodup.copy()
    dup[[0, NSUB]] = True
    cd = shapes.classify_mat(t, TOY, dup)
    assert (cd[NSUB]["cls"], cd[NSUB]["start"]) == ("hash1", "dup")
    assert (cd[0]["cls"], cd[0]["pieces"], cd[0]["s_batches"]) == ("general", 2, 4)  # 70 R, 200 survivors
    assert (c[2 * NSUB]["cls"], c[2 * NSUB]["pieces"]) == ("general", 2)  # 81 > m_rcap and > m_piece
    assert (c[3 * NSUB]["cls"], c[3 * NSUB]["r_batches"], c[3 * NSUB]["pieces"]) == ("general", 2, 3)
    assert c[4 * NSUB]["cls"] == "bitmap" and c[5 * NSUB]["cls"] == "empty"
    cn = shapes.classify_mat(t, dict(TOY, bitmap=0), nodup)
    assert cn[4 * NSUB]["cls"] == "general" and cn[4 * NSUB]["s_batches"] == 2  # 60 survivors > m_piece
    assert cn[NSUB]["cls"] == "hash1"
