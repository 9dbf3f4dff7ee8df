"""A build's Bloom filter applied to a key column on the GPU (hw.filter_keys_device,
hwbrj_build_filter_keys_device): the selection bitmap, bit for bit.

Every expectation comes from the oracle, never from the library: a filter made with orc._Bloom,
orc_bloom_init(..., 42) and orc_bloom_add_all on the valid R keys, one orc_bloom_contains per S row,
ANDed with the validity array and packed with np.packbits(bitorder="little"). Relations are
seq_catalog's sets A and B (duplicates, negative keys, INT_MIN and INT_MAX, planted keys under the NULL
rows)."""
import ctypes

import numpy as np
import pytest

import seq_catalog as sc
import test_gpu_keys_nulls as kn

pytestmark = pytest.mark.gpu

_dcol, _dmask = kn._dcol, kn._dmask
BASIC, BLOCKED, SECTORIZED = sc.BASIC, sc.BLOCKED, sc.SECTORIZED
CATALOG = ("blocked_packed", "blocked_code", "blocked_k3", "blocked_f64", "sectorized_k2", "basic_k1", "basic_f32",
           "two_segments")
# (variant, m, k, B) at which false positives are common on set B: a kernel that tests a wrong later
# bit, a wrong sector or a wrong slice cannot pass these
DENSE = (
    (BLOCKED, 1 << 16, 1, 1024), (BLOCKED, 1 << 16, 1, 2048), (BLOCKED, 1 << 18, 3, 512), (BLOCKED, 1 << 17, 2, 64),
    (BLOCKED, 1 << 17, 2, 8), (SECTORIZED, 1 << 17, 2, 1024), (SECTORIZED, 1 << 18, 4, 512), (SECTORIZED, 1 << 17, 2, 32),
    (BASIC, 1 << 16, 1, 1024),
)
TAILS = (0, 1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
SENTINEL = 0xA5
_PASS = {}


def oracle_pass(orc, Rkeys, Skeys, cfg, key=None):
    """contains(key) of the oracle's filter of Rkeys (variant, m, k, B = cfg; seed 42) for every key of
    Skeys, as a bool array; cached under `key`."""
    if key is not None and key in _PASS:
        return _PASS[key]
    L = orc.lib()
    L.orc_bloom_contains.restype = ctypes.c_int
    L.orc_bloom_contains.argtypes = [ctypes.c_void_p, ctypes.c_int32]
    Rkeys = np.ascontiguousarray(Rkeys, dtype=np.int32)
    f = orc._Bloom()
    assert L.orc_bloom_init(ctypes.byref(f), cfg[0], cfg[1], cfg[2], cfg[3], 42) == 0
    try:
        L.orc_bloom_add_all(ctypes.byref(f), Rkeys.ctypes.data, Rkeys.shape[0])
        fn, p = L.orc_bloom_contains, ctypes.addressof(f)
        keys = np.asarray(Skeys, dtype=np.int32)
        out = np.fromiter((fn(p, k) for k in keys.tolist()), dtype=np.uint8, count=keys.size).astype(bool)
    finally:
        L.orc_bloom_free(ctypes.byref(f))
    if key is not None:
        _PASS[key] = out
    return out


def packed(bits):
    """The bitmap of a bool array: Arrow layout, zero bits up to the dword boundary."""
    pad = np.zeros((bits.size + 31) // 32 * 32, bool)
    pad[:bits.size] = bits
    return np.packbits(pad, bitorder="little")


def popcount(a):
    return int(np.unpackbits(np.asarray(a, dtype=np.uint8)).sum())


def host(t):
    return t.cpu().numpy()


def expect_set(orc, name, cfg, masked_r=True):
    """(valid & pass per S row, the valid R keys) of a catalog set."""
    s = sc.relset(name)
    Rv = s.Rk[s.vR] if masked_r else s.Rk
    return s.vS & oracle_pass(orc, Rv, s.Sk, cfg, key=(name, cfg, masked_r)), Rv


class Dev:
    """A set's columns and bitmaps on the device."""
    _cache = {}

    def __init__(self, cuda, name):
        s = sc.relset(name)
        self.s = s
        self.cR, self.cS = _dcol(cuda, s.Rk), _dcol(cuda, s.Sk)
        self.mR, self.mS = _dmask(cuda, s.vR), _dmask(cuda, s.vS)

    @classmethod
    def get(cls, cuda, name):
        if name not in cls._cache:
            cls._cache[name] = cls(cuda, name)
        return cls._cache[name]


def check(hw, cuda, orc, build, cS, mS, exp, Rv, Sv, cfg):
    """The three checks of every case: the whole bitmap, an out= buffer's bytes past it, n_pass."""
    n = exp.size
    want = packed(exp)
    bm, n_pass, ms = hw.filter_keys_device(build, cS, s_valid=mS)
    got = host(bm)
    print(f"{cfg}: nS {n} expected {int(exp.sum())} n_pass {n_pass} ms {ms:.4f}")
    assert bm.dtype == cuda.uint8 and got.size == want.size == (n + 31) // 32 * 4
    assert np.array_equal(got, want), f"first differing byte {np.nonzero(got != want)[0][:4]}"
    out = cuda.full((want.size + 64,), SENTINEL, dtype=cuda.uint8, device="cuda:0")
    bm2, n2, _ = hw.filter_keys_device(build, cS, s_valid=mS, out=out)
    assert bm2.data_ptr() == out.data_ptr() and bm2.shape[0] == want.size
    o = host(out)
    assert np.array_equal(o[:want.size], want) and (o[want.size:] == SENTINEL).all()
    assert n_pass == n2 == popcount(want) == int(exp.sum())
    assert n_pass == orc.count_filtered(Rv, Sv, *cfg)
    return bm


@pytest.mark.parametrize("name", CATALOG)
def test_catalog_configurations_on_set_a(hw, cuda, orc, name):
    cfg = sc.CONFIGS[name]
    D = Dev.get(cuda, "A")
    exp, Rv = expect_set(orc, "A", cfg)
    share = exp.sum() / D.s.vS.sum()
    print(f"{name}: pass share {share:.3f}")
    assert 0 < exp.sum() < D.s.vS.sum()
    with hw.build_keys_device(D.cR, hw.BloomFilterArgs(*cfg), hw.BUILD_ROWS, r_valid=D.mR) as b:
        check(hw, cuda, orc, b, D.cS, D.mS, exp, Rv, D.s.Sk[D.s.vS], cfg)


@pytest.mark.parametrize("cfg", DENSE, ids=lambda c: "v%d_m%d_k%d_B%d" % (c[0], c[1].bit_length() - 1, c[2], c[3]))
def test_dense_configurations_on_set_b(hw, cuda, orc, cfg):
    D = Dev.get(cuda, "B")
    s = D.s
    exp, Rv = expect_set(orc, "B", cfg)
    assert Rv.size == 56033 and int(s.vS.sum()) == 239947
    fp = int((exp & ~np.isin(s.Sk, Rv)).sum())
    clear = int((s.vS & ~exp).sum())
    print(f"{cfg}: false positives {fp}, clear rows {clear}")
    assert fp >= 1000 and clear >= 1000  # (a condition on the oracle's expectation, before any GPU call)
    with hw.build_keys_device(D.cR, hw.BloomFilterArgs(*cfg), hw.BUILD_ROWS, r_valid=D.mR) as b:
        assert np.array_equal(b.export_filter(cfg[1]), orc.bloom_bitmap(Rv, *cfg)[0]), "the build's filter"
        check(hw, cuda, orc, b, D.cS, D.mS, exp, Rv, s.Sk[s.vS], cfg)


@pytest.mark.parametrize("name", ("blocked_packed", "sectorized_k2", "basic_k1"))
def test_tails(hw, cuda, orc, name):
    """Columns of exactly nS keys and bitmaps of exactly ceil(nS / 8) bytes whose bits past nS are set."""
    cfg = sc.CONFIGS[name]
    D = Dev.get(cuda, "A")
    s = D.s
    exp_all, Rv = expect_set(orc, "A", cfg)
    with hw.build_keys_device(D.cR, hw.BloomFilterArgs(*cfg), hw.BUILD_ROWS, r_valid=D.mR) as b:
        for n in TAILS:
            bits = np.ones((n + 7) // 8 * 8, bool)
            bits[:n] = s.vS[:n]
            vb = np.packbits(bits, bitorder="little")
            assert vb.size == (n + 7) // 8
            mS = cuda.empty(vb.size, dtype=cuda.uint8, device="cuda:0")
            mS.copy_(cuda.from_numpy(vb))
            cS = _dcol(cuda, s.Sk[:n])
            assert cS.shape[0] == n and mS.data_ptr() % 4 == 0
            want = packed(exp_all[:n])
            out = cuda.full((want.size + 32,), SENTINEL, dtype=cuda.uint8, device="cuda:0")
            bm, n_pass, _ = hw.filter_keys_device(b, cS, s_valid=mS, out=out)
            o = host(out)
            assert bm.shape[0] == want.size == (n + 31) // 32 * 4, n
            assert np.array_equal(o[:want.size], want), n
            assert (o[want.size:] == SENTINEL).all(), n
            assert n_pass == int(exp_all[:n].sum()), n
            bm0, n0, _ = hw.filter_keys_device(b, cS, s_valid=mS)
            assert np.array_equal(host(bm0), want) and n0 == n_pass, n


@pytest.mark.parametrize("name", ("blocked_k3", "basic_k1"))
def test_purposes_and_bitmaps(hw, cuda, orc, name):
    cfg = sc.CONFIGS[name]
    args = hw.BloomFilterArgs(*cfg)
    D = Dev.get(cuda, "A")
    s = D.s
    exp, Rv = expect_set(orc, "A", cfg)
    with hw.build_keys_device(D.cR, args, hw.BUILD_COUNT, r_valid=D.mR) as bc, \
            hw.build_keys_device(D.cR, args, hw.BUILD_ROWS, r_valid=D.mR) as br:
        a = check(hw, cuda, orc, bc, D.cS, D.mS, exp, Rv, s.Sk[s.vS], cfg)
        b = check(hw, cuda, orc, br, D.cS, D.mS, exp, Rv, s.Sk[s.vS], cfg)
        assert np.array_equal(host(a), host(b))
    # R without a bitmap: the filter of all of R's keys; S without a bitmap: every row valid
    exp_u = oracle_pass(orc, s.Rk, s.Sk, cfg, key=("A", cfg, False))
    ones = _dmask(cuda, np.ones(s.nS, bool), tail=1)
    for purpose in (hw.BUILD_COUNT, hw.BUILD_ROWS):
        with hw.build_keys_device(D.cR, args, purpose) as bu:
            x = check(hw, cuda, orc, bu, D.cS, None, exp_u, s.Rk, s.Sk, cfg)
            y, ny, _ = hw.filter_keys_device(bu, D.cS, s_valid=ones)
            assert np.array_equal(host(x), host(y)) and ny == int(exp_u.sum())
            check(hw, cuda, orc, bu, D.cS, D.mS, s.vS & exp_u, s.Rk, s.Sk[s.vS], cfg)


@pytest.mark.parametrize("name", ("blocked_packed", "sectorized_k2", "basic_k1"))
def test_in_place(hw, cuda, orc, name):
    cfg = sc.CONFIGS[name]
    D = Dev.get(cuda, "A")
    exp, _ = expect_set(orc, "A", cfg)
    with hw.build_keys_device(D.cR, hw.BloomFilterArgs(*cfg), hw.BUILD_ROWS, r_valid=D.mR) as b:
        apart, n_apart, _ = hw.filter_keys_device(b, D.cS, s_valid=D.mS)
        buf = D.mS.clone()
        assert buf.shape[0] == (D.s.nS + 31) // 32 * 4
        same, n_same, _ = hw.filter_keys_device(b, D.cS, s_valid=buf, out=buf)
        assert same.data_ptr() == buf.data_ptr()
        assert np.array_equal(host(buf), host(apart)) and np.array_equal(host(buf), packed(exp))
        assert n_same == n_apart == int(exp.sum())


@pytest.mark.parametrize("name", ("blocked_packed", "blocked_k3", "basic_k1"))
def test_composition_with_the_probes(hw, cuda, orc, name):
    """The bitmap as s_valid of the probes: the rows they return with the original bitmap."""
    cfg = sc.CONFIGS[name]
    args = hw.BloomFilterArgs(*cfg)
    D = Dev.get(cuda, "A")
    exp, _ = expect_set(orc, "A", cfg)
    with hw.build_keys_device(D.cR, args, hw.BUILD_ROWS, r_valid=D.mR) as b:
        bm, n_pass, _ = hw.filter_keys_device(b, D.cS, s_valid=D.mS)
        assert np.array_equal(host(bm), packed(exp))
        st0, p0, _ = hw.probe_keys_pairs_device(b, D.cS, s_valid=D.mS)
        st1, p1, _ = hw.probe_keys_pairs_device(b, D.cS, s_valid=bm)
        ref = sc.expect(orc, "pairs_p", "A").rows
        assert np.array_equal(sc.u64(host(p0)), ref) and np.array_equal(sc.u64(host(p1)), ref)
        assert st0.filtered == st1.filtered == n_pass
        for anti, fam in ((False, "semi_p"), (True, "anti_p")):
            s0, r0, _ = hw.semi_probe_keys_device(b, D.cS, anti, s_valid=D.mS)
            s1, r1, _ = hw.semi_probe_keys_device(b, D.cS, anti, s_valid=bm)
            ref = sc.expect(orc, fam, "A").rows
            assert np.array_equal(sc.u64(host(r0)), ref), fam
            assert np.array_equal(sc.u64(host(r1)), ref), fam
            assert s1.filtered == n_pass, fam
    with hw.build_keys_device(D.cR, args, hw.BUILD_COUNT, r_valid=D.mR) as bc:
        st = hw.probe_keys_device(bc, D.cS, s_valid=D.mS)
        assert st.filtered == n_pass and st.matches == sc.expect(orc, "count_p", "A").matches


def test_star_join(hw, cuda, orc):
    """S with two key columns, one build per column: the second filter ANDs into the first one's bitmap in
    place, and the pairs probe of build 1 under the intersection returns its pairs on the rows that
    survive both."""
    cfg1, cfg2 = sc.CONFIGS["blocked_packed"], (SECTORIZED, 1 << 17, 2, 512)
    D = Dev.get(cuda, "A")
    s = D.s
    rng = np.random.default_rng(4404)
    R2 = sc._i32(rng.integers(sc.INT_MIN, sc.INT_MAX, size=9001, endpoint=True))
    S2 = sc._i32(np.where(rng.random(s.nS) < 0.5, rng.choice(R2, size=s.nS), rng.integers(sc.INT_MIN, sc.INT_MAX, size=s.nS, endpoint=True)))
    e1, _ = expect_set(orc, "A", cfg1)
    e2 = oracle_pass(orc, R2, S2, cfg2)
    both = e1 & e2
    assert 0 < both.sum() < e1.sum() and (e2 & ~np.isin(S2, R2)).sum() >= 100
    cR2, cS2 = _dcol(cuda, R2), _dcol(cuda, S2)
    with hw.build_keys_device(D.cR, hw.BloomFilterArgs(*cfg1), hw.BUILD_ROWS, r_valid=D.mR) as b1, \
            hw.build_keys_device(cR2, hw.BloomFilterArgs(*cfg2), hw.BUILD_COUNT) as b2:
        sel = D.mS.clone()
        _, n1, _ = hw.filter_keys_device(b1, D.cS, s_valid=sel, out=sel)
        _, n2, _ = hw.filter_keys_device(b2, cS2, s_valid=sel, out=sel)
        assert (n1, n2) == (int(e1.sum()), int(both.sum()))
        assert np.array_equal(host(sel), packed(both))
        st, rows, _ = hw.probe_keys_pairs_device(b1, D.cS, s_valid=sel)
        p = sc.pairs(orc, "A", True)
        want = sc.u64(sc.rows2(p[:, 0], p[:, 1])[e2[p[:, 1]]])
        assert np.array_equal(sc.u64(host(rows)), want)
        assert st.filtered == n2


def test_engine_state_is_untouched(hw, cuda, orc):
    name = "blocked_k3"
    cfg = sc.CONFIGS[name]
    args = hw.BloomFilterArgs(*cfg)
    D, DB = Dev.get(cuda, "A"), Dev.get(cuda, "B")
    s = D.s
    exp, _ = expect_set(orc, "A", cfg)
    with hw.build_keys_device(D.cR, args, hw.BUILD_ROWS, r_valid=D.mR) as b:
        def run_filter():
            bm, n, _ = hw.filter_keys_device(b, D.cS, s_valid=D.mS)
            assert n == int(exp.sum()) and np.array_equal(host(bm), packed(exp))

        # the last synchronous one-shot join's tables and filter
        st = hw.join_keys_device(DB.cR, DB.cS, args)
        assert (st.matches, st.filtered) == sc.counts(orc, "B", name)
        info, filt = hw.tables_info(), hw.export_filter(cfg[1])
        run_filter()
        assert hw.tables_info() == info and np.array_equal(hw.export_filter(cfg[1]), filt)
        assert np.array_equal(filt, orc.bloom_bitmap(DB.s.Rk, *cfg)[0])
        # a pending async join stays pending and is collected with its own counts
        hw.join_keys_device_async(DB.cR, DB.cS, args)
        run_filter()
        done = hw.join_wait_all()
        assert len(done) == 1 and (done[0].matches, done[0].filtered) == sc.counts(orc, "B", name)
        # marks and accumulators
        cV = _dcol(cuda, s.Sv)
        hw.outer_probe_keys_device(b, D.cS, hw.PROBE_MARK_S, s_valid=D.mS)
        hw.group_accum_probe_keys_device(b, D.cS, cV, hw.AGG_SUM, s_valid=D.mS)
        un0 = sc.u64(host(b.unmatched_rows()[0]))
        g0, pairs0, _ = b.group_rows(hw.AGG_SUM, hw.GROUP_ALL)
        g0 = sc.g64(np.ascontiguousarray(host(g0.raw)).view(np.int32))
        assert un0.size > 0 and pairs0 > 0
        run_filter()
        un1 = sc.u64(host(b.unmatched_rows()[0]))
        g1, pairs1, _ = b.group_rows(hw.AGG_SUM, hw.GROUP_ALL)
        g1 = sc.g64(np.ascontiguousarray(host(g1.raw)).view(np.int32))
        assert np.array_equal(un0, un1) and np.array_equal(g0, g1) and pairs0 == pairs1


def test_refusals_and_a_callers_stream(hw, cuda, orc):
    D = Dev.get(cuda, "A")
    nbytes = (D.s.nS + 31) // 32 * 4
    with hw.build_keys_device(D.cR, None, hw.BUILD_ROWS, r_valid=D.mR) as b:  # no filter
        out = cuda.full((nbytes,), SENTINEL, dtype=cuda.uint8, device="cuda:0")
        with pytest.raises(RuntimeError, match=r"\(5\)"):
            hw.filter_keys_device(b, D.cS, s_valid=D.mS, out=out)
        assert (host(out) == SENTINEL).all()
    cfg = sc.CONFIGS["sectorized_k2"]
    exp, _ = expect_set(orc, "A", cfg)
    with hw.build_keys_device(D.cR, hw.BloomFilterArgs(*cfg), hw.BUILD_COUNT, r_valid=D.mR) as b:
        stream = cuda.cuda.Stream()
        bm, n, ms = hw.filter_keys_device(b, D.cS, stream, s_valid=D.mS)
        assert np.array_equal(host(bm), packed(exp)) and n == int(exp.sum()) and ms > 0
