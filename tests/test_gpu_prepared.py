"""Prepared builds on the GPU (hw.build_keys_device and the *_probe_keys_device functions): build R
once, probe it with S batches.

Every expectation is the host reference of the existing key-column tests on the same inputs
(test_gpu_keys_nulls.NRef: orc.join_pairs, orc.bpro and np.isin on the valid rows;
test_gpu_keys_group_nulls.GRef for the group joins) and, for the stats, the one-shot entry's own
result on the same R and the same batch. Rows are compared as sorted multisets. The one-shot
functions and the probes go through the same two check functions (kn.check, kgn.check): the probes
behind an object that answers hw's one-shot names from a pair of builds (ProbeAs)."""
import ctypes

import numpy as np
import pytest

import seq_catalog as sc
import test_gpu_keys_group_nulls as kgn
import test_gpu_keys_nulls as kn
import test_gpu_shapes as gs
from test_gpu_shapes import crc  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

CONFIGS = ("nobloom", "blocked_packed", "blocked_code", "blocked_k3", "blocked_f64", "sectorized_k2", "basic_k1",
           "basic_f32")
STAT_FIELDS = ("filtered", "matches", "mode", "format", "partitions", "subparts", "join_keys", "join_key_bits")
SENTINEL = 0x7B7B7B7B
_dcol, _dmask = kn._dcol, kn._dmask


def mkargs(hw, name):
    c = sc.CONFIGS[name]
    return None if c is None else hw.BloomFilterArgs(*c)


def stat_key(st):
    return tuple(getattr(st, f) for f in STAT_FIELDS)


class Rec:
    """An hw-like object whose join functions also log (function, kind / anti / algorithm, stats
    fields, what the call returned beside its rows), call by call."""

    def __init__(self, target):
        self._t, self.log = target, []

    def __getattr__(self, name):
        v = getattr(self._t, name)
        if not callable(v) or not name.endswith("_device"):
            return v

        def call(*a, **kw):
            r = v(*a, **kw)
            st, rest = (r, ()) if not isinstance(r, tuple) else (r[0], r[1:])
            extras = tuple(x for x in rest[1:] if isinstance(x, (int, tuple)))  # n_class, n_pairs (not ms)
            n = len(rest[0][0]) if rest and isinstance(rest[0], tuple) else (rest[0].shape[0] if rest else None)
            self.log.append((name, kw.get("kind"), kw.get("anti"), kw.get("algorithm"), stat_key(st), n, extras))
            return r
        return call


class ProbeAs:
    """hw's one-shot key-column functions answered by probes: cR, args and r_valid are ignored (they
    are the builds': bc for the counting probe, br for the probes that return rows). Every probe's
    stats must show no R phase."""

    def __init__(self, hw, bc, br):
        self._hw, self.bc, self.br = hw, bc, br

    def __getattr__(self, name):
        return getattr(self._hw, name)

    @staticmethod
    def _no_r_phase(st):
        assert st.ms_r_scatter == 0 and st.ms_r_index == 0 and st.ms_build == 0 and st.ms_total > 0, st
        return st

    def join_keys_device(self, cR, cS, args=None, stream=None, algorithm=0, *, r_valid=None, s_valid=None):
        return self._no_r_phase(self._hw.probe_keys_device(self.bc, cS, stream, algorithm, s_valid=s_valid))

    def join_keys_pairs_device(self, cR, cS, args=None, stream=None, capacity=None, *, r_valid=None, s_valid=None):
        r = self._hw.probe_keys_pairs_device(self.br, cS, stream, capacity, s_valid=s_valid)
        self._no_r_phase(r[0])
        return r

    def semi_join_keys_device(self, cR, cS, args=None, anti=False, stream=None, capacity=None, *, r_valid=None,
                              s_valid=None):
        r = self._hw.semi_probe_keys_device(self.br, cS, anti, stream, capacity, s_valid=s_valid)
        self._no_r_phase(r[0])
        return r

    def outer_join_keys_device(self, cR, cS, args=None, kind=0, stream=None, capacity=None, *, r_valid=None,
                               s_valid=None):
        r = self._hw.outer_probe_keys_device(self.br, cS, kind, stream, capacity, s_valid=s_valid)
        self._no_r_phase(r[0])
        return r

    def group_join_keys_device(self, cR, cS, cV, args=None, kind=0, stream=None, capacity=None, *, r_valid=None,
                               s_valid=None, sv_valid=None):
        r = self._hw.group_probe_keys_device(self.br, cS, cV, kind, stream, capacity, s_valid=s_valid, sv_valid=sv_valid)
        self._no_r_phase(r[0])
        return r

    def group_minmax_join_keys_device(self, cR, cS, cV, args=None, kind=0, stream=None, capacity=None, *, r_valid=None,
                                      s_valid=None, sv_valid=None):
        r = self._hw.group_minmax_probe_keys_device(self.br, cS, cV, kind, stream, capacity, s_valid=s_valid,
                                                    sv_valid=sv_valid)
        self._no_r_phase(r[0])
        return r


# ------------------------------------------------------------------------------ the relations
class Batch:
    """Rows [a, b) of a set's S: its columns and bitmaps on the device (views of the whole columns where
    a is a multiple of 32, else allocations of exactly the batch's size) and its host references."""

    def __init__(self, orc, cuda, D, a, b, view):
        s = D.s
        self.a, self.b, self.n = a, b, b - a
        self.vS, self.vV = s.vS[a:b], D.vV[a:b]
        if view:
            assert a % 32 == 0
            self.cS, self.cV = D.cS[a:b], D.cV[a:b]
            self.mS, self.mV = D.mS[a // 8:], D.mV[a // 8:]  # (the bits past the batch are later rows': ignored)
        else:
            self.cS, self.cV = _dcol(cuda, s.Sk[a:b]), _dcol(cuda, D.Sv[a:b])
            self.mS, self.mV = _dmask(cuda, self.vS, tail=1), _dmask(cuda, self.vV, tail=1)
        self.ref = kn.NRef(orc, s.Rk, s.Sk[a:b], s.vR, self.vS)
        self.gref = kgn.GRef(s.Rk, s.Sk[a:b], D.Sv[a:b], s.vR, self.vS, self.vV)
        self._counts = {}

    def counts(self, orc, name, args):
        """(filtered, matches) of the key joins (S rows with a valid key) from orc.bpro, or None where a
        side is empty."""
        if name not in self._counts:
            self._counts[name] = self.ref.counts(orc, args)
        return self._counts[name]


class Data:
    """One relation set of seq_catalog on the device, a value bitmap that differs from the key bitmap
    (values poisoned underneath), and S's batches."""

    def __init__(self, orc, cuda, name, cuts=None):
        s = self.s = sc.relset(name)
        rng = np.random.default_rng(77 + s.nS)
        self.vV = rng.random(s.nS) >= 0.2
        self.Sv = kgn._poison(s.Sv, self.vV)
        self.cR, self.mR = _dcol(cuda, s.Rk), _dmask(cuda, s.vR)
        self.cS, self.cV = _dcol(cuda, s.Sk), _dcol(cuda, self.Sv)
        self.mS, self.mV = _dmask(cuda, s.vS), _dmask(cuda, self.vV)
        self.whole = Batch(orc, cuda, self, 0, s.nS, True)
        self.batches = [Batch(orc, cuda, self, a, b, view) for a, b, view in (cuts or [])]


_DATA = {}


def data_b(orc, cuda):
    """Set B (R 70,001, S 300,007, a fifth NULL on each side and in the value column). S in batches that
    partition it: 20,000 rows and the rest as views cut at multiples of 32 rows, then 33 rows, 1 row and
    0 rows in allocations of their own."""
    if "B" not in _DATA:
        nS = sc.SETS["B"][1]
        cuts = [(0, 20000, True), (20000, nS - 34, True), (nS - 34, nS - 1, False), (nS - 1, nS, False), (nS, nS, False)]
        _DATA["B"] = Data(orc, cuda, "B", cuts)
        assert [b.n for b in _DATA["B"].batches] == [20000, nS - 20034, 33, 1, 0]
    return _DATA["B"]


def data_a(orc, cuda):
    if "A" not in _DATA:
        _DATA["A"] = Data(orc, cuda, "A")
    return _DATA["A"]


def builds(hw, D, args, count=True):
    bc = hw.build_keys_device(D.cR, args, hw.BUILD_COUNT, r_valid=D.mR) if count else None
    return bc, hw.build_keys_device(D.cR, args, hw.BUILD_ROWS, r_valid=D.mR)


def check_batch(hw, orc, D, B, name, args, bc, br, algos=True):
    """Every join kind on batch B: the one-shot functions and the probes against the host references,
    then the probes' stats and counts against the one-shot calls'."""
    one, prb = Rec(hw), Rec(ProbeAs(hw, bc, br))
    counts = B.counts(orc, name, args)
    gcounts = B.gref.counts(orc, args)
    for h in (one, prb):
        kn.check(h, B.ref, D.cR, B.cS, D.mR, B.mS, args, counts)
        kgn.check(h, B.gref, (D.cR, B.cS, B.cV), (D.mR, B.mS, B.mV), args, gcounts)
        for algo in (hw.ALGO_PRH, hw.ALGO_PRHO) if algos else ():
            st = h.join_keys_device(D.cR, B.cS, args, algorithm=algo, r_valid=D.mR, s_valid=B.mS)
            assert st.matches == B.ref.pairs.shape[0]
    assert len(one.log) == len(prb.log) == 1 + 1 + 2 + 3 + 4 + (2 if algos else 0)
    for a, b in zip(one.log, prb.log):
        assert a == b, (name, B.a, B.b, a, b)


# ------------------------------------------------------------------------------ 1. probe = one-shot
@pytest.mark.parametrize("name", CONFIGS)
def test_probe_equals_one_shot(hw, cuda, orc, name):
    """One build per purpose; every probe kind on every batch (count under the three algorithms, pairs,
    semi, anti, the three outer kinds, both group forms under both kinds)."""
    D, args = data_b(orc, cuda), mkargs(hw, name)
    bc, br = builds(hw, D, args)
    with bc, br:
        assert bc.info()["purpose"] == hw.BUILD_COUNT and br.info()["purpose"] == hw.BUILD_ROWS
        assert br.info()["nR"] == D.s.nR and br.info()["masked"] == 1
        for B in D.batches:
            check_batch(hw, orc, D, B, name, args, bc, br)
        # after a probe: the tables are the build's, and so is the filter
        hw.probe_keys_pairs_device(br, D.batches[2].cS, s_valid=D.batches[2].mS)
        with pytest.raises(hw.TablesError, match=r"\(13\)"):
            hw.tables_info()
        if args is not None:
            with pytest.raises(RuntimeError, match=r"\(5\)"):
                hw.export_filter(args.m)


def test_both_join_paths_occur_among_the_configurations(hw, cuda, orc):
    """HWBRJ_TI_BITMAP after the one-shot pairs join of the same R: the bitmap path and the hash table."""
    D = data_b(orc, cuda)
    seen = set()
    for name in CONFIGS:
        hw.join_keys_pairs_device(D.cR, D.batches[2].cS, mkargs(hw, name), r_valid=D.mR, s_valid=D.batches[2].mS)
        seen.add(hw.tables_info()["bitmap"])
    assert seen == {0, 1}


# ------------------------------------------------------------------------------ 2. R is read once
def test_r_is_read_once(hw, cuda, orc):
    D, name = data_b(orc, cuda), "blocked_packed"
    args = mkargs(hw, name)
    cR, mR = D.cR.clone(), D.mR.clone()
    cuda.cuda.synchronize()
    hw.join_keys_device(cR, D.whole.cS, args, r_valid=mR, s_valid=D.whole.mS)
    want_filter = hw.export_filter(args.m)
    bc = hw.build_keys_device(cR, args, hw.BUILD_COUNT, r_valid=mR)
    br = hw.build_keys_device(cR, args, hw.BUILD_ROWS, r_valid=mR)
    cR.fill_(12345)   # other keys, and every R row valid
    mR.fill_(0xFF)
    cuda.cuda.synchronize()
    with bc, br:
        B = D.batches[1]  # the largest
        prb = ProbeAs(hw, bc, br)
        kn.check(prb, B.ref, None, B.cS, None, B.mS, args, B.counts(orc, name, args))
        kgn.check(prb, B.gref, (None, B.cS, B.cV), (None, B.mS, B.mV), args, B.gref.counts(orc, args))
        assert np.array_equal(br.export_filter(args.m), want_filter)
        assert np.array_equal(bc.export_filter(args.m), want_filter)
        assert want_filter.any()


# ------------------------------------------------------------------------------ 3. builds survive
def _c_pairs(hw, b, B, cap, out=None):
    """(return code, *n_out) of hwbrj_probe_keys_pairs_device itself (the wrapper runs again at the exact
    size on 7)."""
    n = ctypes.c_uint64()
    rc = hw.lib().hwbrj_probe_keys_pairs_device(b._handle(), hw._ptr(B.cS), hw._vptr(B.mS), B.n,
                                                hw._ptr(out) if out is not None else None, cap, ctypes.byref(n), None,
                                                None, None)
    return rc, n.value


def test_builds_survive_everything_else(hw, cuda, orc):
    """Two builds of different R under different configurations, their probes alternated with one-shot
    joins of a larger set under another configuration, an un-waited async join, a capacity overflow,
    hwbrj_release and a probe on another stream; a one-shot join of each family right after a probe."""
    DA, DB = data_a(orc, cuda), data_b(orc, cuda)
    if "C" not in _DATA:
        s = sc.relset("C")
        _DATA["C"] = (s, _dcol(cuda, s.Rk), _dcol(cuda, s.Sk), gs.to_dev(cuda, s.R), gs.to_dev(cuda, s.S))
    sC, cRC, cSC, tRC, tSC = _DATA["C"]
    nameA, nameB, nameC = "blocked_code", "basic_k1", "sectorized_k2"
    aA, aB, aC = mkargs(hw, nameA), mkargs(hw, nameB), mkargs(hw, nameC)
    BA, BB = DA.whole, DB.batches[0]
    bcA, brA = builds(hw, DA, aA)
    bcB, brB = builds(hw, DB, aB)
    pA, pB = ProbeAs(hw, bcA, brA), ProbeAs(hw, bcB, brB)
    want_c = sc.counts(orc, "C", nameC)[0]

    def probe_a(what):
        kn.check(pA, BA.ref, None, BA.cS, None, BA.mS, aA, BA.counts(orc, nameA, aA), what=what)

    def probe_b(what):
        kn.check(pB, BB.ref, None, BB.cS, None, BB.mS, aB, BB.counts(orc, nameB, aB), what=what)

    with bcA, brA, bcB, brB:
        probe_a(("count", "pairs"))
        assert hw.join_keys_device(cRC, cSC, aC).matches == want_c      # a larger one-shot join, another config
        probe_b(("count", "anti"))
        st, pairs, _ = hw.join_keys_pairs_device(cRC, cSC, aC)
        assert st.matches == pairs.shape[0] == want_c
        probe_a(("outer",))
        hw.join_device_async(tRC, tSC, aC)                               # un-waited
        probe_b(("pairs", "semi"))
        kgn.check(pA, BA.gref, (None, BA.cS, BA.cV), (None, BA.mS, BA.mV), aA, BA.gref.counts(orc, aA))
        small = cuda.empty((4, 2), dtype=cuda.int32, device="cuda:0")
        assert _c_pairs(hw, brB, BB, 4, small) == (7, BB.ref.pairs.shape[0]) and BB.ref.pairs.shape[0] > 4  # overflow
        probe_a(("count", "pairs", "semi", "anti"))
        hw.lib().hwbrj_release()
        probe_b(("count", "pairs", "outer"))
        probe_a(("anti", "outer"))
        other = cuda.cuda.Stream(device="cuda:0")
        cuda.cuda.synchronize()
        st, rows, _ = hw.probe_keys_pairs_device(brB, BB.cS, stream=other, s_valid=BB.mS)
        assert np.array_equal(kn._u64(rows.cpu().numpy()), BB.ref.upairs)
        st = hw.probe_keys_device(bcA, BA.cS, stream=other, s_valid=BA.mS)
        assert (st.filtered, st.matches) == BA.counts(orc, nameA, aA)
        # a one-shot join of each family right after a probe (the job table, the slot's words 5 to 7, smark)
        for what in (("count",), ("pairs",), ("semi",), ("anti",), ("outer",)):
            probe_a(("outer",) if what != ("outer",) else ("anti",))
            kn.check(hw, BA.ref, DA.cR, BA.cS, DA.mR, BA.mS, aC, what=what)
        for form in ("sum", "minmax"):
            probe_b(("outer",))
            kgn.check(hw, BA.gref, (DA.cR, BA.cS, BA.cV), (DA.mR, BA.mS, BA.mV), aC, forms=(form,))
        probe_b(("count",))
        assert hw.join_keys_device(cRC, cSC, None).matches == want_c
        probe_a(("count", "pairs"))


# ------------------------------------------------------------------------------ 4. packing
def test_packing_is_fixed_at_build_time(hw, cuda, orc, crc):  # noqa: F811
    """The crafted relation of test_gpu_shapes whose full probe items overflow the stage: a counting build
    made while packing is on answers such a batch through both key formats; a build made right after
    such a join has 32-bit keys, and both keep their format however the hint moves."""
    R, S, X = gs.rel_a(hw, cuda, crc, True)
    args = gs.mk(hw, gs.BLK)
    want = gs.ref_counts(orc, hw, R, S, gs.BLK)
    cR, cS = _dcol(cuda, R[:, 0]), _dcol(cuda, S[:, 0])
    small = lambda: hw.join_device(gs.to_dev(cuda, R[:64]), gs.to_dev(cuda, S[:64]), args)  # noqa: E731
    assert small().unstaged_items == 0                                   # packing on
    with hw.build_keys_device(cR, args, hw.BUILD_COUNT) as b18:
        assert b18.info()["join_key_bits"] == 18
        st = hw.probe_keys_device(b18, cS)
        assert st.join_keys == hw.JOIN_KEYS_MIXED and st.unstaged_items >= 2 and st.join_key_bits == 18
        assert (st.filtered, st.matches) == want
        with hw.build_keys_device(cR, args, hw.BUILD_COUNT) as b32:      # right after a join with unstaged items
            assert b32.info()["join_key_bits"] == 32
            st = hw.probe_keys_device(b32, cS)
            assert st.join_keys == hw.JOIN_KEYS_32 and st.join_key_bits == 32 and (st.filtered, st.matches) == want
            assert small().unstaged_items == 0                           # the hint moves back: packing on
            one = hw.join_keys_device(cR, cS, args)
            assert one.join_key_bits == 18 and (one.filtered, one.matches) == want
            assert small().unstaged_items == 0
            st = hw.probe_keys_device(b32, cS)
            assert st.join_keys == hw.JOIN_KEYS_32 and st.join_key_bits == 32 and (st.filtered, st.matches) == want
            assert b32.info()["join_key_bits"] == 32
            st = hw.probe_keys_device(b18, cS)                            # (the hint is off again after b32's probe)
            assert st.join_keys == hw.JOIN_KEYS_MIXED and st.join_key_bits == 18 and (st.filtered, st.matches) == want


# ------------------------------------------------------------------------------ 5. capacity, guards
def _guarded(hw, cuda, call, want, caps=None):
    """call(d_out or None, capacity, n_out) at capacities 0, 1, n - 1 and n on a buffer of n + 16 rows of
    sentinels: the full count always, 7 below it, nothing past the capacity written, and what is
    written is part of (at capacity n: all of) the expected multiset `want` (sorted uint64)."""
    n = want.size
    for cap in caps if caps is not None else sorted({0, 1, max(n - 1, 0), n}):
        buf = cuda.full((n + 16, 2), SENTINEL, dtype=cuda.int32, device="cuda:0")
        n_out = ctypes.c_uint64(0xDEAD)
        rc = call(hw._ptr(buf), cap, n_out)
        cuda.cuda.synchronize()
        got = buf.cpu().numpy()
        print(f"capacity {cap} of {n}: rc {rc}, n_out {n_out.value}")
        assert n_out.value == n
        assert rc == (7 if cap < n else 0)
        assert (got[cap:] == SENTINEL).all()
        head = kn._u64(got[:cap])
        if cap == n:
            assert np.array_equal(head, want)
        else:
            assert np.isin(head, want).all()


def test_capacity_and_guard_regions(hw, cuda, orc):
    D = data_a(orc, cuda)
    B, args = D.whole, mkargs(hw, "blocked_packed")
    ref = B.ref
    L = hw.lib()
    S = (hw._ptr(B.cS), hw._vptr(B.mS), B.n)
    with hw.build_keys_device(D.cR, args, hw.BUILD_ROWS, r_valid=D.mR) as b:
        h = b._handle()
        _guarded(hw, cuda, lambda o, c, n: L.hwbrj_probe_keys_pairs_device(h, *S, o, c, ctypes.byref(n), None, None, None),
                 ref.upairs)
        anti = kn._u64(kn._rows(ref.Sk[ref.anti], ref.anti))
        _guarded(hw, cuda, lambda o, c, n: L.hwbrj_probe_keys_semi_device(h, *S, hw.JOIN_ANTI, o, c, ctypes.byref(n), None,
                                                                          None, None), anti)
        outer_s = kn._u64(np.concatenate([ref.pairs, kn._rows(np.full(ref.anti.size, -1), ref.anti)]))
        _guarded(hw, cuda, lambda o, c, n: L.hwbrj_probe_keys_outer_device(h, *S, hw.PROBE_MARK_S, o, c, ctypes.byref(n),
                                                                           None, None, None, None), outer_s)
        # (every capacity's probe marked the same R rows, the count-only one too)
        r_only = kn._u64(kn._rows(ref.r_only, np.full(ref.r_only.size, -1)))
        assert 0 < r_only.size < D.s.nR
        _guarded(hw, cuda, lambda o, c, n: L.hwbrj_build_unmatched_device(h, o, c, ctypes.byref(n), None, None), r_only)
        # the count-only forms: capacity 0 without an output
        n = ctypes.c_uint64()
        assert L.hwbrj_build_unmatched_device(h, None, 0, ctypes.byref(n), None, None) == 7 and n.value == r_only.size
        assert L.hwbrj_probe_keys_pairs_device(h, *S, None, 0, ctypes.byref(n), None, None, None) == 7
        assert n.value == ref.upairs.size


# ------------------------------------------------------------------------------ 6. marks
def _stream(hw, b, batches, kind):
    """The batches' rows under a marking kind, S rows offset by the batch's start, and the class sums."""
    rows, cls = [], np.zeros(3, dtype=np.int64)
    for B in batches:
        st, r, c, _ = hw.outer_probe_keys_device(b, B.cS, kind, s_valid=B.mS)
        r = r.cpu().numpy().copy()
        assert c[2] == 0 and st.matches == r.shape[0] == sum(c)
        r[r[:, 1] >= 0, 1] += B.a
        rows.append(r)
        cls += np.array(c)
    return np.concatenate(rows), cls


@pytest.mark.parametrize("name", ["nobloom", "blocked_packed", "basic_k1", "blocked_f64"])
def test_streamed_outer_joins(hw, cuda, orc, name):
    """A PROBE_MARK_S probe per batch, then the unmatched rows: the one-shot OUTER_FULL join of R and the
    whole S. PROBE_MARK_INNER likewise against OUTER_R. Both against the host reference too."""
    D, args = data_b(orc, cuda), mkargs(hw, name)
    W = D.whole.ref
    s_rows, r_rows = kn._rows(np.full(W.anti.size, -1), W.anti), kn._rows(W.r_only, np.full(W.r_only.size, -1))
    with hw.build_keys_device(D.cR, args, hw.BUILD_ROWS, r_valid=D.mR) as b:
        for kind, one_kind, parts in ((hw.PROBE_MARK_S, hw.OUTER_FULL, [W.pairs, s_rows, r_rows]),
                                      (hw.PROBE_MARK_INNER, hw.OUTER_R, [W.pairs, r_rows])):
            b.reset_marks()
            rows, cls = _stream(hw, b, D.batches, kind)
            un, _ = b.unmatched_rows()
            un = un.cpu().numpy()
            assert (un[:, 1] == -1).all()
            got = kn._u64(np.concatenate([rows, un]))
            cls[2] = un.shape[0]
            st, one, one_cls, _ = hw.outer_join_keys_device(D.cR, D.cS, args, kind=one_kind, r_valid=D.mR, s_valid=D.mS)
            print(f"{name} kind {kind}: classes {tuple(cls)} (one-shot {one_cls})")
            assert tuple(int(x) for x in cls) == one_cls
            assert np.array_equal(got, kn._u64(one.cpu().numpy()))
            assert np.array_equal(got, kn._u64(np.concatenate(parts)))
            # the marks stay as they are: the same rows again
            assert np.array_equal(np.sort(b.unmatched_rows()[0].cpu().numpy()[:, 0]), np.sort(un[:, 0]))


def _marks_case(hw, cuda, orc, Rk, vR, s_batches, args, kind=None):
    """Stream s_batches (key arrays, all valid) over a build of (Rk, vR) under a marking kind; every
    batch's rows against NRef, the unmatched rows against numpy. Returns the build (marks set)."""
    kind = hw.PROBE_MARK_S if kind is None else kind
    Rk = np.asarray(Rk).astype(np.int64).astype(np.int32)
    cR, mR = _dcol(cuda, Rk), (None if vR is None else _dmask(cuda, vR))
    v = np.ones(Rk.size, bool) if vR is None else vR
    b = hw.build_keys_device(cR, args, hw.BUILD_ROWS, r_valid=mR)
    matched = np.zeros(Rk.size, bool)
    for Sk in s_batches:
        Sk = np.asarray(Sk).astype(np.int64).astype(np.int32)
        ref = kn.NRef(orc, Rk, Sk, v)
        st, r, c, _ = hw.outer_probe_keys_device(b, _dcol(cuda, Sk), kind)
        want = [ref.pairs] + ([kn._rows(np.full(ref.anti.size, -1), ref.anti)] if kind == hw.PROBE_MARK_S else [])
        assert np.array_equal(kn._u64(r.cpu().numpy()), kn._u64(np.concatenate(want)))
        assert c == (ref.pairs.shape[0], ref.anti.size if kind == hw.PROBE_MARK_S else 0, 0)
        matched |= v & np.isin(Rk, Sk)
    un = b.unmatched_rows()[0].cpu().numpy()
    assert (un[:, 1] == -1).all()
    assert np.array_equal(np.sort(un[:, 0]), np.nonzero(~matched)[0])
    return b, matched


@pytest.mark.parametrize("name", ["blocked_packed", "basic_k1"])
def test_marks_over_pieces_and_batches(hw, cuda, orc, name):
    """One key with more copies than a piece of the join's hash table (every copy gets its mark, the job
    spans several pieces), a key matched only in the last batch, a key matched in every batch (the OR is
    idempotent), NULL R rows with live keys underneath."""
    args = mkargs(hw, name)
    D = data_a(orc, cuda)
    hw.join_keys_pairs_device(D.cR, D.whole.cS, args)
    piece = hw.tables_info()["m_piece"]
    dup, last, every = 424242, -777, 31337
    Rk = np.concatenate([kn._distinct(5000), np.full(piece + 100, dup), [last, every, every]]).astype(np.int32)
    np.random.default_rng(5).shuffle(Rk)
    vR = np.ones(Rk.size, bool)
    vR[np.nonzero(Rk == dup)[0][:7]] = False      # NULL copies of the hot key: never marked
    vR[np.nonzero(Rk == every)[0][0]] = False
    absent = kn._distinct(300, 10**6)
    batches = [np.concatenate([absent[:100], [every, every], kn._distinct(40, 100)]),
               np.concatenate([[every, dup, dup, dup], absent[100:200]]),
               np.concatenate([absent[200:], [last, every], kn._distinct(10, 4000)])]
    for kind in (hw.PROBE_MARK_S, hw.PROBE_MARK_INNER):
        b, matched = _marks_case(hw, cuda, orc, Rk, vR, batches, args, kind)
        with b:
            assert matched[Rk == dup].sum() == piece + 100 - 7 and matched.sum() == piece + 100 - 7 + 2 + 50
            b.reset_marks()
            un = b.unmatched_rows()[0].cpu().numpy()
            assert np.array_equal(np.sort(un[:, 0]), np.arange(Rk.size))   # every R row again


@pytest.mark.parametrize("row", [0, 31, 32, -1])
def test_one_marked_row_at_the_word_edges(hw, cuda, orc, row):
    """nR = 1,031 (no multiple of 32): R row 0, 31, 32 or nR - 1 is the only matched row."""
    Rk = kn._distinct(1031)
    batch = np.concatenate([kn._distinct(64, 10**6), [Rk[row]], kn._distinct(3, 2 * 10**6)])
    b, matched = _marks_case(hw, cuda, orc, Rk, None, [batch, kn._distinct(8, 3 * 10**6)], mkargs(hw, "blocked_packed"))
    with b:
        assert matched.sum() == 1 and matched[row]


def test_all_none_and_null_r(hw, cuda, orc):
    args = mkargs(hw, "blocked_code")
    Rk = kn._distinct(2077)
    b, matched = _marks_case(hw, cuda, orc, Rk, None, [Rk[:1000], Rk[900:]], args)            # all R matched
    with b:
        assert matched.all() and b.unmatched_rows()[0].shape[0] == 0
    b, matched = _marks_case(hw, cuda, orc, Rk, None, [kn._distinct(500, 10**6)], args)        # none
    with b:
        assert not matched.any()
    b, matched = _marks_case(hw, cuda, orc, Rk, np.zeros(Rk.size, bool), [Rk[:1000]], args)    # every R row NULL
    with b:
        assert not matched.any()
    b, matched = _marks_case(hw, cuda, orc, Rk, None, [], args)                                 # no batch at all
    with b:
        assert not matched.any()


def test_marks_belong_to_one_build(hw, cuda, orc):
    D, args = data_a(orc, cuda), mkargs(hw, "sectorized_k2")
    B = D.whole
    with hw.build_keys_device(D.cR, args, hw.BUILD_ROWS, r_valid=D.mR) as b1, \
            hw.build_keys_device(D.cR, args, hw.BUILD_ROWS, r_valid=D.mR) as b2:
        hw.outer_probe_keys_device(b1, B.cS, hw.PROBE_MARK_INNER, s_valid=B.mS)
        assert np.array_equal(np.sort(b1.unmatched_rows()[0].cpu().numpy()[:, 0]), B.ref.r_only)
        assert b2.unmatched_rows()[0].shape[0] == D.s.nR
        # the one-shot kinds on a build leave its marks alone
        hw.outer_probe_keys_device(b2, B.cS, hw.OUTER_FULL, s_valid=B.mS)
        assert b2.unmatched_rows()[0].shape[0] == D.s.nR
        with pytest.raises(RuntimeError, match=r"\(2\)"):
            hw.outer_probe_keys_device(b2, B.cS, 5, s_valid=B.mS)


# ------------------------------------------------------------------------------ 7. lifetime
def test_free_then_a_build_of_another_size(hw, cuda, orc):
    DA, DB = data_a(orc, cuda), data_b(orc, cuda)
    name = "blocked_k3"
    args = mkargs(hw, name)
    bc, br = builds(hw, DB, args)
    B = DB.batches[0]
    check_batch(hw, orc, DB, B, name, args, bc, br, algos=False)
    ic, ir = bc.info(), br.info()
    print(f"bytes: count build {ic['bytes']}, rows build {ir['bytes']}")
    assert 0 < ic["bytes"] < ir["bytes"]
    bc.free()
    br.free()
    bc.free()  # (a second free does nothing)
    with pytest.raises(ValueError, match="freed"):
        hw.probe_keys_device(bc, B.cS)
    bc, br = builds(hw, DA, args)
    with bc, br:
        assert br.info()["nR"] == DA.s.nR and br.info()["bytes"] > 0
        check_batch(hw, orc, DA, DA.whole, name, args, bc, br, algos=False)
    # purposes are checked: 2 before any device call
    with hw.build_keys_device(DA.cR, None, hw.BUILD_COUNT) as c, hw.build_keys_device(DA.cR, None) as r:
        with pytest.raises(RuntimeError, match=r"\(2\)"):
            hw.probe_keys_device(r, DA.whole.cS)
        with pytest.raises(RuntimeError, match=r"\(2\)"):
            hw.probe_keys_pairs_device(c, DA.whole.cS)
        with pytest.raises(RuntimeError, match=r"\(2\)"):
            c.unmatched_rows()
        with pytest.raises(RuntimeError, match=r"\(5\)"):
            r.export_filter(1 << 24)
