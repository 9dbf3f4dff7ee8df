"""Group accumulators of a prepared build on the GPU (hw.group_accum_probe_keys_device,
Build.group_rows, Build.reset_group): S streamed in batches, the aggregates kept per R row in the build.

Every expectation is a host reference of the existing suite (test_gpu_keys_group_nulls.GRef on the
concatenated batches) and, where S is not empty, the one-shot group join of R and the whole S. Per batch
the counts and stats are the GROUP_MATCHED probe's on the same build and batch. Rows are compared as
sorted multisets."""
import ctypes

import numpy as np
import pytest

import test_gpu_keys_group_nulls as kgn
import test_gpu_keys_nulls as kn
import test_gpu_prepared as tp

pytestmark = pytest.mark.gpu

INT_MIN, INT_MAX = kgn.INT_MIN, kgn.INT_MAX
FORMS = ("sum", "minmax")
ONE_SHOT = {"sum": "group_join_keys_device", "minmax": "group_minmax_join_keys_device"}
PROBE = {"sum": "group_probe_keys_device", "minmax": "group_minmax_probe_keys_device"}
_dcol, _dmask, _distinct = kn._dcol, kn._dmask, kn._distinct


def agg_of(hw, form):
    return hw.AGG_SUM if form == "sum" else hw.AGG_MINMAX


def _mod(form):
    return kgn.FORMS[form][0]


def rows_of(hw, b, form, kind):
    """(sorted host rows, n_pairs) of Build.group_rows."""
    rows, pairs, _ = b.group_rows(agg_of(hw, form), kind)
    return _mod(form)._sorted(_mod(form)._host(rows)), pairs


def identity_rows(form, n):
    ident = [0, 0] if form == "sum" else [0, INT_MAX, INT_MIN]
    return np.concatenate([np.arange(n, dtype=np.int64)[:, None], np.tile(np.array(ident, dtype=np.int64), (n, 1))], 1)


def check_rows(hw, b, form, gref, one_shot=None):
    """Both kinds of Build.group_rows against GRef and, when given, one_shot(kind) -> the one-shot join's
    (stats, rows, n_pairs, ms). Returns the GROUP_ALL rows."""
    mod, out = _mod(form), None
    for kind in (hw.GROUP_ALL, hw.GROUP_MATCHED):
        want = gref.rows(form, kind == hw.GROUP_ALL)
        got, pairs = rows_of(hw, b, form, kind)
        print(f"{form} kind {kind}: {got.shape[0]} rows (host {want.shape[0]}), n_pairs {pairs} (host {gref.n_pairs()})")
        assert got.shape == want.shape and np.array_equal(got, want)
        assert pairs == gref.n_pairs()
        if kind == hw.GROUP_ALL:
            assert got.shape[0] == gref.Rk.size
            out = got
        if one_shot is not None:
            _, rows, one_pairs, _ = one_shot(kind)
            assert np.array_equal(got, mod._sorted(mod._host(rows))) and pairs == one_pairs
    return out


def accumulate(hw, b, form, cS, cV, mS=None, mV=None, compare=True):
    """One accumulating probe; its counts and stats against the GROUP_MATCHED probe of the same batch on
    the same build (which leaves the accumulators alone)."""
    st, n_rows, n_pairs, ms = hw.group_accum_probe_keys_device(b, cS, cV, agg_of(hw, form), s_valid=mS, sv_valid=mV)
    assert st.ms_r_scatter == 0 and st.ms_r_index == 0 and st.ms_build == 0 and st.ms_total > 0 and ms > 0, st
    assert st.matches == n_rows
    if compare:
        st2, rows, pairs2, _ = getattr(hw, PROBE[form])(b, cS, cV, hw.GROUP_MATCHED, s_valid=mS, sv_valid=mV)
        print(f"batch of {cS.shape[0]}: n_rows {n_rows} (probe {rows.r_payload.shape[0]}), n_pairs {n_pairs} (probe {pairs2})")
        assert n_rows == rows.r_payload.shape[0] == st2.matches and n_pairs == pairs2
        assert tp.stat_key(st) == tp.stat_key(st2)
        assert st2.ms_r_scatter == 0 and st2.ms_r_index == 0 and st2.ms_build == 0
    return n_rows, n_pairs


# ------------------------------------------------------------------------------ 1. streamed = one-shot
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["nobloom", "blocked_packed", "basic_k1", "blocked_f64"])
def test_streamed_equals_one_shot(hw, cuda, orc, name, form):
    """Set B in its five batches (20,000 rows, the rest, 33, 1 and 0): the rows after the last batch are
    the one-shot join's of R and the whole S, and GRef's."""
    D, args = tp.data_b(orc, cuda), tp.mkargs(hw, name)
    with hw.build_keys_device(D.cR, args, hw.BUILD_ROWS, r_valid=D.mR) as b:
        tot_pairs = 0
        for B in D.batches:
            n_rows, n_pairs = accumulate(hw, b, form, B.cS, B.cV, B.mS, B.mV)
            assert n_pairs == B.gref.n_pairs() and n_rows == B.gref.rows(form, False).shape[0]
            tot_pairs += n_pairs
        assert tot_pairs == D.whole.gref.n_pairs() > 0

        def one_shot(kind):
            return getattr(hw, ONE_SHOT[form])(D.cR, D.cS, D.cV, args, kind=kind, r_valid=D.mR, s_valid=D.mS, sv_valid=D.mV)

        check_rows(hw, b, form, D.whole.gref, one_shot)


# ------------------------------------------------------------------------------ crafted cases
class Case:
    """R (keys Rk, validity vR or None) and S batches [(keys, values[, value validity])] on the device,
    with GRef of R and the concatenated batches."""

    def __init__(self, cuda, Rk, vR, batches):
        self.Rk = np.asarray(Rk).astype(np.int64).astype(np.int32)
        self.vR = vR
        self.cR, self.mR = _dcol(cuda, self.Rk), (None if vR is None else _dmask(cuda, vR))
        self.host, self.dev = [], []
        for bt in batches:
            Sk, Sv = (np.asarray(x).astype(np.int64).astype(np.int32) for x in bt[:2])
            vV = np.ones(Sk.size, bool) if len(bt) < 3 else np.asarray(bt[2], bool)
            assert Sk.size == Sv.size == vV.size
            self.host.append((Sk, Sv, vV))
            self.dev.append((_dcol(cuda, Sk), _dcol(cuda, Sv), None if len(bt) < 3 else _dmask(cuda, vV)))
        self.gref = self.ref_of(range(len(batches)))

    def ref_of(self, which):
        which = list(which)
        cat = [np.concatenate([self.host[i][j] for i in which]) if which else np.empty(0, t)
               for j, t in enumerate((np.int32, np.int32, bool))]
        return kgn.GRef(self.Rk, cat[0], cat[1], self.vR, None, cat[2])

    def build(self, hw, args):
        return hw.build_keys_device(self.cR, args, hw.BUILD_ROWS, r_valid=self.mR)

    def stream(self, hw, b, form, which=None, compare=True):
        for i in range(len(self.dev)) if which is None else which:
            cS, cV, mV = self.dev[i]
            accumulate(hw, b, form, cS, cV, None, mV, compare)

    def one_shot(self, hw, cuda, args, form):
        """kind -> the one-shot join of R and the concatenated batches (None when S is empty)."""
        Sk, Sv, vV = (np.concatenate([h[j] for h in self.host]) if self.host else np.empty(0) for j in range(3))
        if Sk.size == 0:
            return None
        cS, cV, mV = _dcol(cuda, Sk), _dcol(cuda, Sv), _dmask(cuda, vV)
        return lambda kind: getattr(hw, ONE_SHOT[form])(self.cR, cS, cV, args, kind=kind, r_valid=self.mR, sv_valid=mV)

    def run(self, hw, cuda, args, forms=FORMS):
        """Stream every batch under every form on one build; {form: the GROUP_ALL rows}."""
        out = {}
        with self.build(hw, args) as b:
            for form in forms:
                self.stream(hw, b, form)
                out[form] = check_rows(hw, b, form, self.gref, self.one_shot(hw, cuda, args, form))
        return out


# ------------------------------------------------------------------------------ 2. pieces, table forms
@pytest.mark.parametrize("name", ["blocked_packed", "basic_k1"])
def test_pieces_and_both_table_forms(hw, cuda, orc, name):
    """A hot key with 2 m_piece + 5 copies (seven NULL), so its job runs the general form over three
    pieces; more distinct keys than the bitmap path's m_rcap; a key matched only in the last batch and one
    matched in every batch. The hot key appears in batches 1 and 3 only."""
    args = tp.mkargs(hw, name)
    D = tp.data_a(orc, cuda)
    hw.join_keys_pairs_device(D.cR, D.whole.cS, args)
    info = hw.tables_info()
    piece, rcap = info["m_piece"], info["m_rcap"]
    hot, last, every = 424242, -777, 31337
    copies = 2 * piece + 5
    base = _distinct(rcap + 1)
    assert not np.isin([hot, last, every], base).any()
    Rk = np.concatenate([base, np.full(copies, hot), [last, every, every]]).astype(np.int32)
    np.random.default_rng(5).shuffle(Rk)
    vR = np.ones(Rk.size, bool)
    vR[np.nonzero(Rk == hot)[0][:7]] = False
    rng = np.random.default_rng(6)
    absent = _distinct(300, 10**6)

    def batch(keys):
        keys = np.asarray(keys).astype(np.int64)
        return keys, rng.integers(INT_MIN, INT_MAX + 1, size=keys.size)

    batches = [batch(np.concatenate([absent[:100], [every, hot, hot, every], base[:900]])),
               batch(np.concatenate([[every], absent[100:200], base[500:3000]])),
               batch(np.concatenate([absent[200:], [hot, last, every, hot, hot], base[rcap - 50:]]))]
    C = Case(cuda, Rk, vR, batches)
    got = C.run(hw, cuda, args)
    # every valid copy of the hot key carries the whole stream's count and aggregate, a NULL copy the identity
    Sk = np.concatenate([h[0] for h in C.host])
    Sv = np.concatenate([h[1] for h in C.host]).astype(np.int64)
    at = np.nonzero(Rk == hot)[0]
    vals = Sv[Sk == hot]
    assert vals.size == 5
    for form, want in (("sum", [vals.size, vals.sum()]), ("minmax", [vals.size, vals.min(), vals.max()])):
        rows = got[form]
        assert np.array_equal(rows[:, 0], np.arange(Rk.size))
        assert (rows[at[vR[at]], 1:] == np.array(want)).all() and vR[at].sum() == copies - 7
        assert np.array_equal(rows[at[~vR[at]]], identity_rows(form, Rk.size)[at[~vR[at]]])


# ------------------------------------------------------------------------------ 3. exactness
def test_exactness_across_batches(hw, cuda, orc):
    """SUM: a key with three batches of 1,500 values INT32_MAX (the sum passes 2^32 between batches) and
    then 1,500 values INT32_MIN; a key whose batches sum to 0 with count 2. MINMAX: keys whose only value
    equals an identity (INT32_MAX, INT32_MIN); a key whose min arrives in batch 1 and max in batch 3."""
    args = tp.mkargs(hw, "blocked_packed")
    Rk = _distinct(700)
    big, zero, only_max, only_min, spread = Rk[3], Rk[100], Rk[200], Rk[333], Rk[699]
    noise = _distinct(50, 10**6)

    def batch(keys, vals):
        return np.concatenate([noise, keys]), np.concatenate([np.arange(noise.size), vals])

    batches = [batch(np.concatenate([np.full(1500, big), [zero, spread, only_max]]),
                     np.concatenate([np.full(1500, INT_MAX), [5, -1000, INT_MAX]])),
               batch(np.concatenate([np.full(1500, big), [zero, spread]]), np.concatenate([np.full(1500, INT_MAX), [-5, 7]])),
               batch(np.concatenate([np.full(1500, big), [spread, only_min]]),
                     np.concatenate([np.full(1500, INT_MAX), [123456, INT_MIN]])),
               batch(np.full(1500, big), np.full(1500, INT_MIN))]
    C = Case(cuda, Rk, None, batches)
    with C.build(hw, args) as b:
        C.stream(hw, b, "sum", [0, 1])
        mid, _ = rows_of(hw, b, "sum", hw.GROUP_MATCHED)
        assert mid[mid[:, 0] == 3][0].tolist() == [3, 3000, 3000 * INT_MAX] and 3000 * INT_MAX > 2**32
        C.stream(hw, b, "sum", [2, 3])
        rows = check_rows(hw, b, "sum", C.gref, C.one_shot(hw, cuda, args, "sum"))
        assert rows[3].tolist() == [3, 6000, 4500 * INT_MAX + 1500 * INT_MIN]
        assert rows[100].tolist() == [100, 2, 0]
        C.stream(hw, b, "minmax")
        rows = check_rows(hw, b, "minmax", C.gref, C.one_shot(hw, cuda, args, "minmax"))
        assert rows[200].tolist() == [200, 1, INT_MAX, INT_MAX] and rows[333].tolist() == [333, 1, INT_MIN, INT_MIN]
        assert rows[699].tolist() == [699, 3, -1000, 123456]
        assert rows[3].tolist() == [3, 6000, INT_MIN, INT_MAX]


# ------------------------------------------------------------------------------ 4. edges
def _vals(rng, n):
    return rng.integers(-10**6, 10**6, size=n)


@pytest.mark.parametrize("row", [0, 31, 32, -1])
def test_one_matched_row(hw, cuda, orc, row):
    """nR = 1,031: R row 0, 31, 32 or nR - 1 is the only matched row."""
    rng = np.random.default_rng(11)
    Rk = _distinct(1031)
    k1 = np.concatenate([_distinct(64, 10**6), [Rk[row]], _distinct(3, 2 * 10**6), [Rk[row]]])
    k2 = _distinct(8, 3 * 10**6)
    got = Case(cuda, Rk, None, [(k1, _vals(rng, k1.size)), (k2, _vals(rng, k2.size))]).run(hw, cuda, tp.mkargs(hw, "blocked_packed"))
    for form in FORMS:
        assert np.nonzero(got[form][:, 1])[0].tolist() == [row % 1031] and got[form][row % 1031, 1] == 2


def test_no_batch_null_r_null_values_and_an_empty_batch(hw, cuda, orc):
    args = tp.mkargs(hw, "blocked_code")
    rng = np.random.default_rng(12)
    Rk = _distinct(2077)
    got = Case(cuda, Rk, None, []).run(hw, cuda, args)                                             # no batch at all
    for form in FORMS:
        assert np.array_equal(got[form], identity_rows(form, Rk.size))
    got = Case(cuda, Rk, np.zeros(Rk.size, bool), [(Rk[:1000], _vals(rng, 1000))]).run(hw, cuda, args)  # every R row NULL
    for form in FORMS:
        assert np.array_equal(got[form], identity_rows(form, Rk.size))
    got = Case(cuda, Rk, None, [(Rk[:1000], _vals(rng, 1000), np.zeros(1000, bool))]).run(hw, cuda, args)  # every value NULL
    for form in FORMS:
        assert np.array_equal(got[form], identity_rows(form, Rk.size))
    C = Case(cuda, Rk, None, [(Rk[:1000], _vals(rng, 1000)), ([], []), (Rk[900:], _vals(rng, Rk.size - 900))])
    got = C.run(hw, cuda, args)                                                                    # an empty batch between
    for form in FORMS:
        assert (got[form][:, 1] == np.where((np.arange(Rk.size) >= 900) & (np.arange(Rk.size) < 1000), 2, 1)).all()


# ------------------------------------------------------------------------------ 5. lifetime, independence
def test_lifetime_and_independence(hw, cuda, orc):
    D, args = tp.data_b(orc, cuda), tp.mkargs(hw, "blocked_packed")
    s, nR = D.s, D.s.nR
    X, Y = D.batches[0], D.batches[2]

    def gref(batches):
        cat = [np.concatenate([a[B.a:B.b] for B in batches]) for a in (s.Sk, D.Sv, s.vS, D.vV)]
        return kgn.GRef(s.Rk, cat[0], cat[1], s.vR, cat[2], cat[3])

    refX, refXY = X.gref, gref([X, Y])
    assert refXY.n_pairs() > refX.n_pairs() > 0

    def acc(b, form, B):
        accumulate(hw, b, form, B.cS, B.cV, B.mS, B.mV, compare=False)

    with hw.build_keys_device(D.cR, args, hw.BUILD_ROWS, r_valid=D.mR) as b1, \
            hw.build_keys_device(D.cR, args, hw.BUILD_ROWS, r_valid=D.mR) as b2:
        bytes0 = b1.info()["bytes"]
        # a form never touched answers as after a reset, and allocates nothing
        for b in (b1, b2):
            for form in FORMS:
                assert np.array_equal(rows_of(hw, b, form, hw.GROUP_ALL)[0], identity_rows(form, nR))
                assert rows_of(hw, b, form, hw.GROUP_MATCHED)[0].shape[0] == 0
        assert b1.info()["bytes"] == bytes0
        acc(b1, "sum", X)
        assert b1.info()["bytes"] == bytes0 + 16 * nR and b2.info()["bytes"] == bytes0
        check_rows(hw, b1, "sum", refX)
        # what leaves the accumulators alone
        for form in FORMS:
            for kind in (hw.GROUP_MATCHED, hw.GROUP_ALL):
                getattr(hw, PROBE[form])(b1, Y.cS, Y.cV, kind, s_valid=Y.mS, sv_valid=Y.mV)
        un0 = b1.unmatched_rows()[0].shape[0]
        assert un0 == nR
        hw.outer_probe_keys_device(b1, X.cS, hw.PROBE_MARK_S, s_valid=X.mS)
        un1 = np.sort(b1.unmatched_rows()[0].cpu().numpy()[:, 0])
        assert 0 < un1.size < nR
        hw.join_keys_pairs_device(D.cR, D.cS, args, r_valid=D.mR, s_valid=D.mS)
        hw.join_keys_device_async(D.cR, D.cS, args)                      # un-waited
        check_rows(hw, b1, "sum", refX)
        hw.group_probe_keys_device(b1, Y.cS, Y.cV, s_valid=Y.mS, sv_valid=Y.mV)  # (collects the async join)
        hw.lib().hwbrj_release()
        acc(b1, "sum", Y)
        first = check_rows(hw, b1, "sum", refXY)
        assert np.array_equal(check_rows(hw, b1, "sum", refXY), first)   # group_rows again: the same rows
        # an accumulating probe leaves the marks alone
        assert np.array_equal(np.sort(b1.unmatched_rows()[0].cpu().numpy()[:, 0]), un1)
        # the two forms are independent
        assert rows_of(hw, b1, "minmax", hw.GROUP_MATCHED)[0].shape[0] == 0
        acc(b1, "minmax", X)
        assert b1.info()["bytes"] == bytes0 + 32 * nR
        check_rows(hw, b1, "minmax", refX)
        check_rows(hw, b1, "sum", refXY)
        # and so are two builds of the same R
        for form in FORMS:
            assert rows_of(hw, b2, form, hw.GROUP_MATCHED)[0].shape[0] == 0
        acc(b2, "sum", Y)
        check_rows(hw, b2, "sum", Y.gref)
        check_rows(hw, b1, "sum", refXY)
        assert b2.unmatched_rows()[0].shape[0] == nR
        # reset: the identities again, the other form untouched, and the same batches give the same rows
        b1.reset_group(hw.AGG_SUM)
        assert np.array_equal(rows_of(hw, b1, "sum", hw.GROUP_ALL)[0], identity_rows("sum", nR))
        got, pairs = rows_of(hw, b1, "sum", hw.GROUP_MATCHED)
        assert got.shape[0] == 0 and pairs == 0
        check_rows(hw, b1, "minmax", refX)
        acc(b1, "sum", X)
        acc(b1, "sum", Y)
        assert np.array_equal(check_rows(hw, b1, "sum", refXY), first)
        with pytest.raises(RuntimeError, match=r"\(2\)"):
            hw.group_accum_probe_keys_device(b1, X.cS, X.cV, 2, s_valid=X.mS, sv_valid=X.mV)
        with pytest.raises(RuntimeError, match=r"\(2\)"):
            b1.group_rows(hw.AGG_SUM, 2)
        check_rows(hw, b1, "sum", refXY)
    with hw.build_keys_device(D.cR, args, hw.BUILD_COUNT, r_valid=D.mR) as bc:
        with pytest.raises(RuntimeError, match=r"\(2\)"):
            hw.group_accum_probe_keys_device(bc, X.cS, X.cV)
        with pytest.raises(RuntimeError, match=r"\(2\)"):
            bc.group_rows()
        with pytest.raises(RuntimeError, match=r"\(2\)"):
            bc.reset_group(hw.AGG_SUM)


# ------------------------------------------------------------------------------ 6. capacity
@pytest.mark.parametrize("form", FORMS)
def test_capacity_and_guard_regions(hw, cuda, orc, form):
    """hwbrj_build_group_rows_device itself at capacity 0 (no output), n - 1 and n, on a buffer of n + 16
    rows of sentinels: the full count always, 7 below it, exactly `capacity` rows written, each a row of
    the result, nothing behind them."""
    D, args = tp.data_a(orc, cuda), tp.mkargs(hw, "blocked_packed")
    B, L, agg = D.whole, hw.lib(), agg_of(hw, form)
    with hw.build_keys_device(D.cR, args, hw.BUILD_ROWS, r_valid=D.mR) as b:
        accumulate(hw, b, form, B.cS, B.cV, B.mS, B.mV)
        h = b._handle()
        for kind in (hw.GROUP_MATCHED, hw.GROUP_ALL):
            want = B.gref.rows(form, kind == hw.GROUP_ALL)
            rows, want_pairs, _ = b.group_rows(agg, kind)
            assert np.array_equal(_mod(form)._sorted(_mod(form)._host(rows)), want)
            valid = {r.tobytes() for r in rows.raw.cpu().numpy().view(np.int32).reshape(-1, 4)}
            n = want.shape[0]
            assert 1 < n == len(valid)
            for cap, null_out in ((0, True), (0, False), (n - 1, False), (n, False)):
                buf = cuda.full((n + 16, 4), tp.SENTINEL, dtype=cuda.int32, device="cuda:0")
                n_out, pairs = ctypes.c_uint64(0xDEAD), ctypes.c_uint64(0xDEAD)
                rc = L.hwbrj_build_group_rows_device(h, agg, kind, None if null_out else hw._ptr(buf), cap, ctypes.byref(n_out),
                                                     ctypes.byref(pairs), None, None)
                cuda.cuda.synchronize()
                got = buf.cpu().numpy()
                print(f"{form} kind {kind} capacity {cap} of {n}: rc {rc}, n_out {n_out.value}, n_pairs {pairs.value}")
                assert rc == (7 if cap < n else 0) and n_out.value == n and pairs.value == want_pairs
                assert (got[cap:] == tp.SENTINEL).all()
                head = [r.tobytes() for r in got[:cap]]
                assert len(set(head)) == cap and valid.issuperset(head)
        n_out = ctypes.c_uint64(0xDEAD)
        assert L.hwbrj_build_group_rows_device(h, agg, 2, None, 0, ctypes.byref(n_out), None, None, None) == 2
        assert n_out.value == 0xDEAD
        buf = cuda.full((8, 4), tp.SENTINEL, dtype=cuda.int32, device="cuda:0")
        assert L.hwbrj_build_group_rows_device(h, agg, hw.GROUP_ALL, hw._ptr(buf) + 8, 4, ctypes.byref(n_out), None, None,
                                               None) == 2 and n_out.value == 0xDEAD


# ------------------------------------------------------------------------------ 7. the 2^32 rule
@pytest.mark.parametrize("form", FORMS)
def test_the_running_total_stays_below_2_pow_32(hw, cuda, orc, form):
    """After a batch of 40 rows the same pointers with nS = 2^32 - 40 are refused with 3 before any device
    call, and nothing changes. (The accepted neighbour 2^32 - 41 is not issued: it would read past the
    buffers.)"""
    Rk = _distinct(300)
    Sk = np.concatenate([Rk[:30], _distinct(10, 10**6)])
    C = Case(cuda, Rk, None, [(Sk, np.arange(40) - 20)])
    L, agg = hw.lib(), agg_of(hw, form)
    cS, cV, _ = C.dev[0]
    with C.build(hw, tp.mkargs(hw, "blocked_packed")) as b:
        C.stream(hw, b, form)
        before = check_rows(hw, b, form, C.gref)
        n, pairs = ctypes.c_uint64(0xDEAD), ctypes.c_uint64(0xDEAD)
        st = hw._Stats()
        ctypes.memset(ctypes.byref(st), 0x5A, ctypes.sizeof(st))
        rc = L.hwbrj_probe_keys_group_accum_device(b._handle(), hw._ptr(cS), None, hw._ptr(cV), None, 2**32 - 40, agg,
                                                   ctypes.byref(n), ctypes.byref(pairs), None, ctypes.byref(st), None)
        msg = L.hwbrj_last_error().decode()
        print(rc, msg)
        assert rc == 3 and "40 S rows accumulated" in msg and "2^32" in msg
        assert (n.value, pairs.value) == (0xDEAD, 0xDEAD) and bytes(st) == b"\x5a" * ctypes.sizeof(hw._Stats)
        assert np.array_equal(check_rows(hw, b, form, C.gref), before)
        # the other form has its own total
        other = "minmax" if form == "sum" else "sum"
        C.stream(hw, b, other, compare=False)
        b.reset_group(agg)
        C.stream(hw, b, form, compare=False)
        assert np.array_equal(check_rows(hw, b, form, C.gref), before)
