"""The side passes of the global-bitmap mode (basic k = 0 or B < 8): a counting join, then an
open-addressing table of R in HBM and one stream of S against it, for every payload join (pairs,
semi / anti, the outer joins, the group joins), through the tuple entries and the key-column entries.

Every case runs under global_b4 and asserts stats.mode == 3. References are plain numpy on the host
inputs; row multisets are compared exactly as sorted uint64 views of the rows. A key-column entry
sees the same keys with row indices as payloads (and S's payloads as the value column of a group
join). The shapes follow from the side-pass launch constants, named in each test's docstring: the
probes, the R-table pass and the group kernels launch 2048 workgroups of 256 threads, a workgroup of
a probe or of the R-table pass takes a contiguous n / 2048 slice, and the LDS row stage holds 4096
rows."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INT_MIN, INT_MAX = -2**31, 2**31 - 1
NULL = INT_MIN  # the tuple entries' null payload (the key-column entries write -1)
GUARD = 0x5A5A5A5A
MODE_GLOBAL = 3


@pytest.fixture(scope="module")
def args(hw):
    return hw.BloomFilterArgs(hw.BLOCKED, 1 << 20, 1, 4)  # global_b4


def _i32(a):
    return np.ascontiguousarray(np.asarray(a).astype(np.int64).astype(np.int32))


def _rows(*cols):
    return np.ascontiguousarray(np.stack([_i32(c).ravel() for c in cols], 1))


def _dev(cuda, a):
    return cuda.from_numpy(_i32(a)).to("cuda:0")


def _u64(rows):
    """Sorted uint64 view of (n, 2) int32 rows."""
    return np.sort(_i32(rows).reshape(-1, 2).view(np.uint64).ravel())


class Rel:
    """R and S as keys and payloads, on the host and (built once) on the device in both layouts."""

    def __init__(self, cuda, Rk, Rp, Sk, Sp):
        self.Rk, self.Rp, self.Sk, self.Sp = _i32(Rk), _i32(Rp), _i32(Sk), _i32(Sp)
        self.dR, self.dS = _dev(cuda, _rows(Rk, Rp)), _dev(cuda, _rows(Sk, Sp))
        self.cR, self.cS, self.cV = _dev(cuda, Rk), _dev(cuda, Sk), _dev(cuda, Sp)

    def payloads(self, keys):
        """(R payloads, S payloads, null) as an entry sees them."""
        if keys:
            return np.arange(self.Rk.size), np.arange(self.Sk.size), -1
        return self.Rp, self.Sp, NULL


def join_classes(Rk, Rp, Sk, Sp, null):
    """(inner, s_only, r_only) rows {R.payload, S.payload} of the join on the keys."""
    order = np.argsort(Rk, kind="stable")
    sk = Rk[order]
    lo, hi = np.searchsorted(sk, Sk, "left"), np.searchsorted(sk, Sk, "right")
    cnt = hi - lo
    s_idx = np.repeat(np.arange(Sk.size), cnt)
    r_pos = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(lo, cnt)
    inner = _rows(np.asarray(Rp)[order[r_pos]], np.asarray(Sp)[s_idx])
    s_only = _rows(np.full(int((cnt == 0).sum()), null), np.asarray(Sp)[cnt == 0])
    r_un = ~np.isin(Rk, Sk)
    r_only = _rows(np.asarray(Rp)[r_un], np.full(int(r_un.sum()), null))
    return inner, s_only, r_only


def group_rows(Rk, Rp, Sk, Sv, minmax):
    """One (r_payload, count, a, b) int32 row per R row: a, b = the int64 sum's low and high words,
    or min and max (the identities INT_MAX, INT_MIN for an empty group); and the pair total."""
    order = np.argsort(Sk, kind="stable")
    sk, sv = Sk[order], Sv[order].astype(np.int64)
    uk, start, c = np.unique(sk, return_index=True, return_counts=True)
    pos = np.minimum(np.searchsorted(uk, Rk), uk.size - 1)  # (S is not empty)
    hit = uk[pos] == Rk
    count = np.where(hit, c[pos], 0)
    if minmax:
        a = np.where(hit, np.minimum.reduceat(sv, start)[pos], INT_MAX)
        b = np.where(hit, np.maximum.reduceat(sv, start)[pos], INT_MIN)
    else:
        s = np.where(hit, np.add.reduceat(sv, start)[pos], 0).astype(np.int64)
        a, b = s & 0xFFFFFFFF, s >> 32
    return _rows(Rp, count, a, b), int(count.sum())


class Call:
    """One C entry with everything but (d_out, capacity) bound: run(buf, cap) ->
    (rc, n, stats, n_class or None, n_pairs or None)."""

    def __init__(self, hw, args, rel, kind_of, keys, kind=None):
        self.hw, self.a, self.rel, self.kind_of, self.keys, self.kind = hw, args._c(), rel, kind_of, keys, kind

    def run(self, buf, cap):
        hw, rel, L, a = self.hw, self.rel, self.hw.lib(), ctypes.byref(self.a)
        n, st = ctypes.c_uint64(), hw._Stats()
        cls, pairs = (ctypes.c_uint64 * 3)(), ctypes.c_uint64()
        R, S = (rel.cR, rel.cS) if self.keys else (rel.dR, rel.dS)
        head = (R.data_ptr(), R.shape[0], S.data_ptr(), S.shape[0], a)
        tail = (buf, cap, ctypes.byref(n))
        end = (None, ctypes.byref(st), None)
        k = self.kind_of
        if k == "pairs":
            fn = L.hwbrj_join_keys_pairs_device if self.keys else L.hwbrj_join_materialize_device
            rc = fn(*head, *tail, *end)
        elif k == "semi":
            fn = L.hwbrj_join_keys_semi_device if self.keys else L.hwbrj_join_semi_device
            rc = fn(*head, self.kind, *tail, *end)
        elif k == "outer":
            if self.keys:
                rc = L.hwbrj_join_keys_outer_device(*head, self.kind, *tail, cls, *end)
            else:
                rc = L.hwbrj_join_outer_device(*head, self.kind, NULL, *tail, cls, *end)
        else:
            name = "group_minmax" if k == "minmax" else "group"
            if self.keys:
                fn = getattr(L, f"hwbrj_join_keys_{name}_device")
                rc = fn(R.data_ptr(), R.shape[0], S.data_ptr(), rel.cV.data_ptr(), S.shape[0], a, self.kind, *tail,
                        ctypes.byref(pairs), *end)
            else:
                rc = getattr(L, f"hwbrj_join_{name}_device")(*head, self.kind, *tail, ctypes.byref(pairs), *end)
        assert st.mode == MODE_GLOBAL or rc not in (0, 7)
        return (rc, n.value, st, tuple(cls) if k == "outer" else None,
                pairs.value if k in ("group", "minmax") else None)


def run_exact(cuda, call, width=2):
    """All rows of a call (a count-only call, then one at the exact size):
    (host rows, n_class, n_pairs)."""
    rc, n, st, _, _ = call.run(None, 0)
    assert rc in (0, 7) and st.mode == MODE_GLOBAL
    buf = cuda.full((n + 16, width), GUARD, dtype=cuda.int32, device="cuda:0")
    rc, n2, st, cls, pairs = call.run(buf.data_ptr(), n)
    assert (rc, n2, st.matches, st.mode) == (0, n, n, MODE_GLOBAL)
    host = buf.cpu().numpy()
    assert (host[n:] == GUARD).all()
    return host[:n], cls, pairs


# --------------------------------------------------------------------- 1: the capacity contract
_CAP = {}


def _cap_case(cuda):
    """R: 10,000 distinct keys and 2,000 rows repeating some of them; S: 100,000 rows, half of them
    with one of the first 6,000 R keys, half with keys R lacks."""
    if not _CAP:
        rng = np.random.default_rng(101)
        keys = rng.choice(np.arange(-10**6, 10**6), 10000, replace=False)
        Rk = np.concatenate([keys, rng.choice(keys, 2000)])
        Sk = np.concatenate([rng.choice(keys[:6000], 50000), rng.integers(2 * 10**6, 3 * 10**6, size=50000)])
        rng.shuffle(Rk)
        rng.shuffle(Sk)
        Rp = rng.integers(INT_MIN + 1, INT_MAX, size=Rk.size)  # (no payload is NULL)
        Sp = rng.integers(INT_MIN + 1, INT_MAX, size=Sk.size)
        _CAP["rel"] = Rel(cuda, Rk, Rp, Sk, Sp)
    return _CAP["rel"]


def _cap_expected(hw, rel, kind_of, kind, keys):
    """(rows, n_class or None, n_pairs or None) of a case; rows (n, 2) or (n, 4) int32."""
    Rp, Sp, null = rel.payloads(keys)
    if kind_of in ("group", "minmax"):
        rows, pairs = group_rows(rel.Rk, Rp, rel.Sk, rel.Sp, kind_of == "minmax")
        if kind == hw.GROUP_MATCHED:
            rows = rows[rows[:, 1] != 0]
        return rows, None, pairs
    if kind_of == "semi":
        mask = np.isin(rel.Sk, rel.Rk)
        keep = ~mask if kind == hw.JOIN_ANTI else mask
        return _rows(rel.Sk[keep], np.asarray(Sp)[keep]), None, None
    inner, s_only, r_only = join_classes(rel.Rk, Rp, rel.Sk, Sp, null)
    if kind_of == "pairs":
        return inner, None, None
    keep_s, keep_r = kind != hw.OUTER_R, kind != hw.OUTER_S
    rows = np.concatenate([inner] + ([s_only] if keep_s else []) + ([r_only] if keep_r else []))
    return rows, (inner.shape[0], s_only.shape[0] if keep_s else 0, r_only.shape[0] if keep_r else 0), None


_CAP_CASES = [("pairs", None), ("semi", "JOIN_SEMI"), ("semi", "JOIN_ANTI"), ("outer", "OUTER_S"), ("outer", "OUTER_R"),
              ("outer", "OUTER_FULL"), ("group", "GROUP_MATCHED"), ("group", "GROUP_ALL"),
              ("minmax", "GROUP_MATCHED"), ("minmax", "GROUP_ALL")]


@pytest.mark.parametrize("keys", [False, True], ids=["tuples", "keys"])
@pytest.mark.parametrize("kind_of,kind_name", _CAP_CASES, ids=[f"{k}-{n}" for k, n in _CAP_CASES])
def test_capacity_contract_global(hw, cuda, args, kind_of, kind_name, keys):
    """capacity = 1000 below every class's row count, a 4096-row guard behind it (a whole LDS stage
    of 4096 rows flushed past the capacity would land there): code 7, the full counts in *n_out,
    stats.matches and n_class / n_pairs, the guard untouched, every row in [0, capacity) a row of
    the result (pairs included: the first `capacity` pairs are written); and the count-only form
    (capacity 0, d_out NULL) with the same count."""
    rel = _cap_case(cuda)
    inner, s_only, r_only = join_classes(rel.Rk, rel.Rp, rel.Sk, rel.Sp, NULL)
    matched = int(np.isin(rel.Rk, rel.Sk).sum())
    assert min(inner.shape[0], s_only.shape[0], r_only.shape[0], matched) > 1000
    kind = getattr(hw, kind_name) if kind_name else None
    want, want_cls, want_pairs = _cap_expected(hw, rel, kind_of, kind, keys)
    width = want.shape[1]
    assert want.shape[0] > 1000
    call = Call(hw, args, rel, kind_of, keys, kind)
    cap, guard = 1000, 4096
    buf = cuda.full((cap + guard, width), GUARD, dtype=cuda.int32, device="cuda:0")
    rc, n, st, cls, pairs = call.run(buf.data_ptr(), cap)
    print(f"{kind_of} {kind_name} keys={keys}: rc {rc}, n {n} (host {want.shape[0]}), n_class {cls} (host "
          f"{want_cls}), n_pairs {pairs} (host {want_pairs})")
    assert (rc, n, st.mode) == (7, want.shape[0], MODE_GLOBAL)
    assert cls == want_cls and pairs == want_pairs
    host = buf.cpu().numpy()
    assert (host[cap:] == GUARD).all()  # nothing past the capacity
    rows = set(r.tobytes() for r in want)
    assert st.matches == want.shape[0]
    assert all(r.tobytes() in rows for r in host[:cap])  # the first `capacity` rows are rows
    rc, n0, _, cls0, pairs0 = call.run(None, 0)  # count only
    assert (rc, n0, cls0, pairs0) == (7, want.shape[0], want_cls, want_pairs)


# ------------------------------------------------------------------- 2: a burst beyond the stage
_BURST = {}


def _burst_case(cuda):
    if not _BURST:
        rng = np.random.default_rng(202)
        other = rng.choice(np.arange(100, 10**6), 3000, replace=False)
        Rk = np.concatenate([np.full(512, 7), other])
        rng.shuffle(Rk)
        nS, run0, run = 1 << 16, 1000, 4096
        Sk = np.where(rng.random(nS) < 0.3, rng.choice(other[:2000], nS), rng.integers(2 * 10**6, 3 * 10**6, size=nS))
        Sk[run0:run0 + run] = 7
        assert int((Sk == 7).sum()) == run
        Rp = rng.integers(INT_MIN + 1, INT_MAX, size=Rk.size)
        Sp = rng.integers(INT_MIN + 1, INT_MAX, size=nS)
        rel = Rel(cuda, Rk, Rp, Sk, Sp)
        want = {}
        for keys in (False, True):
            rp, sp, null = rel.payloads(keys)
            inner, s_only, r_only = join_classes(rel.Rk, rp, rel.Sk, sp, null)
            assert inner.shape[0] > 512 * run and s_only.shape[0] > 1000 and r_only.shape[0] >= 1000
            want[keys] = {"pairs": (_u64(inner), None),
                          "outer": (_u64(np.concatenate([inner, s_only, r_only])),
                                    (inner.shape[0], s_only.shape[0], r_only.shape[0]))}
        _BURST.update(rel=rel, want=want)
    return _BURST


@pytest.mark.parametrize("keys", [False, True], ids=["tuples", "keys"])
@pytest.mark.parametrize("kind_of", ["pairs", "outer"])
def test_burst_beyond_stage(hw, cuda, args, kind_of, keys):
    """R holds key 7 in 512 rows (and 3,000 other keys, 1,000 of them absent from S); S has 2^16 rows
    with one contiguous run of 4096 rows of key 7 from row 1000. A probe workgroup's slice is
    2^16 / 2048 = 32 rows, so inside the run one round stages 32 * 512 = 16,384 pairs, more than the
    stage's 4096: the one-atomic-per-row overflow branch runs in about 128 workgroups. Pairs and
    OUTER_FULL: exact multisets (about 2.1 M rows) and exact n_class."""
    c = _burst_case(cuda)
    want, want_cls = c["want"][keys][kind_of]
    call = Call(hw, args, c["rel"], kind_of, keys, hw.OUTER_FULL if kind_of == "outer" else None)
    got, cls, _ = run_exact(cuda, call)
    print(f"{kind_of} keys={keys}: {got.shape[0]} rows (host {want.size}), n_class {cls} (host {want_cls})")
    assert got.shape[0] == want.size and cls == want_cls
    assert np.array_equal(_u64(got), want)


# --------------------------------------------------------------- 3: the stage flushes mid-loop
def _semi_flush(hw, cuda, args, anti):
    """S has 3 * 2^22 rows, 6144 per probe workgroup (24 rounds of 256); its first half has keys of
    R (50,000 keys) everywhere, its second half nowhere."""
    rng = np.random.default_rng(303)
    keys = rng.choice(np.arange(-10**6, 10**6), 50000, replace=False)
    nS = 3 << 22
    half = nS // 2
    Sk = np.concatenate([keys[rng.integers(0, keys.size, size=half)],
                         rng.integers(2 * 10**6, 3 * 10**6, size=half)])
    S = _rows(Sk, rng.integers(INT_MIN, INT_MAX, size=nS, endpoint=True))
    dR = _dev(cuda, _rows(keys, rng.integers(INT_MIN, INT_MAX, size=keys.size)))
    st, rows, _ = hw.semi_join_device(dR, _dev(cuda, S), args, anti=anti)
    want = S[half:] if anti else S[:half]
    assert (st.mode, st.matches, rows.shape[0]) == (MODE_GLOBAL, half, half)
    assert np.array_equal(_u64(rows.cpu().numpy()), _u64(want))


def _rtab_flush(hw, cuda, args):
    """R = 2^23 distinct keys in permuted order, S = 1000 rows, half of them matching."""
    rng = np.random.default_rng(404)
    nR = 1 << 23
    Rk = rng.permutation(nR) - (nR // 2)
    Rp = rng.integers(INT_MIN + 1, INT_MAX, size=nR)
    Sk = np.concatenate([rng.choice(Rk, 500), rng.integers(nR, 2 * nR, size=500)])
    rng.shuffle(Sk)
    Sp = rng.integers(INT_MIN + 1, INT_MAX, size=Sk.size)
    inner, _, r_only = join_classes(_i32(Rk), Rp, _i32(Sk), Sp, NULL)
    assert inner.shape[0] == 500 and r_only.shape[0] > nR - 501
    st, rows, cls, _ = hw.outer_join_device(_dev(cuda, _rows(Rk, Rp)), _dev(cuda, _rows(Sk, Sp)), args,
                                            kind=hw.OUTER_R, null_payload=NULL)
    assert st.mode == MODE_GLOBAL and cls == (inner.shape[0], 0, r_only.shape[0])
    assert rows.shape[0] == inner.shape[0] + r_only.shape[0]
    assert np.array_equal(_u64(rows.cpu().numpy()), _u64(np.concatenate([inner, r_only])))


@pytest.mark.parametrize("case", ["semi", "anti", "outer_r"])
def test_stage_flushes_mid_loop(hw, cuda, args, case):
    """semi, anti: S has 6144 rows per probe workgroup; a workgroup of the first (everywhere
    matching) half of S stages more than 4096 SEMI rows, so it flushes inside its loop, and a
    workgroup of the second (nowhere matching) half does the same for ANTI. Exact multisets.
    outer_r: the outer join's R-table pass over T = 2^24 slots at load 0.5: a workgroup's 8192-slot
    slice holds about 4096 entries, nearly all R-only, so the stage reaches its flush threshold
    inside the loop. OUTER_R: exact multiset and n_class."""
    if case == "outer_r":
        _rtab_flush(hw, cuda, args)
    else:
        _semi_flush(hw, cuda, args, case == "anti")
