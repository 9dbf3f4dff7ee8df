"""Every data-dependent path of the join (join_job, k_join_mat) and of the pass-1 scatter, reached
with crafted keys and checked stage by stage from the tables the join leaves in HBM
(hwbrj_tables_info / hwbrj_tables_read, include/hwbrj.h).

Every case asserts, exactly: the counts against orc.bpro; the pass-1 element starts against the
numpy histogram of the keys' partitions; the multiset of job keys in every job's R runs; the
survivor counts (every job under PRO; the crafted jobs under a filter, against orc.count_filtered)
and the crafted jobs' decoded survivors; and, for the join cells, that shapes.classify names the
intended branch for the intended job. A cell whose branch is not observed fails.

Shapes come from the library's own constants (hwbrj_tables_info): nothing here writes down a
kernel constant. Helpers live in tests/shapes.py (CPU-tested in tests/test_shapes.py).

Cells: J1 fused bitmap and run-length edges, J2 / J3 batched bitmap (by sweeps / by
items), J4 / J5 duplicate fallback, J6 hash pieces and R descriptor batches, J7 hash from the start
(24-bit keys, 32-bit words), J8 PRH / PRHO, J9 key formats, J10 parts, M the materializing join,
S1-S5 the scatter.
"""
import numpy as np
import pytest

import shapes

pytestmark = pytest.mark.gpu

BLK = ("blocked", 1 << 24, 1, 1024)     # F = 1024, 16 subs, 18-bit keys, packed S words
BLK512 = ("blocked", 1 << 19, 1, 1024)  # F = 512 (m / B), code words
BLK24 = ("blocked", 1 << 24, 1, 1 << 17)  # F = 128: 24-bit keys, hash table from the start
BASIC1 = ("basic", 1 << 10, 1, 0)       # F = 32, the partition is no code digit: 32-bit words
GEOM = ("mode", "format", "F", "NSUB", "sub_shift", "hash_shift", "nseg", "bitmap", "G", "CH", "BSW", "slot")


def to_dev(cuda, a):
    return cuda.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def mk(hw, cfg):
    if cfg is None:
        return None
    v = {"basic": hw.BASIC, "blocked": hw.BLOCKED, "sectorized": hw.SECTORIZED}[cfg[0]]
    return hw.BloomFilterArgs(v, cfg[1], cfg[2], cfg[3] or 1024)


@pytest.fixture(scope="module")
def crc(orc):
    return shapes.Crc(orc.crc)


_GEOM = {}


def geometry(hw, cuda, cfg, nR, mat=False):
    """The launch shape of a join of |R| = nR under cfg, from a join of throw-away keys of that size
    (plan_geometry's sub-partition count can depend on |R|); the real run must report the same."""
    key = (cfg, nR, mat)
    if key not in _GEOM:
        R = np.stack([np.arange(nR, dtype=np.int32), np.zeros(nR, dtype=np.int32)], 1)
        S = R[:8]
        if mat:
            hw.join_materialize_device(to_dev(cuda, R), to_dev(cuda, S), mk(hw, cfg), capacity=64)
        else:
            hw.join_device(to_dev(cuda, R), to_dev(cuda, S), mk(hw, cfg))
        _GEOM[key] = hw.tables_info()
    return dict(_GEOM[key])


# ------------------------------------------------------------------------------- references
class Filter:
    """The oracle's filter built once from R's keys; passing(keys) = which keys it lets through."""

    def __init__(self, orc, cfg, hw, Rkeys):
        import ctypes
        self.orc, self.ct = orc, ctypes
        self.f = orc._Bloom()
        a = mk(hw, cfg)
        Rkeys = np.ascontiguousarray(Rkeys, dtype=np.int32)
        if orc.lib().orc_bloom_init(ctypes.byref(self.f), a.variant, a.m, a.k, a.B, 42):
            raise MemoryError
        orc.lib().orc_bloom_add_all(ctypes.byref(self.f), Rkeys.ctypes.data, Rkeys.shape[0])

    def count(self, keys):
        keys = np.ascontiguousarray(keys, dtype=np.int32)
        return int(self.orc.lib().orc_count_filtered(self.ct.byref(self.f), keys.ctypes.data, keys.shape[0]))

    def passing(self, keys):
        """Boolean mask, by bisection on orc_count_filtered (all or none of a range: no recursion)."""
        keys = np.ascontiguousarray(keys, dtype=np.int32)
        out = np.zeros(keys.size, dtype=bool)
        todo = [(0, keys.size)]
        while todo:
            lo, hi = todo.pop()
            if lo == hi:
                continue
            c = self.count(keys[lo:hi])
            if c == hi - lo:
                out[lo:hi] = True
            elif c:
                mid = (lo + hi) // 2
                todo += [(lo, mid), (mid, hi)]
        return out

    def close(self):
        self.orc.lib().orc_bloom_free(self.ct.byref(self.f))


def ref_counts(orc, hw, R, S, cfg):
    if cfg is None:
        res, filt, _ = orc.bpro(R, S, 8, 0, 0, 0, 0, use_bloom=False)
    else:
        a = mk(hw, cfg)
        res, filt, _ = orc.bpro(R, S, 8, a.variant, a.m, a.k, a.B)
    return filt, res


def sorted_pairs(p):
    p = np.ascontiguousarray(p, dtype=np.int32).reshape(-1, 2)
    return np.sort(p.view(np.uint32).astype(np.uint64) @ np.array([1 << 32, 1], dtype=np.uint64))


def jobs_of(crc, info, cfg, keys):
    """(q, job, v) of keys in the launch's job layout."""
    if info["sub_shift"] == 0:
        q, sub, v = shapes.job_of_basic(keys, info, cfg[1])
    else:
        q, sub, v = shapes.job_of(crc.code(keys), info)
    return q.astype(np.int64), q.astype(np.int64) * info["NSUB"] + sub, v.astype(np.uint64)


def read_tables(hw, info):
    T = {"r_elem_start": hw.tables_read(hw.TAB_R_ELEM_START), "s_elem_start": hw.tables_read(hw.TAB_S_ELEM_START),
         "r_sweep_start": hw.tables_read(hw.TAB_R_SWEEP_START), "s_item_start": hw.tables_read(hw.TAB_S_ITEM_START),
         "s_list_start": hw.tables_read(hw.TAB_S_LIST_START),
         "r_cnt": hw.tables_read(hw.TAB_R_RUN_CNT).reshape(-1, info["NSUB"]),
         "r_off": hw.tables_read(hw.TAB_R_RUN_OFF).reshape(-1, info["NSUB"]),
         "surv_cnt": hw.tables_read(hw.TAB_SURV_CNT).reshape(-1, info["NSUB"]),
         "surv_off": hw.tables_read(hw.TAB_SURV_OFF).reshape(-1, info["NSUB"])}
    assert T["r_cnt"].shape[0] == info["sweeps"] == T["r_sweep_start"][-1]
    assert T["surv_cnt"].shape[0] == info["items"] == T["s_item_start"][-1]
    if info["mat"]:
        with pytest.raises(hw.TablesError) as e:  # (k_join_split does not run: no parts table)
            hw.tables_read(hw.TAB_NPARTS)
        assert e.value.code == hw.TABLES_OTHER_PIPELINE
        T["nparts"], T["nextra"] = np.ones(info["jobs"], dtype=np.uint32), 0
    else:
        npx = hw.tables_read(hw.TAB_NPARTS)
        assert npx.size == info["jobs"] + 1
        T["nparts"], T["nextra"] = npx[:-1], int(npx[-1])
    return T


def run_case(hw, cuda, orc, crc, R, S, cfg, crafted=(), algo=None, mat=False, want_geom=None):
    """One join, every stage checked. crafted: jobs whose survivors are decoded and compared.
    Returns (stats, info, tables, R_dup_per_job, pairs)."""
    dR, dS = to_dev(cuda, R), to_dev(cuda, S)
    pairs = None
    if mat:
        st, pairs, _ = hw.join_materialize_device(dR, dS, mk(hw, cfg), capacity=int(1.2 * len(S)) + 4096)
        pairs = pairs.cpu().numpy()
    else:
        st = hw.join_device(dR, dS, mk(hw, cfg), algorithm=hw.ALGO_PRO if algo is None else algo)
    info = hw.tables_info()
    T = read_tables(hw, info)
    if want_geom is not None:
        assert {k: info[k] for k in GEOM} == {k: want_geom[k] for k in GEOM}
    # ---- counts
    filt, res = ref_counts(orc, hw, R, S, cfg)
    print(f"counts: filtered {st.filtered} (oracle {filt}), matches {st.matches} (oracle {res}); "
          f"key bits {info['key_bits']}, sweeps {info['sweeps']}, items {info['items']}, unstaged {st.unstaged_items}")
    assert (st.filtered, st.matches) == (filt, res)
    if mat:
        want = orc.join_pairs(R, S)
        assert np.array_equal(sorted_pairs(pairs), sorted_pairs(want))
    # ---- pass 1: element starts = the histogram of the partitions (mode 3 scatters its survivors)
    F, NSUB = info["F"], info["NSUB"]
    rq, rjob, rv = jobs_of(crc, info, cfg, R[:, 0])
    sq, sjob, sv = jobs_of(crc, info, cfg, S[:, 0])
    start = lambda q: np.concatenate([[0], np.cumsum(np.bincount(q, minlength=F))]).astype(np.uint64)
    assert np.array_equal(T["r_elem_start"], start(rq))
    assert info["mode"] != 3
    assert np.array_equal(T["s_elem_start"], start(sq))
    # ---- build: the job keys of every job's R runs, every run inside its sweep slot
    sweep_q = np.repeat(np.arange(F), np.diff(T["r_sweep_start"].astype(np.int64)))
    unit, sub, v = shapes.decode_slots(hw.tables_read(hw.TAB_R_KEYS), info["slot"], T["r_cnt"], T["r_off"],
                                       info["key_bits"], info["hash_shift"])
    got = np.sort(((sweep_q[unit] * NSUB + sub).astype(np.uint64) << np.uint64(32)) | v.astype(np.uint64))
    ref = np.sort((rjob.astype(np.uint64) << np.uint64(32)) | rv)
    assert np.array_equal(got, ref)
    dup = np.zeros(info["jobs"], dtype=bool)
    dup[(ref[1:][ref[1:] == ref[:-1]] >> np.uint64(32)).astype(np.int64)] = True
    # ---- probe: survivors per job
    item_q = np.repeat(np.arange(F), np.diff(T["s_item_start"].astype(np.int64)))
    job_surv = np.zeros((F, NSUB), dtype=np.int64)
    np.add.at(job_surv, item_q, T["surv_cnt"].astype(np.int64))
    job_surv = job_surv.ravel()
    assert int(job_surv.sum()) == st.filtered
    flt = Filter(orc, cfg, hw, R[:, 0]) if cfg is not None else None
    try:
        if cfg is None:
            assert np.array_equal(job_surv, np.bincount(sjob, minlength=info["jobs"]))
        for job in list(crafted)[:8] if cfg is not None else ():
            assert job_surv[job] == flt.count(S[sjob == job, 0]), job
        for job in crafted:  # the decoded survivors = the job's S keys that pass
            q, s = job // NSUB, job % NSUB
            got = []
            for it in range(int(T["s_item_start"][q]), int(T["s_item_start"][q + 1])):
                if T["surv_cnt"][it, s]:
                    got.append(shapes.decode_runs(hw.tables_read(hw.TAB_SURV_ITEM, it), T["surv_cnt"][it, s:s + 1],
                                                  T["surv_off"][it, s:s + 1], info["key_bits"], info["hash_shift"],
                                                  surv=True)[0])
            got = np.sort(np.concatenate(got)) if got else np.zeros(0, dtype=np.uint32)
            mine = sjob == job
            keep = flt.passing(S[mine, 0]) if flt else np.ones(int(mine.sum()), dtype=bool)
            assert np.array_equal(got, np.sort(sv[mine][keep]).astype(np.uint32)), job
    finally:
        if flt:
            flt.close()
    return st, info, T, dup, pairs


# ------------------------------------------------------------------------- relation builder
class Build:
    """Collects placements of crafted job keys for R and S (shapes.craft)."""

    def __init__(self, crc, info, nR, nS, G=None):
        self.crc, self.info, self.nR, self.nS = crc, info, nR, nS
        self.G = G or info["G"]
        self.r, self.s, self.avoid = [], [], set()

    def job(self, q, sub):
        self.avoid.add(q)
        return q * self.info["NSUB"] + sub

    def R(self, w, q, sub, v):
        self.job(q, sub)
        self.r.append((w, shapes.job_codes(self.info, q, sub, v)))

    def S(self, w, q, sub, v):
        self.job(q, sub)
        self.s.append((w, shapes.job_codes(self.info, q, sub, v)))

    def relations(self):
        R = shapes.craft(self.crc, self.info, dict(n=self.nR, G=self.G, place=self.r, avoid_q=self.avoid, salt=1))
        S = shapes.craft(self.crc, self.info, dict(n=self.nS, G=self.G, place=self.s, avoid_q=self.avoid, salt=12345))
        return R, S


def s_keys(rv, n, members_only, base):
    """n survivor job keys for a job whose R keys are rv: all members (cycled), or every other one a
    non-member (base + i: above every rv of the job)."""
    rv = np.asarray(rv)
    v = rv[np.arange(n) % rv.size].copy()
    if not members_only:
        v[1::2] = base + np.arange(v[1::2].size)
    return v


def relation_a(crc, info, members_only):
    """The relation pair of J1, J4, J6 (pieces), J8, J9 and J10: one partition per crafted job.

    Edge jobs e (partition 10 + e, sub 1): an R run of LR[e] keys and a survivor run of LS[e] keys,
    each behind a sub-0 run of 1..4 keys (so packed runs start at every bit offset 0, 2, 4, 6); all
    keys of a side in one scatter workgroup's range, so they share a sweep / an item.
    Partition 100: > kJoinWaves * JFS probe items (1024 S keys from every workgroup), sub 1 heavier
    than kJoinTaskSurv survivors. Partition 200: one repeated R key (J4). Partition 300, sub 2: a
    sweep of `slot` R keys and a second of half as many, with duplicates (J6 / J8: pieces), and > 2
    probe items. Partition 400: two full probe items and a short one of members (J9 mixed, J10)."""
    G, FW, SW, TU = info["G"], info["j_fw"], info["j_sw"], info["j_tail_u"]
    LR = [1, 15, 16, 17, 63, 64, 65, 64 * FW - 1, 64 * FW, 64 * FW + 1, 64 * FW + 64 * TU, 64 * FW + 64 * TU + 1]
    LS = [1, 64 * SW - 1, 64 * SW, 64 * SW + 1, 64 * SW + 64 * TU + 1]
    slot, CH = info["slot"], info["CH"]
    per_w = 1024  # S keys of partition 100 per workgroup
    assert G * per_w > 32 * CH * info["j_waves"] * info["j_fs"] and G * (per_w // 2 + 48) > info["j_task_surv"]
    nR, nS = G * (slot + 512), G * (per_w + 128 + 1024 + 1024)
    b = Build(crc, info, nR, nS)
    X = {"edges": [], "LR": LR, "LS": LS}
    for e, lr in enumerate(LR):
        q, ls = 10 + e, LS[e % len(LS)]
        pre_r, pre_s = (e % 4) or 4, ((e + 1) % 4) or 4
        rv = 5 + 3 * np.arange(lr)  # (uneven histogram buckets for PRH / PRHO)
        b.R(e, q, 0, np.arange(pre_r))
        b.R(e, q, 1, rv)
        b.S(e, q, 0, s_keys(np.arange(pre_r), pre_s, members_only, 1000))
        b.S(e, q, 1, s_keys(rv, ls, members_only, 100000))
        X["edges"].append((b.job(q, 1), lr, ls, pre_r % 4, pre_s % 4))
    # partition 100: many probe items; sub 1 above kJoinTaskSurv survivors
    NS_ = info["NSUB"]
    r100 = np.arange(1000)
    for s in range(NS_):
        b.R(20, 100, s, r100[s::NS_])
    heavy = per_w // 2 + 48
    light = (per_w - heavy) // (NS_ - 1)
    for w in range(G):
        for s in range(NS_):
            n = heavy if s == 1 else light
            b.S(w, 100, s, s_keys(r100[s::NS_], n, members_only, 100000 + w * 600))
    X["walk"] = [b.job(100, s) for s in range(NS_) if s != 1]
    X["heavy"] = b.job(100, 1)
    # partition 200: a repeated R key in a fused-shape job
    rv = np.concatenate([np.arange(50), [7]])
    b.R(21, 200, 3, rv)
    b.S(21, 200, 3, np.concatenate([s_keys(rv[:50], 90, members_only, 70000), [7, 7]]))
    X["dup"] = b.job(200, 3)
    # partition 300 sub 2: a full sweep of one job, then half a sweep; duplicates; >= 3 probe items
    rv = np.arange(slot) * 5 + 1
    rv[100:110] = rv[0:10]
    b.R(30, 300, 2, rv)
    b.R(31, 300, 2, np.arange(slot // 2) * 5 + 3)
    for w in range(G):
        b.S(w, 300, 2, s_keys(rv, 100, members_only, 1 << 17))
    X["pieces"] = b.job(300, 2)
    assert G * 4 > 2 * CH  # (100 keys = 4 chunks per workgroup: more than two probe items)
    # partition 400: two full probe items of members and a short third one
    r400 = np.arange(6000)
    for s in range(NS_):
        b.R(40, 400, s, r400[s::NS_][:188])
        b.R(41, 400, s, r400[s::NS_][188:])
    nw = -(-(2 * CH * 32 + 2048) // 1024)
    for w in range(nw):
        for s in range(NS_):
            b.S(50 + w, 400, s, s_keys(r400[s::NS_], 1024 // NS_, True, 0))
    X["mixed"] = [b.job(400, s) for s in range(NS_)]
    R, S = b.relations()
    return R, S, X


_REL = {}


def rel_a(hw, cuda, crc, members_only):
    if members_only not in _REL:
        _REL[members_only] = relation_a(crc, geometry(hw, cuda, None, 8), members_only)
    return _REL[members_only]


def check_edges(X, T, info, C, cls, start=None):
    """J1's readback: every crafted run length, every start offset mod 4, and the tail branches."""
    TU = 64 * info["j_tail_u"]
    for job, lr, ls, pre_r, pre_s in X["edges"]:
        c = C[(job, 0)]
        assert (c["cls"], c["start"]) == (cls, start), (job, c["cls"], c["start"])
        assert c["r_runs"] == [lr] and c["s_runs"] == [ls], (job, c["r_runs"], c["s_runs"])
        q, s = job // info["NSUB"], job % info["NSUB"]
        sw, it = int(T["r_sweep_start"][q]), int(T["s_item_start"][q])
        assert int(T["r_off"][sw, s]) % 4 == pre_r and (int(T["surv_off"][it, s]) & 0x7FFFFFFF) % 4 == pre_s
        first = 64 * (info["j_fw"] if cls == "fused" else info["j_rw"])
        assert c["r_tail"] == (lr - first >= TU, lr > first and (lr - first) % TU != 0)
        assert c["s_tail"] == (ls - 64 * info["j_sw"] >= TU, ls > 64 * info["j_sw"] and (ls - 64 * info["j_sw"]) % TU != 0)
    if cls == "fused":  # the run-length edges of the issue, on both sides of tail_run's two loops
        tails = {C[(e[0], 0)]["r_tail"] for e in X["edges"]}
        assert tails == {(False, False), (False, True), (True, False), (True, True)}
        assert {C[(e[0], 0)]["s_tail"] for e in X["edges"]} >= {(False, False), (False, True), (True, True)}
    assert {e[3] for e in X["edges"]} == {0, 1, 2, 3} == {e[4] for e in X["edges"]}


def crafted_a(X):
    return [e[0] for e in X["edges"]] + [X["dup"], X["pieces"], X["heavy"], X["walk"][0], X["mixed"][0]]


# ----------------------------------------------------------------------------- join cells
def test_j1_fused_bitmap_run_length_edges(hw, cuda, orc, crc):
    """J1 (+ J4, J6 pieces, J10's job above kJoinTaskSurv): PRO, 18-bit keys. Run lengths from
    HWBRJ_JFW / HWBRJ_JSW / kJoinTailU; the walk after the fused loads from kJoinWaves * HWBRJ_JFS."""
    R, S, X = rel_a(hw, cuda, crc, False)
    hw.join_device(to_dev(cuda, R[:64]), to_dev(cuda, S[:64]), None)  # (no unstaged item before: keys are packed)
    st, info, T, dup, _ = run_case(hw, cuda, orc, crc, R, S, None, crafted_a(X))
    assert st.join_keys == hw.JOIN_KEYS_PACKED and info["key_bits"] == 18 and info["bitmap"] == 1
    C = shapes.classify(T, info, dup, jobs=crafted_a(X) + X["walk"])
    check_edges(X, T, info, C, "fused")
    for job in X["walk"]:  # more survivor runs than the fused loads take: the walk after them
        c = C[(job, 0)]
        assert c["cls"] == "fused" and c["s_walk"] and len(c["s_runs"]) > info["j_waves"] * info["j_fs"]
    # J4: one repeated R key sends the fused job to the hash table
    assert (C[(X["dup"], 0)]["cls"], C[(X["dup"], 0)]["start"]) == ("hash", "dup_fused")
    # J6: more than kJoinPiece keys with duplicates, two pieces
    c = C[(X["pieces"], 0)]
    assert c["cls"] == "hash" and c["start"] == "dup_fused" and len(c["pieces"]) >= 2
    assert c["r_keys"] > info["j_piece"] and c["pieces"][0] == info["slot"]
    # J10 without the hook: a job above kJoinTaskSurv survivors is cut in two
    assert T["nparts"][X["heavy"]] == 2 and C[(X["heavy"], 0)]["s_keys"] + C[(X["heavy"], 1)]["s_keys"] > info["j_task_surv"]
    assert C[(X["heavy"], 1)]["cls"] == "fused" and T["nextra"] == 1


def relation_b(crc, info):
    """J2 / J5: partitions 50 and 51 hold more than kJoinWaves * HWBRJ_JFR sweeps of distinct R keys
    (every scatter workgroup sends 16 full chunks and a partial one); 51 has one repeated key."""
    G, NS_ = info["G"], info["NSUB"]
    per = -(-(info["j_fused"] + 1) * info["BSW"] // G)  # chunks per workgroup
    keys = (per - 1) * 32 + 8
    assert keys <= 64 * NS_
    b = Build(crc, info, G * 2 * (keys + 8), G * 512)
    for w in range(G):
        for q in (50, 51):
            for s in range(NS_):
                b.R(w, q, s, w * 64 + np.arange(len(range(s, keys, NS_))))  # (distinct: < 64 per workgroup)
    b.R(0, 51, 5, [7])  # (7 is workgroup 0's already: one repeated key)
    for q in (50, 51):
        b.S(3, q, 5, np.concatenate([np.arange(0, 600, 3), [7, 7], 200000 + np.arange(40)]))
    R, S = b.relations()
    return R, S, b.job(50, 5), b.job(51, 5)


def test_j2_j5_batched_bitmap_by_sweeps_and_duplicate(hw, cuda, orc, crc):
    """J2, J5: more sweeps than the fused path takes (kJoinWaves * HWBRJ_JFR); the same shape with
    one repeated R key falls back to the hash table."""
    g0 = geometry(hw, cuda, None, 8)
    R, S, j2, j5 = relation_b(crc, g0)
    st, info, T, dup, _ = run_case(hw, cuda, orc, crc, R, S, None, [j2, j5])
    C = shapes.classify(T, info, dup, jobs=[j2, j5])
    assert C[(j2, 0)]["cls"] == "batched" and len(C[(j2, 0)]["r_runs"]) > info["j_fused"]
    assert (C[(j5, 0)]["cls"], C[(j5, 0)]["start"]) == ("hash", "dup_batched")
    assert len(C[(j5, 0)]["r_runs"]) > info["j_fused"] and C[(j5, 0)]["r_batches"] == 1


def relation_j3(crc, info):
    """J3: partition 60 holds more than kJoinDesc probe items of S non-members (and a few members),
    R 4 G (about 1000) keys: a nearly empty filter, so part 0 keeps all items and few survivors."""
    G, NS_, CH = info["G"], info["NSUB"], info["CH"]
    per = -(-((info["j_desc"] + 1) * CH * 32) // G)
    b = Build(crc, info, G * 4, G * (per + 64))
    assert 3 * NS_ <= G * 4
    for s in range(NS_):
        for v in range(3):  # (a scatter workgroup's range holds 4 of R's tuples)
            b.R((3 * s + v) // 4, 60, s, [v])
    for w in range(G):
        i = 1000 + w * per + np.arange(per)
        for s in range(NS_):
            b.S(w, 60, s, np.concatenate([[s % 3], i[s::NS_] // NS_]))
    R, S = b.relations()
    return R, S, [b.job(60, s) for s in range(NS_)]


def test_j3_batched_bitmap_by_items(hw, cuda, orc, crc):
    """J3: more probe items in part 0 than kJoinDesc (two survivor descriptor batches), at most
    kJoinTaskSurv survivors; blocked filter."""
    g0 = geometry(hw, cuda, BLK, 8)
    R, S, jobs = relation_j3(crc, g0)
    st, info, T, dup, _ = run_case(hw, cuda, orc, crc, R, S, BLK, jobs[:2], want_geom=g0)
    C = shapes.classify(T, info, dup, jobs=jobs)
    for job in jobs:
        c = C[(job, 0)]
        assert T["nparts"][job] == 1 and c["cls"] == "batched" and c["s_batches"] == 2, (job, c["cls"])
        assert len(c["s_runs"]) > info["j_desc"] and 0 < c["s_keys"] <= info["j_task_surv"]


def test_j10_parts_beyond_the_task_table(hw, cuda, orc, crc, hook):
    """J10: with HWBRJ_HOOK_JOIN_SPLIT = 1 every job of J3's partition asks for one part per probe
    item, more than kJoinExtra in all: the task table truncates, the counts stay."""
    g0 = geometry(hw, cuda, None, 8)
    R, S, jobs = relation_j3(crc, g0)
    hook(hw.HOOK_JOIN_SPLIT, 1)
    st, info, T, dup, _ = run_case(hw, cuda, orc, crc, R, S, None, jobs[:1])
    assert info["split"] == 1 and T["nextra"] > info["j_extra"]
    assert int(T["nparts"].astype(np.int64).sum()) - info["jobs"] == info["j_extra"]  # (the table's bound)
    items = int(T["s_item_start"][61] - T["s_item_start"][60])
    assert items > info["j_desc"] and sorted(set(T["nparts"][jobs].tolist()))[-1] == items
    C = shapes.classify(T, info, dup, jobs=jobs)
    q, sub, _ = shapes.job_of(crc.code(S[:, 0]), info)
    assert sum(c["s_keys"] for (j, p), c in C.items() if j == jobs[0]) == int(((q == 60) & (sub == 0)).sum())


def relation_j6b(crc, info):
    """J6's second job: partitions 70 (distinct keys) and 71 (one repeated key) hold more than
    kJoinDesc sweeps: two R descriptor batches, in the bitmap and in the hash form."""
    G, NS_ = info["G"], info["NSUB"]
    per = -(-(info["j_desc"] + 1) * info["BSW"] // G)
    keys = (per - 1) * 32 + 8
    b = Build(crc, info, G * 2 * (keys + 8), G * 1024)
    assert keys <= 512 * NS_ and G * 512 <= 1 << (32 - info["hash_shift"])
    for w in range(G):
        for q in (70, 71):
            for s in range(NS_):
                b.R(w, q, s, w * 512 + np.arange(len(range(s, keys, NS_))))
    b.R(1, 71, 4, [9])  # (9 is workgroup 0's already: one repeated key)
    for q in (70, 71):
        b.S(2, q, 4, np.concatenate([np.arange(0, 3000, 7), [9, 9, 9], (1 << 17) + 90000 + np.arange(64)]))
    R, S = b.relations()
    return R, S, b.job(70, 4), b.job(71, 4)


def test_j6_two_r_descriptor_batches(hw, cuda, orc, crc):
    """J6: more sweeps in a partition than kJoinDesc, batched bitmap and hash table."""
    g0 = geometry(hw, cuda, None, 8)
    R, S, jb, jh = relation_j6b(crc, g0)
    st, info, T, dup, _ = run_case(hw, cuda, orc, crc, R, S, None, [jb, jh])
    C = shapes.classify(T, info, dup, jobs=[jb, jh])
    assert C[(jb, 0)]["cls"] == "batched" and C[(jb, 0)]["r_batches"] == 2
    c = C[(jh, 0)]
    assert (c["cls"], c["start"], c["r_batches"]) == ("hash", "dup_batched", 2) and len(c["pieces"]) >= 3


@pytest.mark.parametrize("cfg", [BLK24, BASIC1], ids=["24bit", "32bit"])
def test_j7_hash_from_the_start(hw, cuda, orc, crc, cfg):
    """J7: keys too wide for the bitmap (24-bit packed keys) and 32-bit words (basic k = 1, where the
    partition is the first filter bit's slice); one job with one piece, one with several."""
    nR0 = 1 << 20
    g0 = geometry(hw, cuda, cfg, nR0)
    G, NS_ = g0["G"], g0["NSUB"]
    big, small = g0["j_piece"] + 1000, 300
    part = -(-big // 4)  # the large job's keys come from four workgroups, the small job's from a fifth
    assert g0["bitmap"] == 0 and nR0 % (4 * G) == 0 and nR0 // G >= part
    if cfg is BASIC1:  # keys by rejection: candidates whose (partition, sub) is the job's
        cand = np.arange(1, 2 * g0["F"] * NS_ * big, dtype=np.int64).astype(np.int32)
        q, sub, _ = shapes.job_of_basic(cand, g0, cfg[1])
        ka, kb = cand[(q == 3) & (sub == 1)][:big].copy(), cand[(q == 5) & (sub == 0)][:small]
        rest = cand[(q != 3) & (q != 5)]
        assert ka.size == big and kb.size == small and rest.size >= nR0 + 3000
        ka[5] = ka[4]  # (a duplicate)
        Rk = rest[:nR0].copy()
        lo = [shapes.wg_range(nR0, G, w)[0] for w in range(5)]
        for w in range(4):
            Rk[lo[w]:lo[w] + ka[w * part:(w + 1) * part].size] = ka[w * part:(w + 1) * part]
        Rk[lo[4]:lo[4] + small] = kb
        Sk = np.concatenate([ka[::3], ka[4:5], kb, kb[:7], rest[nR0 - 500:nR0 + 3000]])
        ja, jb = 3 * NS_ + 1, 5 * NS_ + 0
        R = np.stack([Rk, np.arange(nR0, dtype=np.int32)], 1)
        S = np.stack([Sk, np.arange(Sk.size, dtype=np.int32)], 1)
    else:
        b = Build(crc, g0, nR0, G * 2048)
        va = np.arange(big) * 3
        va[5] = va[4]  # (a duplicate)
        for w in range(4):
            b.R(w, 3, 1, va[w * part:(w + 1) * part])
        b.R(4, 5, 0, np.arange(small) * 9)
        b.S(0, 3, 1, np.concatenate([va[::3], [va[4]] * 2, 1 << 20 | np.arange(50)]))
        b.S(1, 5, 0, np.concatenate([np.arange(small) * 9, np.arange(small) * 9 + 1]))
        R, S = b.relations()
        ja, jb = b.job(3, 1), b.job(5, 0)
    hw.join_device(to_dev(cuda, R[:64]), to_dev(cuda, S[:64]), mk(hw, cfg))  # (packing on)
    st, info, T, dup, _ = run_case(hw, cuda, orc, crc, R, S, cfg, [ja, jb], want_geom=g0)
    assert info["key_bits"] == (32 if cfg is BASIC1 else 24)
    C = shapes.classify(T, info, dup, jobs=[ja, jb])
    a, c = C[(ja, 0)], C[(jb, 0)]
    assert (a["cls"], a["start"]) == ("hash", "hash") == (c["cls"], c["start"])
    assert len(a["pieces"]) >= 2 and a["r_keys"] == big and c["pieces"] == [small]


@pytest.mark.parametrize("algo", ["PRH", "PRHO"])
def test_j8_histogram_joins(hw, cuda, orc, crc, algo):
    """J8: PRH and PRHO on relation A. Pieces of 1, 15, 16, 17 keys (NH = 4 and its doubling edge)
    and of a whole sweep slot (the largest NH), buckets of uneven sizes (keys 5 + 3 i: bucket starts
    that are no multiples of 4), duplicates (partitions 200 and 300)."""
    R, S, X = rel_a(hw, cuda, crc, False)
    st, info, T, dup, _ = run_case(hw, cuda, orc, crc, R, S, None, crafted_a(X),
                                   algo=hw.ALGO_PRH if algo == "PRH" else hw.ALGO_PRHO)
    assert info["jkind"] == (1 if algo == "PRH" else 2)
    C = shapes.classify(T, info, dup, jobs=crafted_a(X))
    nh = {}
    for job, lr, ls, _, _ in X["edges"]:
        c = C[(job, 0)]
        assert (c["cls"], c["start"], c["pieces"]) == ("hash", "hash", [lr])
        nh[lr] = c["nh"][0]
    assert nh[1] == nh[15] == nh[16] == 4 and nh[17] == 8
    c = C[(X["pieces"], 0)]
    assert c["pieces"][0] == info["slot"] and c["nh"][0] == info["slot"] // 4 and dup[X["pieces"]] and dup[X["dup"]]
    # uneven buckets: the sweep-slot piece's bucket starts (prefix sums of its histogram) are not all
    # multiples of 4
    v = (5 + 3 * np.arange(X["LR"][-1])) & (C[(X["edges"][-1][0], 0)]["nh"][0] - 1)
    assert (np.cumsum(np.bincount(v)) % 4 != 0).any()


def test_j9_32bit_codes(hw, cuda, orc, crc):
    """J9: J1, J4 and J6 with 32-bit codes. A join with an unstaged probe item switches packing off
    for the next one (as test_join_key_formats_across_launches does)."""
    R, S, X = rel_a(hw, cuda, crc, True)
    st0 = hw.join_device(to_dev(cuda, R), to_dev(cuda, S), mk(hw, BLK))
    assert st0.unstaged_items > 0
    st, info, T, dup, _ = run_case(hw, cuda, orc, crc, R, S, None, crafted_a(X))
    assert st.join_keys == hw.JOIN_KEYS_32 and info["key_bits"] == 32
    C = shapes.classify(T, info, dup, jobs=crafted_a(X))
    check_edges(X, T, info, C, "fused")
    assert (C[(X["dup"], 0)]["cls"], C[(X["dup"], 0)]["start"]) == ("hash", "dup_fused")
    assert C[(X["pieces"], 0)]["cls"] == "hash" and len(C[(X["pieces"], 0)]["pieces"]) >= 2


@pytest.mark.parametrize("split", [False, True], ids=["whole", "split"])
def test_j9_j10_mixed_launch(hw, cuda, orc, crc, hook, split):
    """J9 mixed: relation A under the blocked filter with packing on; partition 400's full probe
    items overflow the stage (32-bit runs), its short one is staged: jobs with both formats.
    J10: with HWBRJ_HOOK_JOIN_SPLIT the J6 job and a mixed job are cut into one part per item."""
    R, S, X = rel_a(hw, cuda, crc, True)
    g0 = geometry(hw, cuda, BLK, len(R))
    assert 32 * g0["CH"] > g0["stage_cap"] >= 2048
    hw.join_device(to_dev(cuda, R[:64]), to_dev(cuda, S[:64]), mk(hw, BLK))  # (no unstaged item: packing on)
    if split:
        hook(hw.HOOK_JOIN_SPLIT, 1)
    crafted = crafted_a(X)
    st, info, T, dup, _ = run_case(hw, cuda, orc, crc, R, S, BLK, crafted, want_geom=g0)
    assert st.join_keys == hw.JOIN_KEYS_MIXED and st.unstaged_items >= 2 and info["key_bits"] == 18
    C = shapes.classify(T, info, dup, jobs=crafted + X["mixed"])
    if not split:
        check_edges(X, T, info, C, "fused")
        for job in X["mixed"]:
            assert C[(job, 0)]["formats"] == {0, 1} and C[(job, 0)]["cls"] == "fused"
        assert (C[(X["dup"], 0)]["cls"], C[(X["dup"], 0)]["start"]) == ("hash", "dup_fused")
        assert len(C[(X["pieces"], 0)]["pieces"]) >= 2
    else:
        for job in (X["pieces"], X["mixed"][0]):
            q = job // info["NSUB"]
            items = int(T["s_item_start"][q + 1] - T["s_item_start"][q])
            assert T["nparts"][job] == items >= 3
            assert all(C[(job, p)]["cls"] != "empty" for p in range(items))
        assert {f for p in range(3) for f in C[(X["mixed"][0], p)]["formats"]} == {0, 1}
        assert all(C[(X["pieces"], p)]["cls"] == "hash" for p in range(3))


# -------------------------------------------------------------------- the materializing join
def test_m_materializing_join(hw, cuda, orc, crc):
    """M: k_join_mat's bitmap path (one and several survivor batches of kMatRCap), its hash table in
    one piece (duplicates on both sides) and in several pieces (general form, > kMatPiece R tuples and
    survivors), pairs against orc.join_pairs."""
    g00 = geometry(hw, cuda, None, 8, mat=True)
    G = g00["G"]
    big = 2 * g00["m_piece"] + 100
    assert big > g00["m_rcap"]
    nR = G * (big + 124)
    g0 = geometry(hw, cuda, None, nR, mat=True)
    b = Build(crc, g0, nR, G * (big // 4 + 256))
    b.R(0, 10, 1, np.arange(100) * 2)
    b.S(0, 10, 1, np.arange(300))
    rv = np.concatenate([np.arange(100), [5, 5, 6]])
    b.R(1, 11, 1, rv)
    b.S(1, 11, 1, np.concatenate([np.arange(0, 200, 2), [5, 5, 6, 6]]))
    rv = np.arange(big) * 2
    rv[10] = rv[11]
    b.R(2, 12, 1, rv)
    for w in range(8):
        b.S(8 + w, 12, 1, np.arange(big // 4) * 3 + w)
    b.R(3, 13, 1, np.arange(50))
    for w in range(12):
        b.S(20 + w, 13, 1, (np.arange(400) + w) % 75)
    R, S = b.relations()
    ja, jb, jc, jd = (b.job(q, 1) for q in (10, 11, 12, 13))
    st, info, T, dup, pairs = run_case(hw, cuda, orc, crc, R, S, None, [ja, jb, jc, jd], mat=True, want_geom=g0)
    assert info["mat"] == 1 and info["key_bits"] == 32 and info["bitmap"] == 1
    C = shapes.classify_mat(T, info, dup, jobs=[ja, jb, jc, jd])
    assert (C[ja]["cls"], C[ja]["s_batches"]) == ("bitmap", 1)
    assert (C[jb]["cls"], C[jb]["start"]) == ("hash1", "dup")
    assert C[jc]["cls"] == "general" and C[jc]["pieces"] >= 3 and C[jc]["s_batches"] >= 2 and C[jc]["start"] is None
    assert C[jc]["r_keys"] > info["m_rcap"]
    assert (C[jd]["cls"], C[jd]["s_batches"]) == ("bitmap", 2) and C[jd]["s_keys"] > info["m_rcap"]


# ------------------------------------------------------------------------------- readback
def test_readback_refuses(hw, cuda, orc):
    """hwbrj_tables_*: refused with their documented codes while a join is pending, for basic k >= 2
    (other tables), after a release, and with too small a buffer."""
    import ctypes
    rng = np.random.default_rng(3)
    R = np.stack([rng.permutation(50000).astype(np.int32), np.arange(50000, dtype=np.int32)], 1)
    S = np.stack([rng.integers(0, 100000, size=200000).astype(np.int32), np.arange(200000, dtype=np.int32)], 1)
    dR, dS = to_dev(cuda, R), to_dev(cuda, S)
    hw.join_device(dR, dS, None)
    assert hw.tables_info()["jobs"] == hw.tables_info()["F"] * hw.tables_info()["NSUB"]
    need = ctypes.c_uint64()
    buf = np.zeros(4, dtype=np.uint32)
    assert hw.lib().hwbrj_tables_read(hw.TAB_R_SWEEP_START, buf.ctypes.data, 16, ctypes.byref(need)) == hw.TABLES_TOO_SMALL
    assert need.value == (hw.tables_info()["F"] + 1) * 4 and not buf.any()
    assert hw.lib().hwbrj_tables_read(63, None, 0, ctypes.byref(need)) == 2
    hw.join_device_async(dR, dS, None)
    with pytest.raises(hw.TablesError) as e:
        hw.tables_info()
    assert e.value.code == hw.TABLES_PENDING
    with pytest.raises(hw.TablesError) as e:
        hw.tables_read(hw.TAB_R_RUN_CNT)
    assert e.value.code == hw.TABLES_PENDING
    hw.join_wait()
    with pytest.raises(hw.TablesError) as e:  # (an async join: no synchronous join's tables)
        hw.tables_info()
    assert e.value.code == hw.TABLES_NONE
    st = hw.join_device(dR, dS, hw.BloomFilterArgs(hw.BASIC, 1 << 20, 2, 1024))
    assert (st.filtered, st.matches) == ref_counts(orc, hw, R, S, ("basic", 1 << 20, 2, 1024))
    with pytest.raises(hw.TablesError) as e:
        hw.tables_info()
    assert e.value.code == hw.TABLES_OTHER_PIPELINE
    hw.join_device(dR, dS, None)
    hw.tables_info()
    hw.lib().hwbrj_release()
    with pytest.raises(hw.TablesError) as e:
        hw.tables_read(hw.TAB_S_ITEM_START)
    assert e.value.code == hw.TABLES_NONE


# ---------------------------------------------------------------------------- scatter cells
U32 = np.uint32
S_CELLS = ["S1", "S2a", "S2b", "S2c", "S2d", "S2e", "S2f", "S3", "S4", "S5"]


def scatter_codes(cell, info):
    """The crafted side's codes of a scatter cell: a list of code arrays (one join each)."""
    G, F, RND = info["G"], info["F"], info["sc_round"]
    l2f = F.bit_length() - 1
    uniq = lambda n, salt=0: shapes.filler_codes(info, n, (), salt)

    def in_q(q, idx):  # codes of partition q, distinct for distinct idx < 2^(32 - log2 F)
        idx = np.asarray(idx, dtype=np.uint64)
        assert idx.size == 0 or int(idx.max()) < 1 << (32 - l2f)
        return U32(q) | (idx << np.uint64(l2f)).astype(np.uint32)

    if cell == "S1":
        return [uniq(n, n) for n in list(range(10)) + [4 * G - 1, 4 * G, 4 * G + 1]]
    if cell.startswith("S2"):
        # a workgroup's range is a multiple of 4 tuples (units of 4), all but the last one's: "every
        # workgroup gets exactly L" exists for L = 0 mod 4, so kScRound - 1, kScRound + 1 and
        # 2 kScRound + 5 are the last workgroup's lengths (the others: kScRound, kScRound, 2 kScRound + 4)
        n = {"a": G * RND - 1, "b": G * RND, "c": G * RND + 1, "d": G * (2 * RND + 4) + 1,
             "e": G * (RND - 4), "f": G * (RND + 4)}[cell[2]]
        lens = [hi - lo for lo, hi in (shapes.wg_range(n, G, w) for w in range(G))]
        want = {"a": [RND] * (G - 1) + [RND - 1], "b": [RND] * G, "c": [RND] * (G - 1) + [RND + 1],
                "d": [2 * RND + 4] * (G - 1) + [2 * RND + 5], "e": [RND - 4] * G, "f": [RND + 4] * G}[cell[2]]
        assert lens == want
        return [uniq(n, ord(cell[2]))]
    if cell == "S3":  # element i of a workgroup -> partition i mod F: all F stages fill in one round
        L = 4 * RND
        assert F * 8 > info["sc_flushes"], "F stages flush in one round: more tasks than the fixed ones"
        i = np.arange(L)
        return [np.concatenate([in_q(0, w * (L // F) + i // F) | (i % F).astype(np.uint32) for w in range(G)])]
    if cell == "S4":  # one partition per workgroup receives whole rounds: kScRound / 32 direct chunks
        L = 3 * RND
        return [np.concatenate([in_q((7 * w + 3) % F, (w // F) * L + np.arange(L)) for w in range(G)])]
    if cell == "S5":  # skewed and uniform rounds alternate; the last round is a skewed partial one
        L = 4 * RND + RND // 2 + 36
        assert L % 4 == 0
        c = uniq(G * L, 5)
        for w in range(G):
            for r in (0, 2, 4):
                lo, hi = r * RND, min(L, (r + 1) * RND)
                c[w * L + lo:w * L + hi] = in_q((5 * w + r) % F, (1 << 20) + (r // 2) * RND + np.arange(hi - lo))
        return [c]
    raise KeyError(cell)


@pytest.mark.parametrize("how", ["R-F1024", "S-F1024", "R-F512", "S-F512", "R-pairs", "S-pairs"])
@pytest.mark.parametrize("cell", S_CELLS)
def test_scatter_cells(hw, cuda, orc, crc, cell, how):
    """S1-S5 with the crafted relation on the R side and on the S side, at F = 1024 (PRO) and F = 512
    (blocked, m / B = 512), and once more per side through the materializing join
    (scatter_body_pay; pairs against orc.join_pairs). Which branch of the scatter a round takes is
    recorded in no table: it is argued from the input, as follows.
      S1   0..9 tuples and 4 G - 1, 4 G, 4 G + 1: workgroups with no element, the tail alone.
      S2   workgroup lengths kScRound - 4, - 1, + 0, + 1, + 4 and 2 kScRound + 4, + 5 (a..f: see
           scatter_codes): the full-round and the partial-round loads, the tail.
      S3   element i of a workgroup goes to partition i mod F, so every stage fills in the same
           round: F flushes, F * 8 copy tasks > kScK * kScThreads, the loop past the fixed tasks.
      S4   whole rounds into one partition: kScRound / 32 chunks per round, all but the stage line
           written directly, the pending words in their skew form.
      S5   skewed and uniform rounds alternate (pskew changes every round); the last round is
           skewed and partial.
    Asserted: counts (pairs), the pass-1 element starts, every job's R keys, the survivor counts."""
    side, kind = how.split("-")
    cfg, mat = (BLK512 if kind == "F512" else None), kind == "pairs"
    info = geometry(hw, cuda, cfg, 8, mat=mat)
    for codes in scatter_codes(cell, info):
        n = codes.size
        keys = crc.key_of(codes)
        big = np.stack([keys, np.arange(n, dtype=np.int32)], 1)
        m = min(n, 3000)
        other = np.concatenate([keys[:: max(1, n // max(m, 1))][:m], crc.key_of(shapes.filler_codes(info, 500, (), 99))])
        small = np.stack([other, np.arange(other.size, dtype=np.int32)], 1)
        R, S = (big, small) if side == "R" else (small, big)
        run_case(hw, cuda, orc, crc, R, S, cfg, mat=mat)
