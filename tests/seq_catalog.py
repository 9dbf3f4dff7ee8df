"""The catalog behind tests/test_sequences.py and tests/test_gpu_sequences.py: relation sets, filter
configurations, join families, their host references and the two schedules that run every join entry
after every other on one engine. Host only: numpy and the oracle, neither torch nor the library.

A step is (family, config, set). Its reference is computed here once per (reference, set) from
orc.join_pairs, np.isin and a sort plus reduceat, `filtered` once per (set, config) from orc.bpro:
nothing is ever compared with the library's output of another call. A probe of a prepared build
(layout p) has the reference of the one-shot join of the same R and S."""
import random
from collections import OrderedDict, namedtuple

import numpy as np

INT_MIN, INT_MAX = -2**31, 2**31 - 1
NULL_T, NULL_K = INT_MIN, -1  # the null payload of the tuple outer joins (no payload is INT_MIN) / of key columns
BASIC, BLOCKED, SECTORIZED = 0, 1, 2
MODE_NOBLOOM, MODE_BLOCK, MODE_BASIC, MODE_GLOBAL = 0, 1, 2, 3

# ------------------------------------------------------------------------------ relation sets
# name: (|R|, |S|, seed, share of S drawn from R's keys)
SETS = {"A": (3001, 20011, 1101, 0.40), "B": (70001, 300007, 2202, 0.55), "C": (400000, 1500000, 3303, 0.22)}
SET_NAMES = tuple(SETS)


def _i32(a):
    return np.ascontiguousarray(np.asarray(a).astype(np.int64).astype(np.int32))


def rows2(a, b):
    """(n, 2) int32 rows of two columns."""
    return np.ascontiguousarray(np.stack([_i32(a).ravel(), _i32(b).ravel()], 1)).reshape(-1, 2)


def u64(rows):
    """Sorted rows, each (n, 2) int32 row as one 64-bit word: an exact multiset comparison."""
    return np.sort(np.ascontiguousarray(_i32(rows).reshape(-1, 2)).view(np.uint64).ravel())


def g64(rows):
    """(n, 4) int32 group rows as two uint64 views {r_payload, count} and {a, b}, rows sorted."""
    v = np.ascontiguousarray(_i32(rows).reshape(-1, 4)).view(np.uint64).reshape(-1, 2)
    return v[np.lexsort((v[:, 1], v[:, 0]))]


def plant(Rk, Sk, vR, vS, rng):
    """Under NULL rows, alternately a live key of the other side and an absent key (the rule of _plant in
    test_gpu_keys_nulls.py): a kernel that ignores a mask bit makes extra pairs or loses anti rows."""
    nr, ns = np.nonzero(~vR)[0], np.nonzero(~vS)[0]
    liveR, liveS = Rk[vR].copy(), Sk[vS].copy()
    absent = -(np.arange(nr.size + ns.size, dtype=np.int64) + 7) * 2654435761 % (2**31)
    Rk[nr[::2]] = rng.choice(liveS, size=nr[::2].size)
    Rk[nr[1::2]] = absent[: nr[1::2].size]
    Sk[ns[::2]] = rng.choice(liveR, size=ns[::2].size)
    Sk[ns[1::2]] = absent[nr.size: nr.size + ns[1::2].size]


class RelSet:
    """One relation set: key columns Rk, Sk (duplicates on both sides, negative keys, INT_MIN and INT_MAX
    on both), tuple payloads Rp, Sp (never INT_MIN), S's value column Sv (the whole int32 range) and the
    validity arrays vR, vS (about a fifth NULL, planted keys underneath). For the group joins with
    validity bitmaps: vV, the validity of S's values (about a fifth NULL, not vS), and Svn, Sv with
    INT_MIN / INT_MAX alternating under the NULL value bits (test_gpu_keys_group_nulls._poison). Both are
    drawn from a generator of their own, so every other array is what it was without them."""

    def __init__(self, name):
        nR, nS, seed, share = SETS[name]
        rng = np.random.default_rng(seed)
        self.name, self.nR, self.nS = name, nR, nS
        dom = rng.integers(INT_MIN, INT_MAX, size=nR, endpoint=True)       # R's key domain, negative keys included
        Rk = rng.choice(dom, size=nR)                                      # with replacement: duplicates
        Sk = np.where(rng.random(nS) < share, rng.choice(dom, size=nS), rng.integers(INT_MIN, INT_MAX, size=nS, endpoint=True))
        vR, vS = rng.random(nR) >= 0.2, rng.random(nS) >= 0.2
        for k, v, rows in ((Rk, vR, (0, nR // 2, nR - 1)), (Sk, vS, (1, nS // 3, nS // 2, nS - 1))):
            k[list(rows)] = [INT_MIN, INT_MAX, INT_MIN, INT_MAX][: len(rows)]
            v[list(rows)] = True
        Rk, Sk = _i32(Rk), _i32(Sk)
        plant(Rk, Sk, vR, vS, rng)
        self.Rk, self.Sk, self.vR, self.vS = Rk, Sk, vR, vS
        self.Rp = _i32(rng.integers(INT_MIN + 1, INT_MAX, size=nR, endpoint=True))
        self.Sp = _i32(rng.integers(INT_MIN + 1, INT_MAX, size=nS, endpoint=True))
        Sv = rng.integers(INT_MIN, INT_MAX, size=nS, endpoint=True)
        Sv[[0, nS - 1]] = [INT_MIN, INT_MAX]
        self.Sv = _i32(Sv)
        self.R, self.S = rows2(Rk, self.Rp), rows2(Sk, self.Sp)            # the tuple relations
        self.Ri, self.Si = rows2(Rk, np.arange(nR)), rows2(Sk, np.arange(nS))  # {key, row}: what a key-column entry sees
        rR, rS = np.nonzero(vR)[0], np.nonzero(vS)[0]
        self.Rm, self.Sm = self.Ri[rR], self.Si[rS]                        # the compacted valid rows, original indices
        rng2 = np.random.default_rng(seed + 7)
        self.vV = rng2.random(nS) >= 0.2
        Svn = self.Sv.copy()
        at = np.nonzero(~self.vV)[0]
        Svn[at[::2]], Svn[at[1::2]] = INT_MIN, INT_MAX
        self.Svn = Svn
        self.Smv = self.Si[np.nonzero(vS & self.vV)[0]]                    # the S rows that take part in a masked group join


_SETS = {}


def relset(name):
    if name not in _SETS:
        _SETS[name] = RelSet(name)
    return _SETS[name]


# ---------------------------------------------------------------------------- configurations
# name: None (no filter) or (variant, m, k, B): the nine of test_gpu_materialize._args, and the two
# small-F ones blocked_f64 and basic_f32 (F = 64, F = 32)
CONFIGS = {
    "nobloom": None,
    "blocked_packed": (BLOCKED, 1 << 24, 1, 1024),
    "blocked_code": (BLOCKED, 1 << 24, 1, 2048),
    "blocked_k3": (BLOCKED, 1 << 24, 3, 512),
    "blocked_f64": (BLOCKED, 1 << 15, 1, 512),
    "sectorized_k2": (SECTORIZED, 1 << 24, 2, 1024),
    "basic_k1": (BASIC, 1 << 24, 1, 1024),
    "basic_f32": (BASIC, 1 << 10, 1, 1024),
    "basic_k3": (BASIC, 1 << 22, 3, 1024),
    "global_b4": (BLOCKED, 1 << 20, 1, 4),
    "two_segments": (BLOCKED, 1 << 31, 1, 1024),
}
CONFIG_NAMES = tuple(CONFIGS)
UNSLICED = ("global_b4", "basic_k3")  # refused (9) with validity bitmaps and by the partitioned join


def config_mode(name):
    """hwbrj_stats_t.mode of a configuration."""
    c = CONFIGS[name]
    if c is None:
        return MODE_NOBLOOM
    if name == "global_b4":
        return MODE_GLOBAL
    return MODE_BASIC if c[0] == BASIC else MODE_BLOCK


# ---------------------------------------------------------------------------------- families
# op: count | pairs | semi | outer | group | minmax | part; layout: t (tuples) | k (key columns) | p (key
# columns, a probe of a prepared build); kind: the entry's kind argument by name (or the HWBRJ_ALGO_* of
# a counting join; PROBE_MARK_*: the outer join streamed over batches of S, then the unmatched R rows);
# masked: with validity bitmaps (the group joins: S's value bitmap too); wait: async
Family = namedtuple("Family", "name op layout masked kind wait")
FAMILIES = (
    Family("count_t", "count", "t", False, "ALGO_PRO", False),
    Family("count_t_async", "count", "t", False, "ALGO_PRO", True),
    Family("count_k", "count", "k", False, "ALGO_PRO", False),
    Family("count_k_async", "count", "k", False, "ALGO_PRO", True),
    Family("count_km", "count", "k", True, "ALGO_PRO", False),
    Family("prh_t", "count", "t", False, "ALGO_PRH", False),
    Family("prho_t", "count", "t", False, "ALGO_PRHO", False),
    Family("pairs_t", "pairs", "t", False, None, False),
    Family("pairs_km", "pairs", "k", True, None, False),
    Family("semi_t", "semi", "t", False, "JOIN_SEMI", False),
    Family("anti_k", "semi", "k", False, "JOIN_ANTI", False),
    Family("anti_km", "semi", "k", True, "JOIN_ANTI", False),
    Family("full_t", "outer", "t", False, "OUTER_FULL", False),
    Family("full_km", "outer", "k", True, "OUTER_FULL", False),
    Family("outer_s_k", "outer", "k", False, "OUTER_S", False),
    Family("outer_r_t", "outer", "t", False, "OUTER_R", False),
    Family("gsum_t", "group", "t", False, "GROUP_ALL", False),
    Family("gsum_k", "group", "k", False, "GROUP_ALL", False),
    Family("gminmax_t", "minmax", "t", False, "GROUP_MATCHED", False),
    Family("gminmax_k", "minmax", "k", False, "GROUP_MATCHED", False),
    Family("part_t", "part", "t", False, None, False),
    Family("gsum_km", "group", "k", True, "GROUP_ALL", False),
    Family("gminmax_km", "minmax", "k", True, "GROUP_MATCHED", False),
    Family("count_p", "count", "p", True, "ALGO_PRO", False),
    Family("pairs_p", "pairs", "p", True, None, False),
    Family("semi_p", "semi", "p", True, "JOIN_SEMI", False),
    Family("anti_p", "semi", "p", True, "JOIN_ANTI", False),
    Family("full_p", "outer", "p", True, "OUTER_FULL", False),
    Family("full_pu", "outer", "p", False, "OUTER_FULL", False),
    Family("stream_full_p", "outer", "p", True, "PROBE_MARK_S", False),
    Family("stream_r_p", "outer", "p", True, "PROBE_MARK_INNER", False),
    Family("gsum_p", "group", "p", True, "GROUP_ALL", False),
    Family("gminmax_p", "minmax", "p", True, "GROUP_MATCHED", False),
)
FAMILY = {f.name: f for f in FAMILIES}
FAMILY_NAMES = tuple(FAMILY)
PAYLOAD = tuple(f.name for f in FAMILIES if f.op in ("pairs", "semi", "outer", "group", "minmax"))
MASKED = tuple(f.name for f in FAMILIES if f.masked)
ASYNC = tuple(f.name for f in FAMILIES if f.wait)
PROBES = tuple(f.name for f in FAMILIES if f.layout == "p")
STREAMED = tuple(f.name for f in FAMILIES if (f.kind or "").startswith("PROBE_MARK"))
STREAMED_AS = {"PROBE_MARK_S": "OUTER_FULL", "PROBE_MARK_INNER": "OUTER_R"}  # the one-shot join a streamed one adds up to


def is_step(family, config):
    """Whether the header puts (family, config) inside its contract (else: a refusal with code 9)."""
    f = FAMILY[family]
    return not ((f.masked or f.op == "part" or f.layout == "p") and config in UNSLICED)


def mask_kind(family):
    """Which rows a family's join sees: False (all), True (the valid keys: vR, vS) or "values" (a group
    join with bitmaps: vR, and S rows whose key and value are both valid, vS & vV)."""
    f = FAMILY[family]
    return "values" if f.masked and f.op in ("group", "minmax") else f.masked


def build_key(family, config, set_name):
    """The prepared build a probe step uses: (set, config, purpose, masked)."""
    f = FAMILY[family]
    assert f.layout == "p"
    return (set_name, config, "BUILD_COUNT" if f.op == "count" else "BUILD_ROWS", f.masked)


def batches(nS):
    """A streamed step's batches of S, [a, b): three that partition it, cut at multiples of 32 rows (a
    bitmap's byte a / 8 is then a 4-byte boundary), and an empty one."""
    c1, c2 = nS // 3 // 32 * 32, 2 * nS // 3 // 32 * 32
    return ((0, c1), (c1, c2), (c2, nS), (c2, c2))


STEPS = tuple((f, c, s) for f in FAMILY_NAMES for c in CONFIG_NAMES for s in SET_NAMES if is_step(f, c))

# ---------------------------------------------------------------------------------- references
# rows: sorted uint64 (g64 for the group joins), or None for a counting join; n: the row count (0 for a
# counting join); matches: stats.matches; cls: n_class or None; n_pairs: the group joins' pair total
Expect = namedtuple("Expect", "rows n matches cls n_pairs")
_PAIRS, _HITS, _EXPECT, _FILTERED = {}, {}, {}, {}


def pairs(orc, set_name, masked=False):
    """{R row, S row} of every match, from the oracle (masked: on the compacted valid rows)."""
    key = (set_name, masked)
    if key not in _PAIRS:
        s = relset(set_name)
        _PAIRS[key] = orc.join_pairs(s.Rm, s.Sm) if masked else orc.join_pairs(s.Ri, s.Si)
    return _PAIRS[key]


def group_rows(Rk, Rp, Sk, Sv, minmax):
    """One (r_payload, count, a, b) int32 row per R row: a, b = the int64 sum's low and high words, or
    min and max (INT_MAX, INT_MIN for an empty group); and the sum of the counts. A sort of S by key and
    one reduceat per aggregate (test_gpu_side_pass.group_rows)."""
    order = np.argsort(Sk, kind="stable")
    sk, sv = Sk[order], Sv[order].astype(np.int64)
    uk, start, c = np.unique(sk, return_index=True, return_counts=True)
    pos = np.minimum(np.searchsorted(uk, Rk), uk.size - 1)
    hit = uk[pos] == Rk
    count = np.where(hit, c[pos], 0)
    if minmax:
        a = np.where(hit, np.minimum.reduceat(sv, start)[pos], INT_MAX)
        b = np.where(hit, np.maximum.reduceat(sv, start)[pos], INT_MIN)
    else:
        s = np.where(hit, np.add.reduceat(sv, start)[pos], 0).astype(np.int64)
        a, b = s & 0xFFFFFFFF, s >> 32
    rows = np.ascontiguousarray(np.stack([_i32(Rp), _i32(count), _i32(a), _i32(b)], 1))
    return rows, int(count.sum())


def _hits(s, masked):
    """(S rows with a partner in R, R rows with a partner in S), among the valid rows."""
    key = (s.name, masked)
    if key not in _HITS:
        vR, vS = (s.vR, s.vS) if masked else (np.ones(s.nR, bool), np.ones(s.nS, bool))
        _HITS[key] = (vS & np.isin(s.Sk, s.Rk[vR]), vR & np.isin(s.Rk, s.Sk[vS]))
    return _HITS[key]


Ref = namedtuple("Ref", "op keys kind nulls")  # what a reference depends on: several families share one


def ref_of(family):
    """The reference a family is held against: its op, whether rows are row indices (key columns, probes
    included), the one-shot kind, and whether it is a group join that reads Svn."""
    f = FAMILY[family]
    keys = f.layout in ("k", "p")
    if f.op in ("count", "part"):
        return Ref("count", False, None, False)
    return Ref(f.op, keys, STREAMED_AS.get(f.kind, f.kind), f.masked and f.op in ("group", "minmax"))


def _masked_group_rows(s, r, values):
    """The group joins with validity bitmaps, on the valid rows alone: a valid R row keeps its position
    as r_payload, an S row takes part iff its key and (values) its value are valid; under GROUP_ALL a
    NULL R row gives its identity row."""
    minmax = r.op == "minmax"
    rR, v = np.nonzero(s.vR)[0], (s.vS & s.vV if values else s.vS)
    rows, n_pairs = group_rows(s.Rk[rR], rR, s.Sk[v], s.Svn[v], minmax)
    if r.kind == "GROUP_MATCHED":
        return rows[rows[:, 1] != 0], n_pairs
    nulls = np.nonzero(~s.vR)[0]
    ident = (0, INT_MAX, INT_MIN) if minmax else (0, 0, 0)
    null_rows = np.stack([_i32(nulls)] + [np.full(nulls.size, x, np.int32) for x in ident], 1)
    return np.ascontiguousarray(np.concatenate([rows, null_rows])), n_pairs


def _expect(orc, r, s, masked):
    """Reference r on set s with the masks honoured (masked: True, or "values" with vV too) or ignored."""
    keys = r.keys
    p = pairs(orc, s.name, bool(masked))
    if r.op == "count":
        return Expect(None, 0, p.shape[0], None, None)
    Rp, Sp, null = (np.arange(s.nR), np.arange(s.nS), NULL_K) if keys else (s.Rp, s.Sp, NULL_T)
    inner = rows2(np.asarray(Rp)[p[:, 0]], np.asarray(Sp)[p[:, 1]])
    if r.op == "pairs":
        return Expect(u64(inner), p.shape[0], p.shape[0], None, None)
    if r.op in ("group", "minmax"):
        if masked:
            rows, n_pairs = _masked_group_rows(s, r, masked == "values")
        else:
            Sv = (s.Svn if r.nulls else s.Sv) if keys else s.Sp
            rows, n_pairs = group_rows(s.Rk, Rp, s.Sk, Sv, r.op == "minmax")
            if r.kind == "GROUP_MATCHED":
                rows = rows[rows[:, 1] != 0]
        return Expect(g64(rows), rows.shape[0], rows.shape[0], None, n_pairs)
    # existence and class rows: np.isin on the valid rows; a NULL row has no partner
    s_hit, r_hit = _hits(s, masked)
    if r.op == "semi":
        keep = ~s_hit if r.kind == "JOIN_ANTI" else s_hit
        rows = rows2(s.Sk[keep], np.asarray(Sp)[keep])
        return Expect(u64(rows), rows.shape[0], rows.shape[0], None, None)
    keep_s, keep_r = r.kind != "OUTER_R", r.kind != "OUTER_S"
    s_only = rows2(np.full(int((~s_hit).sum()), null), np.asarray(Sp)[~s_hit]) if keep_s else np.empty((0, 2), np.int32)
    r_only = rows2(np.asarray(Rp)[~r_hit], np.full(int((~r_hit).sum()), null)) if keep_r else np.empty((0, 2), np.int32)
    rows = np.concatenate([inner, s_only, r_only])
    return Expect(u64(rows), rows.shape[0], rows.shape[0], (inner.shape[0], s_only.shape[0], r_only.shape[0]), None)


def expect(orc, family, set_name, ignore_masks=False):
    """The reference of (family, set). ignore_masks: what a masked family would return without its
    bitmaps (True), or a masked group join without S's value bitmap alone ("vV"); test_sequences.py
    shows that both differ."""
    masked = mask_kind(family)
    if ignore_masks:
        masked = bool(masked) and ignore_masks == "vV"
    key = (ref_of(family), set_name, masked)
    if key not in _EXPECT:
        _EXPECT[key] = _expect(orc, key[0], relset(set_name), masked)
    return _EXPECT[key]


def counts(orc, set_name, config, masked=False):
    """(matches, filtered) of the counting join, from orc.bpro (masked: on the compacted valid rows;
    "values": R compacted by vR, S by vS & vV, what a group join with bitmaps filters)."""
    key = (set_name, config, masked)
    if key not in _FILTERED:
        s, c = relset(set_name), CONFIGS[config]
        R, S = (s.Rm, s.Smv) if masked == "values" else (s.Rm, s.Sm) if masked else (s.Ri, s.Si)
        if c is None:
            res, filt, _ = orc.bpro(R, S, 8, 0, 0, 0, 0, use_bloom=False)
        else:
            res, filt, _ = orc.bpro(R, S, 8, c[0], c[1], c[2], c[3])
        _FILTERED[key] = (res, filt)
    return _FILTERED[key]


def filtered(orc, set_name, config, masked=False):
    return counts(orc, set_name, config, masked)[1]


# ------------------------------------------------------------------------------ the schedule
CAP, CHUNK, SEED = 1100, 25, 20251
LIVE_BUILDS, ELDERS, ELDER_EVERY = 8, 2, 40


class BuildCache:
    """The prepared builds the probe steps share, by build_key. A build is made on first use and kept; at
    most LIVE_BUILDS are alive, in two generations, each freed oldest first: every ELDER_EVERY-th build
    made is one of the ELDERS, which live through some 2 * ELDER_EVERY other builds (probed again after
    hundreds of other joins), the others are freed after LIVE_BUILDS - ELDERS later ones (and made again
    when their key returns). make(key) and free(build) are the caller's."""

    def __init__(self, make, free):
        self.make, self.free, self.made = make, free, 0
        self.young, self.elder = OrderedDict(), OrderedDict()

    def get(self, key):
        for q in (self.young, self.elder):
            if key in q:
                return q[key]
        q, cap = (self.elder, ELDERS) if self.made % ELDER_EVERY == 0 else (self.young, LIVE_BUILDS - ELDERS)
        self.made += 1
        if len(q) == cap:
            self.free(q.popitem(last=False)[1])
        q[key] = self.make(key)
        return q[key]

    def live(self):
        return list(self.elder.values()) + list(self.young.values())

    def clear(self):
        for q in (self.young, self.elder):
            while q:
                self.free(q.popitem(last=False)[1])


def goals_of(prev, step):
    """The coverage goals an entry meets: its step, and with its predecessor the ordered pairs of
    families, configs, sets, (family, next config) and (config, next family)."""
    f, c, s = step
    g = [("step", step)]
    if prev is not None:
        pf, pc, ps = prev
        g += [("ff", pf, f), ("cc", pc, c), ("ss", ps, s), ("fc", pf, c), ("cf", pc, f)]
    return g


def all_goals():
    fs, cs, ss = FAMILY_NAMES, CONFIG_NAMES, SET_NAMES
    g = {("step", st) for st in STEPS}
    g |= {("ff", a, b) for a in fs for b in fs} | {("cc", a, b) for a in cs for b in cs}
    g |= {("ss", a, b) for a in ss for b in ss}
    g |= {("fc", a, b) for a in fs for b in cs if any(is_step(f, b) for f in fs)}
    g |= {("cf", a, b) for a in cs for b in fs}
    return g


def schedule():
    """A deterministic greedy walk over the steps: each entry is the step that meets the most goals
    still open after its predecessor (ties: the step that opens the most, then a seeded draw)."""
    rng = random.Random(SEED)
    todo, out, prev = all_goals(), [], None
    while todo:
        # what a step would leave reachable: open goals that have its family / config / set first
        first = {}
        for g in todo:
            if g[0] != "step":
                first[(g[0][0], g[1])] = first.get((g[0][0], g[1]), 0) + 1
        best, best_score = [], (-1, -1)
        for st in STEPS:
            gain = sum(1 for g in goals_of(prev, st) if g in todo)
            opens = first.get(("f", st[0]), 0) + first.get(("c", st[1]), 0) + first.get(("s", st[2]), 0)
            if (gain, opens) > best_score:
                best, best_score = [st], (gain, opens)
            elif (gain, opens) == best_score:
                best.append(st)
        st = best[rng.randrange(len(best))]
        todo -= set(goals_of(prev, st))
        out.append(st)
        prev = st
        assert len(out) <= 4 * CAP, "the walk does not converge"
    return out


def chunks(entries, size=CHUNK):
    """The schedule in chunks; each chunk but the first begins by repeating its predecessor's last
    step, so a chunk run alone still makes its first transition."""
    out = []
    for i in range(0, len(entries), size):
        out.append(([entries[i - 1]] if i else []) + entries[i: i + size])
    return out


# ------------------------------------------------------------------------- the disturber schedule
# (kind, family or None, config or None): what runs, deliberately, before a follower step
def disturbers():
    d = [("code7", f, c) for c in ("blocked_packed", "global_b4") for f in PAYLOAD if is_step(f, c)]
    d += [("count_only", None, None)]
    d += [("refused9", kind, c) for kind in ("masked", "part", "build") for c in UNSLICED]
    d += [("m_not_pow2", None, None), ("misaligned", None, None), ("unwaited", 1, None), ("unwaited", 3, None),
          ("release", None, None), ("export_filter", None, None), ("tables_read", None, None), ("join_split", None, None),
          ("caller_stream", None, None)]
    # prepared builds: one made in front of the follower and probed behind it; one made, probed and freed;
    # the unmatched rows above their capacity
    d += [("build", "BUILD_COUNT", None), ("build", "BUILD_ROWS", None), ("build_free", None, None), ("unmatched7", None, None)]
    return d


SLICED = tuple(c for c in CONFIG_NAMES if c not in UNSLICED)  # the configurations of a prepared build
ON_B = ("join_split", "unmatched7")  # disturbers that need set B


def disturber_schedule():
    """Every disturber followed once by every family: entries (disturber, its set, follower step, i). The
    follower's set alternates between A and B and the disturber runs on the other one (join_split: always
    on B, the set with jobs above 700 survivors; unmatched7: always on B, the set with more than 1,000
    unmatched R rows); the follower's config cycles over the ones valid for
    its family; i (the entry's index) picks what a disturber cycles over."""
    out, i = [], 0
    for nd, d in enumerate(disturbers()):
        for nf, f in enumerate(FAMILY_NAMES):
            valid = [c for c in CONFIG_NAMES if is_step(f, c)]
            s = "AB"[(nd + nf) % 2]
            dset = "B" if d[0] in ON_B else "BA"[(nd + nf) % 2]
            out.append((d, dset, (f, valid[(nd + nf) % len(valid)], s), i))
            i += 1
    return out


def disturber_goals():
    return {(d, f) for d in disturbers() for f in FAMILY_NAMES}
