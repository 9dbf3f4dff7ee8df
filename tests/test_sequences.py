"""The catalog of tests/test_gpu_sequences.py (seq_catalog.py) on the host: the schedules meet their
coverage goals, and the references are sharp enough that a stale answer of another set, or a join that
ignored its validity bitmaps (a group join: S's value bitmap alone), cannot pass; the probe steps'
build cache keeps some builds for hundreds of steps and makes freed ones again."""
import itertools

import numpy as np
import pytest

import seq_catalog as sc
from test_gpu_materialize import _args

OLD_FAMILIES = ("count_t count_t_async count_k count_k_async count_km prh_t prho_t pairs_t pairs_km semi_t anti_k anti_km "
                "full_t full_km outer_s_k outer_r_t gsum_t gsum_k gminmax_t gminmax_k part_t").split()


def test_configs_are_the_materializing_tests():
    """The seven partition-slice configs, global_b4 and nobloom are test_gpu_materialize._args's; the two
    small-F ones are blocked m = 2^15, B = 512 (F = 64) and basic m = 2^10 (F = 32), both k = 1."""
    import hwbloomradixjoin_amd as hw  # (the argument class only: the library is not loaded)
    ref = _args(hw)
    assert (sc.BASIC, sc.BLOCKED, sc.SECTORIZED) == (hw.BASIC, hw.BLOCKED, hw.SECTORIZED)
    for name, c in sc.CONFIGS.items():
        if name in ref:
            a = ref[name]
            assert (c is None and a is None) or c == (a.variant, a.m, a.k, a.B), name
    assert sc.CONFIGS["blocked_f64"] == (hw.BLOCKED, 1 << 15, 1, 512) and sc.CONFIGS["basic_f32"][:3] == (hw.BASIC, 1 << 10, 1)
    assert {"nobloom", "blocked_packed", "blocked_f64", "sectorized_k2", "basic_k1", "basic_f32", "basic_k3", "global_b4",
            "two_segments"} <= set(sc.CONFIGS)


def test_families_and_steps():
    assert len(sc.FAMILIES) == len(set(sc.FAMILY_NAMES)) == 33
    refused = [(f, c) for f in sc.FAMILY_NAMES for c in sc.CONFIG_NAMES if not sc.is_step(f, c)]
    assert sorted(refused) == sorted((f, c) for f in set(sc.MASKED + ("part_t",) + sc.PROBES) for c in sc.UNSLICED)
    assert len(sc.MASKED) == 15 and len(sc.ASYNC) == 2 and len(sc.PAYLOAD) == 24
    assert len(sc.PROBES) == 10 and sc.STREAMED == ("stream_full_p", "stream_r_p")
    assert set(sc.PROBES) - set(sc.MASKED) == {"full_pu"}
    assert len(sc.STEPS) == (33 * len(sc.CONFIGS) - len(refused)) * 3 == 987
    assert [f.name for f in sc.FAMILIES[:21]] == OLD_FAMILIES  # (the families the catalog began with, in place)
    # the probe families are held against their one-shot counterpart's reference
    for p, one in (("count_p", "count_km"), ("pairs_p", "pairs_km"), ("anti_p", "anti_km"), ("full_p", "full_km"),
                   ("stream_full_p", "full_km"), ("gsum_p", "gsum_km"), ("gminmax_p", "gminmax_km")):
        assert sc.ref_of(p) == sc.ref_of(one) and sc.mask_kind(p) == sc.mask_kind(one)
    assert sc.ref_of("stream_r_p") == sc.Ref("outer", True, "OUTER_R", False) and sc.mask_kind("stream_r_p") is True
    assert sc.ref_of("full_pu") == sc.Ref("outer", True, "OUTER_FULL", False) and sc.mask_kind("full_pu") is False
    assert sc.mask_kind("gsum_km") == sc.mask_kind("gminmax_p") == "values"
    for nS in (20011, 300007, 1500000):
        b = sc.batches(nS)
        assert [x[0] for x in b[:3]] + [nS] == [0] + [x[1] for x in b[:3]] and b[3][0] == b[3][1]
        assert all(a % 32 == 0 for a, _ in b) and all(y - x > 1000 for x, y in b[:3])


def test_relation_sets():
    for name, (nR, nS, _, _) in sc.SETS.items():
        s = sc.relset(name)
        assert (s.Rk.size, s.Sk.size) == (nR, nS) == (s.nR, s.nS)
        for k, v in ((s.Rk, s.vR), (s.Sk, s.vS)):
            assert k.dtype == np.int32 and (k < 0).any()
            assert (k[v] == sc.INT_MIN).any() and (k[v] == sc.INT_MAX).any()
            assert np.unique(k).size < k.size          # duplicate keys
            assert 0.17 < (~v).mean() < 0.23           # about a fifth NULL
        assert s.Rp.min() > sc.INT_MIN and s.Sp.min() > sc.INT_MIN  # no tuple payload is the null marker
        assert s.Sv.min() == sc.INT_MIN and s.Sv.max() == sc.INT_MAX
        # S's value bitmap: a fifth NULL, not the key bitmap either way, extremes underneath
        assert s.vV.shape == s.vS.shape and 0.17 < (~s.vV).mean() < 0.23
        assert (s.vS & ~s.vV).sum() > s.nS // 10 and (~s.vS & s.vV).sum() > s.nS // 10
        assert s.Svn.dtype == np.int32 and np.array_equal(s.Svn[s.vV], s.Sv[s.vV])
        under = s.Svn[~s.vV]
        assert (under[::2] == sc.INT_MIN).all() and (under[1::2] == sc.INT_MAX).all()
        assert np.array_equal(s.Smv, s.Si[s.vS & s.vV])
        # under the NULL rows: live keys of the other side, and absent ones
        for k, v, other, ov in ((s.Rk, s.vR, s.Sk, s.vS), (s.Sk, s.vS, s.Rk, s.vR)):
            live = np.isin(k[~v], other[ov])
            assert live[::2].all() and 0.3 < live.mean() < 0.8
    assert [sc.SETS[n][:2] for n in "ABC"] == [(3001, 20011), (70001, 300007), (400000, 1500000)]


def test_schedule_meets_its_goals():
    e = sc.schedule()
    assert e == sc.schedule()  # deterministic
    n = len(sc.FAMILY_NAMES)
    assert n * n + 1 <= len(e) <= sc.CAP < len(e) + 100 and sc.CAP % 100 == 0  # (every ordered pair of families is one entry)
    met = set()
    for prev, st in zip([None] + e[:-1], e):
        assert st in sc.STEPS
        met |= set(sc.goals_of(prev, st))
    goals = sc.all_goals()
    n, c = len(sc.FAMILY_NAMES), len(sc.CONFIG_NAMES)
    assert len(goals) == len(sc.STEPS) + n * n + c * c + 9 + 2 * n * c
    assert goals <= met, sorted(goals - met)[:10]
    # chunks: each begins with its predecessor's last step, so its first transition is the schedule's
    ch = sc.chunks(e)
    assert all(len(x) <= sc.CHUNK + 1 for x in ch)
    assert all(b[0] == a[-1] for a, b in zip(ch, ch[1:]))
    assert [st for i, x in enumerate(ch) for st in (x[1:] if i else x)] == e


def test_disturber_schedule_meets_its_goals():
    d = sc.disturber_schedule()
    assert d == sc.disturber_schedule()
    assert {(x[0], x[2][0]) for x in d} == sc.disturber_goals() and len(d) == len(sc.disturber_goals())
    kinds = {x[0][0] for x in d}
    assert kinds == {"code7", "count_only", "refused9", "m_not_pow2", "misaligned", "unwaited", "release", "export_filter",
                     "tables_read", "join_split", "caller_stream", "build", "build_free", "unmatched7"}
    assert {x[0][1] for x in d if x[0][0] == "build"} == {"BUILD_COUNT", "BUILD_ROWS"}
    assert set(sc.PROBES) - {"count_p"} <= {f for f, c in {(x[0][1], x[0][2]) for x in d if x[0][0] == "code7"} if c == "blocked_packed"}
    assert {(x[0][1], x[0][2]) for x in d if x[0][0] == "code7"} == \
        {(f, c) for f in sc.PAYLOAD for c in ("blocked_packed", "global_b4") if sc.is_step(f, c)}
    assert {(x[0][1], x[0][2]) for x in d if x[0][0] == "refused9"} == {(k, c) for k in ("masked", "part", "build") for c in sc.UNSLICED}
    assert {x[0][1] for x in d if x[0][0] == "unwaited"} == {1, 3}
    for dist, dset, (f, c, s), _ in d:
        assert sc.is_step(f, c) and s in "AB" and dset in "AB" and (dset != s or dist[0] in sc.ON_B)
    assert sc.ON_B == ("join_split", "unmatched7")
    for f in sc.FAMILY_NAMES:  # the followers' configs cycle: every family meets several, on both sets
        mine = [x[2] for x in d if x[2][0] == f]
        assert len({c for _, c, _ in mine}) >= 5 and {s for _, _, s in mine} == {"A", "B"}


def _summary(orc, family, set_name):
    """What a step asserts as numbers: row count, matches, the class counts, n_pairs, and `filtered`
    under every config whose filter rejects anything."""
    e = sc.expect(orc, family, set_name)
    f = sc.FAMILY[family]
    s = sc.relset(set_name)
    mk = sc.mask_kind(family)
    passed = int((s.vS & s.vV).sum()) if mk == "values" else int(s.vS.sum()) if f.masked else s.nS
    filt = tuple(x for x in (sc.filtered(orc, set_name, c, mk) for c in sc.CONFIG_NAMES if sc.is_step(family, c))
                 if x != passed)
    return (e.n, e.matches) + (e.cls or ()) + ((e.n_pairs,) if e.n_pairs is not None else ()) + filt


@pytest.mark.parametrize("family", sc.FAMILY_NAMES)
def test_no_two_sets_share_a_number(orc, family):
    """A stale answer of another set cannot pass: every summary number differs between any two sets."""
    sums = {s: _summary(orc, family, s) for s in sc.SET_NAMES}
    for a, b in itertools.combinations(sc.SET_NAMES, 2):
        mine, theirs = {x for x in sums[a] if x}, {x for x in sums[b] if x}
        assert mine and theirs and not (mine & theirs), (family, a, b, mine & theirs)
        if not sc.FAMILY[family].op in ("count", "part"):
            ea, eb = sc.expect(orc, family, a), sc.expect(orc, family, b)
            assert ea.rows.shape != eb.rows.shape


@pytest.mark.parametrize("set_name", sc.SET_NAMES)
@pytest.mark.parametrize("family", sc.MASKED)
def test_masks_change_every_masked_reference(orc, family, set_name):
    with_masks, without = sc.expect(orc, family, set_name), sc.expect(orc, family, set_name, ignore_masks=True)
    assert (with_masks.n, with_masks.matches, with_masks.cls) != (without.n, without.matches, without.cls) or \
        sc.FAMILY[family].kind == "GROUP_ALL"  # (one row per R row, whatever the masks: the rows and n_pairs differ)
    assert (with_masks.matches, with_masks.n_pairs) != (without.matches, without.n_pairs)
    if sc.FAMILY[family].kind != "GROUP_ALL":
        assert with_masks.matches != without.matches
    else:
        assert with_masks.n == without.n == sc.relset(set_name).nR and with_masks.n_pairs < without.n_pairs
    if with_masks.rows is not None:
        assert not np.array_equal(with_masks.rows, without.rows)
    for c in sc.CONFIG_NAMES:
        if sc.is_step(family, c):
            assert sc.counts(orc, set_name, c, sc.mask_kind(family)) != sc.counts(orc, set_name, c, False)


@pytest.mark.parametrize("set_name", sc.SET_NAMES)
@pytest.mark.parametrize("family", [f for f in sc.MASKED if sc.mask_kind(f) == "values"])
def test_the_value_bitmap_alone_changes_every_masked_group_reference(orc, family, set_name):
    """A kernel that honours vR and vS but drops sv_valid cannot pass: the rows, n_pairs and (under every
    config) `filtered` differ, and the values that would leak are the extremes planted under vV."""
    want, leak = sc.expect(orc, family, set_name), sc.expect(orc, family, set_name, ignore_masks="vV")
    assert want.n_pairs < leak.n_pairs
    assert not np.array_equal(want.rows, leak.rows)
    if sc.FAMILY[family].kind == "GROUP_ALL":
        assert want.n == leak.n == sc.relset(set_name).nR
    else:
        assert want.n < leak.n
    changed = [c for c in sc.CONFIG_NAMES if sc.is_step(family, c)
               and sc.counts(orc, set_name, c, "values")[1] != sc.counts(orc, set_name, c, True)[1]]
    assert len(changed) == len(sc.SLICED), changed
    assert {sc.counts(orc, set_name, c, "values")[0] for c in sc.SLICED} == {want.n_pairs}
    s = sc.relset(set_name)
    hit = s.vS & ~s.vV & np.isin(s.Sk, s.Rk[s.vR])  # the S rows that would leak into a group
    assert hit.sum() > 100 and set(np.unique(s.Svn[hit])) == {sc.INT_MIN, sc.INT_MAX}


def test_the_build_cache_keeps_elders_and_makes_freed_builds_again():
    """The probe steps' builds over the main schedule: never more than LIVE_BUILDS alive, some probed
    again 200 steps and more after they were made, and most made again after they were freed."""
    now, born, freed, alive, ages, again = [0], {}, set(), set(), [], 0

    def make(key):
        born[key] = now[0]
        alive.add(key)
        assert len(alive) <= sc.LIVE_BUILDS
        return key

    def free(key):
        alive.remove(key)
        freed.add(key)

    cache = sc.BuildCache(make, free)
    for t, st in enumerate(sc.schedule()):
        now[0] = t
        if st[0] in sc.PROBES:
            key = sc.build_key(*st)
            if key in alive:
                ages.append(now[0] - born[key])
            else:
                again += key in freed
            assert cache.get(key) == key and key in alive
    assert sorted(cache.live()) == sorted(alive) and len(alive) == sc.LIVE_BUILDS
    assert sum(a >= 200 for a in ages) >= 3 and again >= 100, (sorted(ages)[-5:], again)
    cache.clear()
    assert not alive


@pytest.mark.parametrize("set_name", sc.SET_NAMES)
def test_three_match_counts_agree(orc, set_name):
    """orc.join_pairs, orc.bpro (every config) and the sum of the group counts: one match count."""
    n = sc.pairs(orc, set_name).shape[0]
    assert n > 0
    assert {sc.counts(orc, set_name, c)[0] for c in sc.CONFIG_NAMES} == {n}
    for fam in ("gsum_t", "gsum_k", "gminmax_t", "gminmax_k"):
        e = sc.expect(orc, fam, set_name)
        assert e.n_pairs == n
        assert int((e.rows[:, 0] >> np.uint64(32)).sum()) == n  # the rows' own counts
    # vS & vV: the masked group joins' pair total, their rows' own counts, and orc.bpro on those rows
    relv = sc.relset(set_name)
    nv = orc.join_pairs(relv.Rm, relv.Smv).shape[0]
    for fam in ("gsum_km", "gminmax_km", "gsum_p", "gminmax_p"):
        e = sc.expect(orc, fam, set_name)
        assert e.n_pairs == nv and int((e.rows[:, 0] >> np.uint64(32)).sum()) == nv
    assert {sc.counts(orc, set_name, c, "values")[0] for c in sc.SLICED} == {nv}
    assert 0 < nv < sc.pairs(orc, set_name, masked=True).shape[0]
    s = sc.relset(set_name)
    p = sc.pairs(orc, set_name)
    assert np.array_equal(s.Rk[p[:, 0]], s.Sk[p[:, 1]])
    m = sc.pairs(orc, set_name, masked=True)
    assert 0 < m.shape[0] < n and s.vR[m[:, 0]].all() and s.vS[m[:, 1]].all()
    assert {sc.counts(orc, set_name, c, True)[0] for c in sc.CONFIG_NAMES if c not in sc.UNSLICED} == {m.shape[0]}
