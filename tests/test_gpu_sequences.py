"""Every join entry after every other on one engine (seq_catalog.py): the engine's buffers only grow and
are never cleared wholesale, so each join relies on what its predecessor left behind. The schedule runs
every (family, config, set) step and every ordered pair of families, configs and sets; the disturber
schedule puts a refusal, a capacity overflow, un-waited async joins, hwbrj_release, a readback, a hook
or another stream in front of every family.

Every step asserts its return code, stats.matches, stats.filtered (the oracle's), stats.mode, the exact
row multiset, n_class / n_pairs and an untouched guard region behind its output buffer, each against
the host references of seq_catalog.py. Row multisets are compared on the device as sorted 64-bit views
of the rows (the group joins' 16-byte rows as two such views, sorted by both). A failure names the step
and its predecessor."""
import ctypes
import re

import numpy as np
import pytest

import seq_catalog as sc

pytestmark = pytest.mark.gpu

GUARD, GUARD_ROWS = 0x5A5A5A5A, 4096  # (a whole LDS row stage of the side passes flushed past the capacity would land there)
SCHEDULE = sc.chunks(sc.schedule())
_D = sc.disturber_schedule()
DISTURBERS = [_D[i: i + sc.CHUNK] for i in range(0, len(_D), sc.CHUNK)]  # (each entry brings its own predecessor)


class Dev:
    """A relation set on the device, each array in an allocation of exactly its size: tuples, key
    columns, S's value column and the packed validity bitmaps (ceil(n / 32) * 4 bytes)."""

    def __init__(self, cuda, s):
        def exact(a):
            a = np.ascontiguousarray(a)
            t = cuda.empty(a.shape, dtype=cuda.uint8 if a.dtype == np.uint8 else cuda.int32, device="cuda:0")
            t.copy_(cuda.from_numpy(a))
            return t

        def bitmap(valid):
            bits = np.zeros((valid.size + 31) // 32 * 32, bool)
            bits[: valid.size] = valid
            return exact(np.packbits(bits, bitorder="little"))

        self.dR, self.dS = exact(s.R), exact(s.S)
        self.cR, self.cS, self.cV = exact(s.Rk), exact(s.Sk), exact(s.Sv)
        self.mR, self.mS = bitmap(s.vR), bitmap(s.vS)
        cuda.cuda.synchronize()
        assert self.mR.data_ptr() % 4 == 0 and self.mS.data_ptr() % 4 == 0 and self.cR.data_ptr() % 16 == 0


class Env:
    """What the steps share: the library, the oracle, the device inputs (made once per module) and the
    references on the device."""

    def __init__(self, hw, cuda, orc):
        from hwbloomradixjoin_amd import pjoin
        self.hw, self.cuda, self.orc, self.pjoin = hw, cuda, orc, pjoin
        self.L = hw.lib()
        assert self.L.hwbrj_set_device(0) == 0
        self.dev = {n: Dev(cuda, sc.relset(n)) for n in sc.SET_NAMES}
        self.args = {n: (None if c is None else hw.BloomFilterArgs(*c)) for n, c in sc.CONFIGS.items()}
        self.rows_d, self.sub_checked, self.filters = {}, set(), {}
        # every host reference once, here: no chunk pays for it, whichever runs first or alone
        for s in sc.SET_NAMES:
            for f in sc.FAMILY_NAMES:
                sc.expect(orc, f, s)
            for c in sc.CONFIG_NAMES:
                for masked in (False, True):
                    if not (masked and c in sc.UNSLICED):
                        sc.counts(orc, s, c, masked)

    def want_rows(self, family, set_name):
        """The reference rows of (family, set) on the device, sorted as the step's rows will be."""
        key = (family, set_name)
        if key not in self.rows_d:
            rows = sc.expect(self.orc, family, set_name).rows
            t = self.cuda.from_numpy(np.ascontiguousarray(rows).view(np.int64)).to("cuda:0")
            self.rows_d[key] = self.sorted_rows(t)
        return self.rows_d[key]

    def sorted_rows(self, t):
        """Rows as int64 words, sorted: a (n,) tensor of 8-byte rows, or a (n, 2) tensor of 16-byte rows
        (sorted by both words: a stable sort by the second, then by the first)."""
        cuda = self.cuda
        if t.dim() == 1:
            return cuda.sort(t)[0]
        i1 = cuda.sort(t[:, 1], stable=True)[1]
        i0 = cuda.sort(t[i1, 0], stable=True)[1]
        return t[i1[i0]]


@pytest.fixture(scope="module")
def env(hw, cuda, orc):
    return Env(hw, cuda, orc)


@pytest.fixture(autouse=True)
def clean_end(hw):
    """Every test ends with nothing pending and every hook off."""
    yield
    n = ctypes.c_int(0)
    hw.lib().hwbrj_join_wait_all(None, 0, ctypes.byref(n))  # (collects what a failed test left; 6 if nothing was)
    assert n.value == 0, f"{n.value} joins were left pending"
    assert "HOOK" not in hw.version()


def _code(fn):
    """The library's return code of a wrapper call that raises on a nonzero one (0: it returned)."""
    try:
        fn()
    except RuntimeError as e:
        return int(re.search(r"failed \((\d+)\)", str(e)).group(1))
    return 0


def call(env, family, config, set_name, buf, cap, stream=None):
    """One payload entry through the C ABI with d_out = buf (a tensor or None) and `cap` rows:
    (rc, n_out, stats, n_class or None, n_pairs or None)."""
    hw, L, f, d = env.hw, env.L, sc.FAMILY[family], env.dev[set_name]
    a = env.args[config]
    a = a._c() if a is not None else None
    ap = ctypes.byref(a) if a is not None else None
    sp = ctypes.c_void_p(stream.cuda_stream) if stream is not None else None
    n, st, cls, pairs = ctypes.c_uint64(), hw._Stats(), (ctypes.c_uint64 * 3)(), ctypes.c_uint64()
    keys = f.layout == "k"
    R, S = (d.cR, d.cS) if keys else (d.dR, d.dS)
    if f.masked:
        head = (R.data_ptr(), d.mR.data_ptr(), R.shape[0], S.data_ptr(), d.mS.data_ptr(), S.shape[0], ap)
    else:
        head = (R.data_ptr(), R.shape[0], S.data_ptr(), S.shape[0], ap)
    tail = (buf.data_ptr() if buf is not None else None, cap, ctypes.byref(n))
    end = (sp, ctypes.byref(st), None)
    kind = getattr(hw, f.kind) if f.kind else None
    sfx = "_nulls_device" if f.masked else "_device"
    env.cuda.cuda.current_stream().synchronize()  # (the buffer's fill runs on torch's stream)
    if f.op == "pairs":
        rc = getattr(L, "hwbrj_join_keys_pairs" + sfx if keys else "hwbrj_join_materialize_device")(*head, *tail, *end)
    elif f.op == "semi":
        rc = getattr(L, "hwbrj_join_keys_semi" + sfx if keys else "hwbrj_join_semi_device")(*head, kind, *tail, *end)
    elif f.op == "outer":
        if keys:
            rc = getattr(L, "hwbrj_join_keys_outer" + sfx)(*head, kind, *tail, cls, *end)
        else:
            rc = L.hwbrj_join_outer_device(*head, kind, sc.NULL_T, *tail, cls, *end)
    else:
        name = "group_minmax" if f.op == "minmax" else "group"
        if keys:
            rc = getattr(L, f"hwbrj_join_keys_{name}_device")(R.data_ptr(), R.shape[0], S.data_ptr(), d.cV.data_ptr(),
                                                              S.shape[0], ap, kind, *tail, ctypes.byref(pairs), *end)
        else:
            rc = getattr(L, f"hwbrj_join_{name}_device")(*head, kind, *tail, ctypes.byref(pairs), *end)
    return (rc, n.value, st, tuple(cls) if f.op == "outer" else None, pairs.value if f.op in ("group", "minmax") else None)


def out_buffer(env, family, rows):
    """`rows` rows and the guard region behind them, all sentinel."""
    width = 4 if sc.FAMILY[family].op in ("group", "minmax") else 2
    return env.cuda.full((rows + GUARD_ROWS, width), GUARD, dtype=env.cuda.int32, device="cuda:0")


def enqueue(env, step, stream=None):
    """An async counting join, not waited for."""
    family, config, set_name = step
    d = env.dev[set_name]
    if sc.FAMILY[family].layout == "k":
        env.hw.join_keys_device_async(d.cR, d.cS, env.args[config], stream=stream)
    else:
        env.hw.join_device_async(d.dR, d.dS, env.args[config], stream=stream)


def check_counts(env, st, step, label):
    """A counting join's stats against the oracle."""
    family, config, set_name = step
    want = sc.counts(env.orc, set_name, config, sc.FAMILY[family].masked)
    got = (st.matches, st.filtered, st.mode)
    assert got == (want[0], want[1], sc.config_mode(config)), f"{label}: (matches, filtered, mode) {got}, oracle {want}"
    assert want[0] == sc.expect(env.orc, family, set_name).matches


def run_step(env, step, prev, stream=None, pending=()):
    """One step with all its assertions. pending: the un-waited async joins enqueued before it; an async
    step then collects them with join_wait_all and checks every join, oldest first."""
    hw, cuda, orc = env.hw, env.cuda, env.orc
    family, config, set_name = step
    f, d, args = sc.FAMILY[family], env.dev[set_name], env.args[config]
    label = f"step {step} after {prev}"
    assert sc.is_step(family, config)
    if f.op == "part":
        st = env.pjoin.join_partitioned(d.dR, d.dS, d.dR.shape[0], args)
        return check_counts(env, st, step, label)
    if f.op == "count":
        if f.wait:
            enqueue(env, step, stream)
            if pending:
                sts = hw.join_wait_all()
                assert len(sts) == len(pending) + 1, f"{label}: {len(sts)} joins collected"
                for st, p in zip(sts, list(pending) + [step]):
                    check_counts(env, st, p, f"{label} (collected: {p})")
                return None
            st = hw.join_wait()
        elif f.layout == "t":
            st = hw.join_device(d.dR, d.dS, args, stream=stream, algorithm=getattr(hw, f.kind))
        elif f.masked:
            st = hw.join_keys_device(d.cR, d.cS, args, stream=stream, r_valid=d.mR, s_valid=d.mS)
        else:
            st = hw.join_keys_device(d.cR, d.cS, args, stream=stream)
        return check_counts(env, st, step, label)
    exp = sc.expect(orc, family, set_name)
    buf = out_buffer(env, family, exp.n)
    rc, n, st, cls, pairs = call(env, family, config, set_name, buf, exp.n, stream)
    want_f = sc.filtered(orc, set_name, config, f.masked)
    got = (rc, n, st.matches, st.filtered, st.mode, cls, pairs)
    want = (0, exp.n, exp.matches, want_f, sc.config_mode(config), exp.cls, exp.n_pairs)
    assert got == want, f"{label}: (rc, n_out, matches, filtered, mode, n_class, n_pairs) {got}, reference {want}"
    assert bool((buf[exp.n:] == GUARD).all()), f"{label}: the guard region behind the output was written"
    rows = buf[: exp.n].view(cuda.int64)
    rows = rows.ravel() if rows.shape[1] == 1 else rows
    same = cuda.equal(env.sorted_rows(rows), env.want_rows(family, set_name))
    if not same:
        bad = int((env.sorted_rows(rows) != env.want_rows(family, set_name)).sum())
        untouched = int((buf[: exp.n] == GUARD).all(dim=1).sum())
        raise AssertionError(f"{label}: the rows are not the reference's ({bad} of {exp.n} sorted words differ, "
                             f"{untouched} rows never written)")
    return None


def sub_multiset(got, want):
    """Whether every row of `got` occurs in `want` at least as often (rows as bytes)."""
    from collections import Counter
    g, w = Counter(r.tobytes() for r in got), Counter(r.tobytes() for r in want)
    return all(w[k] >= c for k, c in g.items())


def host_rows(exp, width):
    """A reference's rows as (n, width) int32."""
    return np.ascontiguousarray(exp.rows).view(np.int32).reshape(-1, width)


def run_disturber(env, d, dset, i, hook):
    """The disturber of one entry, with its own assertions. Returns the async joins it left un-waited."""
    hw, cuda, orc, L = env.hw, env.cuda, env.orc, env.L
    kind = d[0]
    dev = env.dev[dset]
    label = f"disturber {d} on {dset}"
    if kind == "code7":
        family, config = d[1], d[2]
        exp = sc.expect(orc, family, dset)
        cap = exp.n - 1000
        assert cap > 0
        buf = out_buffer(env, family, cap)
        rc, n, st, cls, pairs = call(env, family, config, dset, buf, cap)
        got, want = (rc, n, st.matches, st.mode, cls, pairs), (7, exp.n, exp.n, sc.config_mode(config), exp.cls, exp.n_pairs)
        assert got == want, f"{label}: (rc, n_out, matches, mode, n_class, n_pairs) {got}, reference {want}"
        assert bool((buf[cap:] == GUARD).all()), f"{label}: written beyond the capacity"
        if (family, config, dset) not in env.sub_checked:  # every row in [0, capacity) is a row of the result
            env.sub_checked.add((family, config, dset))
            assert sub_multiset(buf[:cap].cpu().numpy(), host_rows(exp, buf.shape[1])), f"{label}: rows in [0, capacity)"
    elif kind == "count_only":
        family = sc.PAYLOAD[i % len(sc.PAYLOAD)]
        config = [c for c in ("blocked_packed", "global_b4", "nobloom", "basic_k3") if sc.is_step(family, c)][i % 2]
        exp = sc.expect(orc, family, dset)
        rc, n, st, cls, pairs = call(env, family, config, dset, None, 0)
        got, want = (rc, n, st.matches, cls, pairs), (7, exp.n, exp.n, exp.cls, exp.n_pairs)
        assert got == want, f"{label} ({family}, {config}): (rc, n_out, matches, n_class, n_pairs) {got}, reference {want}"
    elif kind == "refused9":
        config = d[2]
        if d[1] == "part":
            rc = _code(lambda: env.pjoin.join_partitioned(dev.dR, dev.dS, dev.dR.shape[0], env.args[config]))
        else:
            family = sc.MASKED[i % len(sc.MASKED)]
            if sc.FAMILY[family].op == "count":
                rc = _code(lambda: hw.join_keys_device(dev.cR, dev.cS, env.args[config], r_valid=dev.mR, s_valid=dev.mS))
            else:
                rc = call(env, family, config, dset, None, 0)[0]
        assert rc == 9, f"{label}: code {rc}"
    elif kind == "m_not_pow2":
        bad = hw.BloomFilterArgs(hw.BLOCKED, 3 << 20, 1, 1024)
        fn = (lambda: hw.join_device(dev.dR, dev.dS, bad)) if i % 2 else (lambda: hw.join_keys_device(dev.cR, dev.cS, bad))
        assert _code(fn) == 2, label
    elif kind == "misaligned":
        st = hw._Stats()
        rc = L.hwbrj_join_keys_device(dev.cR.data_ptr() + 4, dev.cR.shape[0] - 1, dev.cS.data_ptr(), dev.cS.shape[0], None, 0,
                                      None, ctypes.byref(st))
        assert rc == 2 and b"align" in L.hwbrj_last_error(), f"{label}: code {rc}"
    elif kind == "unwaited":
        left = []
        for j in range(d[1]):
            step = (("count_t_async", "count_k_async")[(i + j) % 2], ("blocked_packed", "nobloom", "basic_k1")[(i + j) % 3], dset)
            enqueue(env, step)
            left.append(step)
        return left
    elif kind == "release":
        L.hwbrj_release()
    elif kind == "export_filter":
        run_step(env, ("count_t", "blocked_packed", dset), label)
        c = sc.CONFIGS["blocked_packed"]
        if dset not in env.filters:
            env.filters[dset] = orc.bloom_bitmap(sc.relset(dset).Rk, *c)[0]
        assert np.array_equal(hw.export_filter(c[1]), env.filters[dset]), f"{label}: the exported filter"
    elif kind == "tables_read":
        run_step(env, ("count_k", ("nobloom", "blocked_packed")[i % 2], dset), label)
        info = hw.tables_info()
        assert hw.tables_read(hw.TAB_R_ELEM_START)[-1] == dev.cR.shape[0] and info["jobs"] == info["F"] * info["NSUB"], label
        hw.tables_read(hw.TAB_NPARTS)
    elif kind == "join_split":
        hook(hw.HOOK_JOIN_SPLIT, 700)
        run_step(env, ("count_t", "blocked_f64", dset), label)  # (set B: about 4,000 survivors per job)
        assert hw.tables_info()["split"] == 700 and hw.tables_read(hw.TAB_NPARTS)[:-1].max() > 1, label
        hook(hw.HOOK_JOIN_SPLIT, 0)
    elif kind == "caller_stream":
        s1 = cuda.cuda.Stream()
        run_step(env, (("count_t", "pairs_t", "count_k")[i % 3], "blocked_packed", dset), label, stream=s1)
    else:
        raise AssertionError(f"unknown disturber {d}")
    return []


@pytest.mark.parametrize("i", range(len(SCHEDULE)))
def test_schedule_chunk(env, i):
    """About 25 entries of the schedule; chunk i > 0 first repeats chunk i - 1's last step."""
    prev = None
    for step in SCHEDULE[i]:
        run_step(env, step, prev)
        prev = step


@pytest.mark.parametrize("i", range(len(DISTURBERS)))
def test_disturbers_chunk(env, hook, i):
    """About 25 entries of the disturber schedule: the disturber, then its follower on the library's own
    stream. A synchronous follower of un-waited async joins is checked alone (it consumes them); an async
    follower is collected with join_wait_all and every returned join is checked."""
    for d, dset, step, n in DISTURBERS[i]:
        left = run_disturber(env, d, dset, n, hook)
        run_step(env, step, f"disturber {d} on {dset}", pending=left if sc.FAMILY[step[0]].wait else ())


def test_job_table_changes_are_covered(env):
    """job_surv is cleared only when NJ = F x NSUB changes: consecutive synchronous tuple counting joins
    see NJ rise, fall, and stay equal with the set changed (a stale job table of another set's join)."""
    walk = [("blocked_f64", "A"), ("blocked_f64", "C"), ("basic_f32", "B"), ("blocked_f64", "A"), ("basic_f32", "C"),
            ("blocked_f64", "C"), ("nobloom", "B"), ("blocked_packed", "A"), ("basic_f32", "A"), ("blocked_f64", "B")]
    seen, prev, last = set(), None, None
    for config, s in walk:
        step = ("count_t", config, s)
        run_step(env, step, prev)
        info = env.hw.tables_info()
        nj = info["F"] * info["NSUB"]
        print(f"{step}: F {info['F']} NSUB {info['NSUB']} NJ {nj}")
        if last is not None:
            seen.add("rise" if nj > last[0] else "fall" if nj < last[0] else "equal, set changed" if s != last[1] else "same")
        prev, last = step, (nj, s)
    assert {"rise", "fall", "equal, set changed"} <= seen, seen


def test_ring_slots_dirtied_by_payload_joins(env):
    """64 outer and group joins on set A write words 6-7 of their ring slots (the class and pair
    counters); 130 un-waited async counting joins then take every slot twice: each join's counts are
    its own oracle counts, in order (an enqueue that finds the ring full collects it on the way)."""
    prev = None
    for j in range(64):
        step = (("full_t", "gsum_k", "outer_s_k", "gminmax_t", "outer_r_t", "gsum_t", "full_km", "gminmax_k")[j % 8],
                ("blocked_packed", "nobloom", "basic_k1")[j % 3], "A")
        run_step(env, step, prev)
        prev = step
    steps = [(("count_t_async", "count_k_async")[j % 2], ("blocked_packed", "nobloom", "basic_k1")[(j // 2) % 3], "A")
             for j in range(130)]
    for step in steps:
        enqueue(env, step)
    sts = env.hw.join_wait_all(capacity=256)
    assert len(sts) == len(steps)
    for j, (st, step) in enumerate(zip(sts, steps)):
        check_counts(env, st, step, f"async join {j} {step}")
