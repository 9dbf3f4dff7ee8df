"""Every join entry after every other on one engine (seq_catalog.py): the engine's buffers only grow and
are never cleared wholesale, so each join relies on what its predecessor left behind. The schedule runs
every (family, config, set) step and every ordered pair of families, configs and sets; the disturber
schedule puts a refusal, a capacity overflow, un-waited async joins, hwbrj_release, a readback, a hook
or another stream in front of every family.

Every step asserts its return code, stats.matches, stats.filtered (the oracle's), stats.mode, the exact
row multiset, n_class / n_pairs and an untouched guard region behind its output buffer, each against
the host references of seq_catalog.py. Row multisets are compared on the device as sorted 64-bit views
of the rows (the group joins' 16-byte rows as two such views, sorted by both). A failure names the step
and its predecessor.

A probe family's step is a probe of a prepared build of its (set, config, purpose, masked): made on
first use, right behind whatever step preceded it, and kept in Env's cache (seq_catalog.BuildCache),
so builds live through many other joins, hwbrj_release and un-waited async joins, and freed ones are
made again. A probe asserts what its one-shot counterpart's step asserts, and that it ran no R phase.
A streamed family's step is reset_marks, a marking probe per batch of S and the unmatched R rows, all
into one guarded buffer: together the one-shot outer join's rows and class counts."""
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
    columns, S's value column (cV; cVn: with the extremes under its NULLs) and the packed validity
    bitmaps (ceil(n / 32) * 4 bytes; mV: of S's values)."""

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
        self.cVn, self.mV = exact(s.Svn), bitmap(s.vV)
        cuda.cuda.synchronize()
        assert self.mR.data_ptr() % 4 == 0 and self.mS.data_ptr() % 4 == 0 and self.cR.data_ptr() % 16 == 0
        assert self.mV.data_ptr() % 4 == 0 and self.cS.data_ptr() % 16 == 0 and self.cVn.data_ptr() % 16 == 0


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
        self.rows_d, self.sub_checked, self.filters, self.r_only = {}, set(), {}, {}
        self.builds = sc.BuildCache(self.make_build, lambda b: b.free())
        # every host reference once, here: no chunk pays for it, whichever runs first or alone
        for s in sc.SET_NAMES:
            for f in sc.FAMILY_NAMES:
                sc.expect(orc, f, s)
            for c in sc.CONFIG_NAMES:
                for masked in (False, True, "values"):
                    if not (masked and c in sc.UNSLICED):
                        sc.counts(orc, s, c, masked)

    def make_build(self, key):
        """A prepared build of key = (set, config, purpose, masked)."""
        set_name, config, purpose, masked = key
        d = self.dev[set_name]
        b = self.hw.build_keys_device(d.cR, self.args[config], getattr(self.hw, purpose), r_valid=d.mR if masked else None)
        info = b.info()
        assert (info["nR"], info["purpose"], info["masked"]) == (d.cR.shape[0], getattr(self.hw, purpose), int(masked)), key
        return b

    def build_for(self, family, config, set_name):
        """The cached build of a probe step (made now if it is not alive)."""
        return self.builds.get(sc.build_key(family, config, set_name))

    def print_builds(self):
        live = self.builds.live()
        print(f"live builds: {len(live)} ({self.builds.made} made so far), {sum(b.info()['bytes'] for b in live)} bytes")

    def want_rows(self, family, set_name):
        """The reference rows of (family, set) on the device, sorted as the step's rows will be."""
        key = (sc.ref_of(family), sc.mask_kind(family), set_name)
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
    e = Env(hw, cuda, orc)
    yield e
    e.builds.clear()  # every build freed with the module


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


PROBE_ENTRY = {"pairs": "pairs", "semi": "semi", "outer": "outer", "group": "group", "minmax": "group_minmax"}


def probe_call(env, family, config, set_name, buf, cap, stream=None, build=None, batch=None):
    """call() for a probe family: the hwbrj_probe_keys_* entry of its op on `build` (default: the cached
    build of the step) and rows [a, b) of S (batch; default: all), as views of the set's columns: the
    bitmap pointers advance by a / 8 bytes (a is a multiple of 32)."""
    hw, L, f, d = env.hw, env.L, sc.FAMILY[family], env.dev[set_name]
    b = build if build is not None else env.build_for(family, config, set_name)
    lo, hi = batch if batch is not None else (0, d.cS.shape[0])
    assert lo % 32 == 0 and 0 <= lo <= hi <= d.cS.shape[0]
    sp = ctypes.c_void_p(stream.cuda_stream) if stream is not None else None
    n, st, cls, pairs = ctypes.c_uint64(), hw._Stats(), (ctypes.c_uint64 * 3)(), ctypes.c_uint64()
    group = f.op in ("group", "minmax")
    head = (b._handle(), d.cS.data_ptr() + 4 * lo, d.mS.data_ptr() + lo // 8 if f.masked else None)
    if group:
        head += (d.cVn.data_ptr() + 4 * lo, d.mV.data_ptr() + lo // 8)
    head += (hi - lo,) + ((getattr(hw, f.kind),) if f.kind else ())
    tail = (buf.data_ptr() if buf is not None else None, cap, ctypes.byref(n))
    extra = (cls,) if f.op == "outer" else (ctypes.byref(pairs),) if group else ()
    env.cuda.cuda.current_stream().synchronize()  # (the buffer's fill runs on torch's stream)
    rc = getattr(L, f"hwbrj_probe_keys_{PROBE_ENTRY[f.op]}_device")(*head, *tail, *extra, sp, ctypes.byref(st), None)
    return (rc, n.value, st, tuple(cls) if f.op == "outer" else None, pairs.value if group else None)


def no_r_phase(st, label):
    """A probe's stats show no R phase (they are hwbrj_stats_t's)."""
    got = (st.ms_r_scatter, st.ms_r_index, st.ms_build)
    assert got == (0, 0, 0) and st.ms_total > 0, f"{label}: (ms_r_scatter, ms_r_index, ms_build) {got}, ms_total {st.ms_total}"


def call(env, family, config, set_name, buf, cap, stream=None, build=None, batch=None):
    """One payload entry through the C ABI with d_out = buf (a tensor or None) and `cap` rows:
    (rc, n_out, stats, n_class or None, n_pairs or None). build, batch: probe_call's."""
    hw, L, f, d = env.hw, env.L, sc.FAMILY[family], env.dev[set_name]
    if f.layout == "p":
        return probe_call(env, family, config, set_name, buf, cap, stream, build, batch)
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
        if f.masked:
            rc = getattr(L, f"hwbrj_join_keys_{name}_nulls_device")(R.data_ptr(), d.mR.data_ptr(), R.shape[0], S.data_ptr(),
                                                                    d.mS.data_ptr(), d.cVn.data_ptr(), d.mV.data_ptr(),
                                                                    S.shape[0], ap, kind, *tail, ctypes.byref(pairs), *end)
        elif keys:
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


def r_only_rows(env, family, set_name):
    """The sorted R rows of the reference's R-only rows {R row, -1} (key columns)."""
    key = (sc.ref_of(family), sc.mask_kind(family), set_name)
    if key not in env.r_only:
        rows = host_rows(sc.expect(env.orc, family, set_name), 2)
        env.r_only[key] = np.sort(rows[rows[:, 1] == sc.NULL_K, 0])
    return env.r_only[key]


def unmatched(env, b, buf, cap, stream=None):
    """(rc, n_out) of hwbrj_build_unmatched_device into buf (a tensor or None)."""
    n = ctypes.c_uint64()
    sp = ctypes.c_void_p(stream.cuda_stream) if stream is not None else None
    env.cuda.cuda.current_stream().synchronize()
    rc = env.L.hwbrj_build_unmatched_device(b._handle(), buf.data_ptr() if buf is not None else None, cap, ctypes.byref(n), sp,
                                            None)
    return rc, n.value


def check_marks(env, b, family, set_name, label):
    """The build's marks are those of a marking probe of the whole S: the unmatched rows are the
    reference's R-only rows (count only, then the rows)."""
    want = r_only_rows(env, family, set_name)
    assert want.size == sc.expect(env.orc, family, set_name).cls[2] > 0
    assert unmatched(env, b, None, 0) == (7, want.size), f"{label}: the unmatched count"
    buf = out_buffer(env, family, want.size)
    assert unmatched(env, b, buf, want.size) == (0, want.size), f"{label}: the unmatched rows"
    got = buf.cpu().numpy()
    assert (got[want.size:] == np.int32(GUARD)).all() and (got[: want.size, 1] == sc.NULL_K).all(), label
    assert np.array_equal(np.sort(got[: want.size, 0]), want), f"{label}: the marks are not the reference's"


def run_stream(env, step, prev, stream=None, build=None):
    """A streamed outer join: reset_marks, a marking probe per batch of S, each behind its predecessor
    in one guarded buffer with the rows left as capacity, then the unmatched R rows behind them. The
    union is the one-shot join's multiset (the batch's start added to its S rows), the summed n_class
    with the unmatched count as class 2 its n_class, the summed `filtered` the whole set's (the filter
    is R's alone)."""
    cuda, orc = env.cuda, env.orc
    family, config, set_name = step
    label = f"step {step} after {prev}"
    exp = sc.expect(orc, family, set_name)
    b = build if build is not None else env.build_for(family, config, set_name)
    assert env.L.hwbrj_build_reset_marks(b._handle()) == 0, label
    buf = out_buffer(env, family, exp.n)
    off, cls_sum, filt = 0, [0, 0, 0], 0
    for lo, hi in sc.batches(env.dev[set_name].cS.shape[0]):
        rc, n, st, cls, _ = call(env, family, config, set_name, buf[off:], exp.n - off, stream, b, (lo, hi))
        got, want = (rc, st.matches, st.mode, cls[2], n <= exp.n - off), (0, n, sc.config_mode(config), 0, True)
        assert got == want and n == cls[0] + cls[1], f"{label}, batch [{lo}, {hi}): (rc, matches, mode, class 2, fits) {got}, " \
                                                   f"expected {want}; n_out {n}, n_class {cls}"
        no_r_phase(st, label)
        if stream is not None:
            stream.synchronize()
        buf[off: off + n, 1] += lo
        off, filt = off + n, filt + st.filtered
        cls_sum = [x + y for x, y in zip(cls_sum, cls)]
    rc, n = unmatched(env, b, buf[off:], exp.n - off, stream)
    cls_sum[2] = n
    got = (rc, off + n, tuple(cls_sum), filt)
    want = (0, exp.n, exp.cls, sc.filtered(orc, set_name, config, sc.mask_kind(family)))
    assert got == want, f"{label}: (rc of unmatched, rows, n_class, filtered) {got}, reference {want}"
    assert unmatched(env, b, None, 0) == (7 if n else 0, n), f"{label}: the second unmatched count"
    if stream is not None:
        stream.synchronize()
    assert bool((buf[exp.n:] == GUARD).all()), f"{label}: the guard region behind the output was written"
    rows = buf[: exp.n].view(cuda.int64).ravel()
    if not cuda.equal(env.sorted_rows(rows), env.want_rows(family, set_name)):
        bad = int((env.sorted_rows(rows) != env.want_rows(family, set_name)).sum())
        raise AssertionError(f"{label}: the rows are not the reference's ({bad} of {exp.n} sorted words differ)")


def run_step(env, step, prev, stream=None, pending=(), build=None):
    """One step with all its assertions. pending: the un-waited async joins enqueued before it; an async
    step then collects them with join_wait_all and checks every join, oldest first. build: a probe
    family's build, where it is not the cached one."""
    hw, cuda, orc = env.hw, env.cuda, env.orc
    family, config, set_name = step
    f, d, args = sc.FAMILY[family], env.dev[set_name], env.args[config]
    label = f"step {step} after {prev}"
    assert sc.is_step(family, config)
    if family in sc.STREAMED:
        return run_stream(env, step, prev, stream, build)
    if f.op == "part":
        st = env.pjoin.join_partitioned(d.dR, d.dS, d.dR.shape[0], args)
        return check_counts(env, st, step, label)
    if f.op == "count" and f.layout == "p":
        b = build if build is not None else env.build_for(family, config, set_name)
        st = hw._Stats()
        sp = ctypes.c_void_p(stream.cuda_stream) if stream is not None else None
        rc = env.L.hwbrj_probe_keys_device(b._handle(), d.cS.data_ptr(), d.mS.data_ptr(), d.cS.shape[0], getattr(hw, f.kind), sp,
                                           ctypes.byref(st))
        assert rc == 0, f"{label}: code {rc}"
        no_r_phase(st, label)
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
    rc, n, st, cls, pairs = call(env, family, config, set_name, buf, exp.n, stream, build)
    want_f = sc.filtered(orc, set_name, config, sc.mask_kind(family))
    got = (rc, n, st.matches, st.filtered, st.mode, cls, pairs)
    want = (0, exp.n, exp.matches, want_f, sc.config_mode(config), exp.cls, exp.n_pairs)
    assert got == want, f"{label}: (rc, n_out, matches, filtered, mode, n_class, n_pairs) {got}, reference {want}"
    if f.layout == "p":
        no_r_phase(st, label)
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


ROWS_PROBES = tuple(f for f in sc.PROBES if f != "count_p" and sc.FAMILY[f].masked)  # what a masked rows build is probed with


def whole_probe(exp, family):
    """(n_out, n_class) of one call on the whole S: the reference's, but for a streamed family's marking
    probe, which writes no R-only row (they are left to the marks)."""
    if family in sc.STREAMED:
        return exp.cls[0] + exp.cls[1], (exp.cls[0], exp.cls[1], 0)
    return exp.n, exp.cls


def run_disturber(env, d, dset, i, hook):
    """The disturber of one entry, with its own assertions. Returns the async joins it left un-waited,
    and what it has to do behind the follower (a function, or None)."""
    hw, cuda, orc, L = env.hw, env.cuda, env.orc, env.L
    kind = d[0]
    dev = env.dev[dset]
    label = f"disturber {d} on {dset}"
    if kind == "code7":
        # (a probe that overflows leaves its cached build to the later steps; a marking probe's marks
        # are those of a probe at full capacity)
        family, config = d[1], d[2]
        exp = sc.expect(orc, family, dset)
        n_all, cls_all = whole_probe(exp, family)
        cap = n_all - 1000
        assert cap > 0
        if family in sc.STREAMED:
            assert L.hwbrj_build_reset_marks(env.build_for(family, config, dset)._handle()) == 0
        buf = out_buffer(env, family, cap)
        rc, n, st, cls, pairs = call(env, family, config, dset, buf, cap)
        got, want = (rc, n, st.matches, st.mode, cls, pairs), (7, n_all, n_all, sc.config_mode(config), cls_all, exp.n_pairs)
        assert got == want, f"{label}: (rc, n_out, matches, mode, n_class, n_pairs) {got}, reference {want}"
        assert bool((buf[cap:] == GUARD).all()), f"{label}: written beyond the capacity"
        if (family, config, dset) not in env.sub_checked:  # every row in [0, capacity) is a row of the result
            env.sub_checked.add((family, config, dset))
            assert sub_multiset(buf[:cap].cpu().numpy(), host_rows(exp, buf.shape[1])), f"{label}: rows in [0, capacity)"
        if family in sc.STREAMED:
            check_marks(env, env.build_for(family, config, dset), family, dset, label)
    elif kind == "count_only":
        family = sc.PAYLOAD[i % len(sc.PAYLOAD)]
        config = [c for c in ("blocked_packed", "global_b4", "nobloom", "basic_k3") if sc.is_step(family, c)][i % 2]
        exp = sc.expect(orc, family, dset)
        n_all, cls_all = whole_probe(exp, family)
        if family in sc.STREAMED:
            assert L.hwbrj_build_reset_marks(env.build_for(family, config, dset)._handle()) == 0
        rc, n, st, cls, pairs = call(env, family, config, dset, None, 0)
        got, want = (rc, n, st.matches, cls, pairs), (7, n_all, n_all, cls_all, exp.n_pairs)
        assert got == want, f"{label} ({family}, {config}): (rc, n_out, matches, n_class, n_pairs) {got}, reference {want}"
        if family in sc.STREAMED:
            check_marks(env, env.build_for(family, config, dset), family, dset, f"{label} ({family}, {config})")
    elif kind in ("build", "build_free"):
        purpose = d[1] or ("BUILD_COUNT", "BUILD_ROWS")[i % 2]
        config = sc.SLICED[i % len(sc.SLICED)]
        family = "count_p" if purpose == "BUILD_COUNT" else ROWS_PROBES[i % len(ROWS_PROBES)]
        b = env.make_build((dset, config, purpose, True))

        def probe_and_free(where):
            run_step(env, (family, config, dset), f"{label}, {where}", build=b)
            b.free()
        if kind == "build":  # kept across the follower, probed behind it
            return [], lambda: probe_and_free("behind its follower")
        probe_and_free("made, probed and freed")
    elif kind == "unmatched7":
        family, config = "stream_r_p", sc.SLICED[i % len(sc.SLICED)]
        exp, b = sc.expect(orc, family, dset), env.build_for("stream_r_p", config, dset)
        assert L.hwbrj_build_reset_marks(b._handle()) == 0
        n_all, cls_all = whole_probe(exp, family)
        buf = out_buffer(env, family, n_all)
        rc, n, st, cls, _ = call(env, family, config, dset, buf, n_all)
        assert (rc, n, cls) == (0, n_all, cls_all) and bool((buf[n_all:] == GUARD).all()), f"{label}: {(rc, n, cls)}"
        n_un = exp.cls[2]
        cap = n_un - 1000
        assert cap > 0
        buf = out_buffer(env, family, cap)
        assert unmatched(env, b, buf, cap) == (7, n_un), f"{label}: (rc, n_out) of the unmatched rows"
        got = buf.cpu().numpy()
        assert (got[cap:] == np.int32(GUARD)).all(), f"{label}: written beyond the capacity"
        assert (got[:cap, 1] == sc.NULL_K).all() and np.unique(got[:cap, 0]).size == cap, label
        assert np.isin(got[:cap, 0], r_only_rows(env, family, dset)).all(), f"{label}: rows in [0, capacity)"
    elif kind == "refused9" and d[1] == "build":
        a = env.args[d[2]]._c()
        h = ctypes.c_void_p(0xDEAD)
        rc = L.hwbrj_build_keys_device(dev.cR.data_ptr(), dev.mR.data_ptr() if i % 4 < 2 else None, dev.cR.shape[0],
                                       ctypes.byref(a), (hw.BUILD_COUNT, hw.BUILD_ROWS)[i % 2], None, ctypes.byref(h), None)
        assert (rc, h.value) == (9, 0xDEAD), f"{label}: code {rc}, *build {h.value}"
    elif kind == "refused9":
        config = d[2]
        if d[1] == "part":
            rc = _code(lambda: env.pjoin.join_partitioned(dev.dR, dev.dS, dev.dR.shape[0], env.args[config]))
        else:
            one_shot = [f for f in sc.MASKED if f not in sc.PROBES]  # (a build under these configs: ("refused9", "build", c))
            family = one_shot[i % len(one_shot)]
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
        return left, None
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
        run_step(env, (("count_t", "pairs_t", "count_k", "pairs_p")[i % 4], "blocked_packed", dset), label, stream=s1)
    else:
        raise AssertionError(f"unknown disturber {d}")
    return [], None


@pytest.mark.parametrize("i", range(len(SCHEDULE)))
def test_schedule_chunk(env, i):
    """About 25 entries of the schedule; chunk i > 0 first repeats chunk i - 1's last step."""
    prev = None
    for step in SCHEDULE[i]:
        run_step(env, step, prev)
        prev = step
    env.print_builds()


def filters_after_a_probe(env, step, label):
    """After a probe the engine has no filter to export (5) while the build's own is still the oracle's
    filter of R's valid keys (two_segments: 256 MiB, left out)."""
    hw, (family, config, set_name) = env.hw, step
    c = sc.CONFIGS[config]
    m = c[1] if c is not None else 1 << 24
    if m > 1 << 24:
        return
    assert _code(lambda: hw.export_filter(m)) == 5, f"{label}: the engine's filter after a probe"
    b = env.build_for(family, config, set_name)
    if c is None:
        assert _code(lambda: b.export_filter(m)) == 5, f"{label}: a build without a filter"
        return
    key = (set_name, config, sc.FAMILY[family].masked)
    if key not in env.filters:
        s = sc.relset(set_name)
        env.filters[key] = env.orc.bloom_bitmap(s.Rk[s.vR] if key[2] else s.Rk, *c)[0]
    assert np.array_equal(b.export_filter(m), env.filters[key]), f"{label}: the build's filter"


@pytest.mark.parametrize("i", range(len(DISTURBERS)))
def test_disturbers_chunk(env, hook, i):
    """About 25 entries of the disturber schedule: the disturber, then its follower on the library's own
    stream. A synchronous follower of un-waited async joins is checked alone (it consumes them); an async
    follower is collected with join_wait_all and every returned join is checked. A `build` disturber's
    build is probed behind the follower; behind a probe follower of `export_filter`, the filters."""
    for d, dset, step, n in DISTURBERS[i]:
        left, after = run_disturber(env, d, dset, n, hook)
        label = f"disturber {d} on {dset}"
        run_step(env, step, label, pending=left if sc.FAMILY[step[0]].wait else ())
        if after is not None:
            after()
        if d[0] == "export_filter" and step[0] in sc.PROBES:
            filters_after_a_probe(env, step, f"step {step} after {label}")
    env.print_builds()


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
    """66 outer and group joins on set A, probes of prepared builds among them (their S scatter zeroes
    the slot), write words 6-7 of their ring slots (the class and pair counters); 130 un-waited async
    counting joins then take every slot twice: each join's counts are its own oracle counts, in order
    (an enqueue that finds the ring full collects it on the way)."""
    prev = None
    dirty = ("full_t", "gsum_k", "outer_s_k", "gminmax_t", "outer_r_t", "gsum_t", "full_km", "gminmax_k", "full_p", "gsum_p",
             "gminmax_km")
    for j in range(6 * len(dirty)):
        step = (dirty[j % len(dirty)], ("blocked_packed", "nobloom", "basic_k1")[j % 3], "A")
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
