"""Dev: time the outer joins at the north-star shape (|R| = 128M, |S| = 1024M, q = 0.01, blocked,
m = 2^30, k = 1) against their yardsticks, in one process, alternating after a warm-up:

  join_materialize_device, semi_join_device, semi_join_device(anti=True),
  outer_join_device of OUTER_S, OUTER_R and OUTER_FULL; then one run of each outer kind with args=None.

Prints every run and writes medians, min-max, the phase table, the bytes the shapes move and the
measured copy rate to the file given as argv[1] (default profiles/outer_join/northstar.txt); argv[2] =
repetitions (default 7, at least 7). Times are the calls' own device times (events around the
pipeline). The class counts are asserted: R is a primary key, so there are the north star's
10,240,000 inner rows, the other 1,013,760,000 S rows are S-only, and the R-only rows are the
128,000,000 R rows minus the distinct matched R keys, which a semi-join of R against S (arguments
swapped) counts."""
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import hwbloomradixjoin_amd as hw  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "outer_join", "northstar.txt")
reps = max(7, int(sys.argv[2])) if len(sys.argv) > 2 else 7
nR, nS, q = 128000000, 1024000000, 0.01
N_INNER, N_S_ONLY, FILTERED = 10240000, 1013760000, 124236515
dR = torch.empty((nR, 2), dtype=torch.int32, device="cuda")
dS = torch.empty((nS, 2), dtype=torch.int32, device="cuda")
hw.generate_device(dR, 2, nR, nR, 1.0, 12345)
hw.generate_device(dS, 2, 2**31 - 1, nR, q, 54321)
args = hw.BloomFilterArgs(hw.BLOCKED, 1 << 30, 1, 1024)
NULL = -2**31

# the distinct matched R keys: the R rows that have a partner in S (count-only semi-join, swapped)
n = ctypes.c_uint64()
rc = hw.lib().hwbrj_join_semi_device(dS.data_ptr(), nS, dR.data_ptr(), nR, None, hw.JOIN_SEMI, None, 0,
                                     ctypes.byref(n), None, None, None)
assert rc in (0, 7), (rc, hw.lib().hwbrj_last_error())
N_R_ONLY = nR - n.value
seen = torch.zeros(nR + 1, dtype=torch.bool, device="cuda")  # (cross-check: R's keys are 1 .. |R|)
sk = dS[:, 0]
seen[sk[(sk >= 1) & (sk <= nR)].long()] = True
assert int(seen.sum()) == n.value, (int(seen.sum()), n.value)
del seen, sk
print(f"matched R keys {n.value}, R-only rows {N_R_ONLY}", flush=True)
WANT = {hw.OUTER_S: (N_INNER, N_S_ONLY, 0), hw.OUTER_R: (N_INNER, 0, N_R_ONLY),
        hw.OUTER_FULL: (N_INNER, N_S_ONLY, N_R_ONLY)}
torch.cuda.empty_cache()


def mat():
    st, pairs, ms = hw.join_materialize_device(dR, dS, args, capacity=N_INNER)
    assert (st.filtered, pairs.shape[0]) == (FILTERED, N_INNER), (st.filtered, pairs.shape[0])
    return ms, st


def semi(anti):
    want = N_S_ONLY if anti else N_INNER
    st, rows, ms = hw.semi_join_device(dR, dS, args, anti=anti, capacity=want)
    assert (st.matches, rows.shape[0]) == (want, want), (st.matches, rows.shape[0])
    return ms, st


def outer(a, kind):
    want = WANT[kind]
    st, rows, cls, ms = hw.outer_join_device(dR, dS, a, kind=kind, null_payload=NULL, capacity=sum(want))
    assert cls == want, (cls, want)
    assert (st.matches, rows.shape[0]) == (sum(want), sum(want)), (st.matches, rows.shape[0])
    assert st.filtered == (FILTERED if a is not None else nS), st.filtered
    return ms, st


def bytes_moved(kind, filtered):
    """HBM bytes of a pipeline from the shapes (4-byte words, 8-byte tuples; F3 of DESIGN.md's traffic
    model). Common to every payload pipeline: the S scatter reads the tuples and writes words +
    payloads, the probe reads the words and writes the survivors' codes + positions, the R side reads
    R, writes and re-reads its words, and writes the join's codes, the join reads those and the
    survivors. The materializing pipeline and the outer joins add R's payloads (scatter, build, join);
    the rows are 8 bytes each; S-preserving kinds clear and read the marks (one bit per S position) and
    read the payloads again in the emission; ANTI's emission also reads the words."""
    common = (8 * nS + 8 * nS) + (4 * nS + 8 * filtered) + (8 * nR + 4 * nR + 4 * nR + 4 * nR) + (4 * nR + 8 * filtered)
    rpay = 4 * nR + 4 * nR + 4 * nR + 4 * nR
    marks = 2 * (nS // 8)
    return {"materialize": common + rpay + 8 * N_INNER,
            "anti": common + marks + 8 * nS + 8 * N_S_ONLY,
            "outer_s": common + rpay + marks + 4 * nS + 8 * (N_INNER + N_S_ONLY),
            "outer_r": common + rpay + 8 * (N_INNER + N_R_ONLY),
            "outer_full": common + rpay + marks + 4 * nS + 8 * (N_INNER + N_S_ONLY + N_R_ONLY)}[kind]


cases = [("materialize", mat), ("semi", lambda: semi(False)), ("anti", lambda: semi(True)),
         ("outer_s", lambda: outer(args, hw.OUTER_S)), ("outer_r", lambda: outer(args, hw.OUTER_R)),
         ("outer_full", lambda: outer(args, hw.OUTER_FULL))]
for name, fn in cases:  # warm-up: code objects, buffers, clocks
    ms, _ = fn()
    print(f"warm-up {name}: {ms:.3f} ms", flush=True)
times = {name: [] for name, _ in cases}
joins = {name: [] for name, _ in cases}  # the join phase of every run
phases = {}
for r in range(reps):
    for name, fn in cases:
        ms, st = fn()
        times[name].append(ms)
        joins[name].append(st.ms_join)
        phases[name] = st
        print(f"rep {r} {name}: {ms:.3f} ms", flush=True)
nofilter = {}
for name, kind in (("outer_s", hw.OUTER_S), ("outer_r", hw.OUTER_R), ("outer_full", hw.OUTER_FULL)):
    outer(None, kind)  # (warm-up of the no-filter geometry's buffers)
    nofilter[name], _ = outer(None, kind)
    print(f"no filter {name}: {nofilter[name]:.3f} ms", flush=True)
copy = hw.copy_bandwidth()
med = {k: statistics.median(v) for k, v in times.items()}
spread = {k: max(v) - min(v) for k, v in times.items()}
lines = [f"outer joins at the north star: |R| = {nR}, |S| = {nS}, q = {q}, blocked m = 2^30 k = 1 B = 1024",
         f"{hw.lib().hwbrj_version().decode()}", f"{reps} alternating repetitions after one warm-up each; device ms",
         f"rows asserted: inner {N_INNER}, S-only {N_S_ONLY}, R-only {N_R_ONLY} (distinct matched R keys {n.value})",
         f"{'case':14s} {'median':>9s} {'min':>9s} {'max':>9s} {'GB moved':>9s} {'GB/s':>7s}"]
for name, _ in cases:
    t = times[name]
    gb = bytes_moved(name, FILTERED) / 1e9 if name != "semi" else float("nan")
    lines.append(f"{name:14s} {med[name]:9.3f} {min(t):9.3f} {max(t):9.3f} {gb:9.2f} {gb / med[name] * 1e3:7.0f}")
lines.append(f"{'join phase':14s} {'median':>9s} {'min':>9s} {'max':>9s}")
for name, _ in cases:
    j = joins[name]
    lines.append(f"{name:14s} {statistics.median(j):9.3f} {min(j):9.3f} {max(j):9.3f}")
for name, ms in nofilter.items():
    lines.append(f"{name + ' no filter':22s} {ms:9.3f} (one run after one warm-up)")
for name, _ in cases:
    st = phases[name]
    lines.append(f"phases (last run) {name}: r_sc {st.ms_r_scatter:.3f} r_ix {st.ms_r_index:.3f} build {st.ms_build:.3f} "
                 f"s_sc {st.ms_s_scatter:.3f} s_ix {st.ms_s_index:.3f} probe {st.ms_probe:.3f} join {st.ms_join:.3f}")
bound = med["materialize"] + med["anti"] - med["semi"]
margin = spread["materialize"] + spread["anti"] + spread["semi"]
lines.append(f"OUTER_S yardstick: median {med['outer_s']:.3f} ms <= materialize {med['materialize']:.3f} + anti "
             f"{med['anti']:.3f} - semi {med['semi']:.3f} = {bound:.3f} ms (margin: the three spreads, {margin:.3f} ms): "
             f"{'met' if med['outer_s'] <= bound + margin else 'NOT met'}")
excess = med["outer_r"] - med["materialize"]
lines.append(f"OUTER_R: {excess:.3f} ms over materialize for {N_R_ONLY} R-only rows ({8 * N_R_ONLY / 1e9:.2f} GB): "
             f"{8 * N_R_ONLY / excess / 1e6 if excess > 0 else float('inf'):.0f} GB/s for the added bytes")
lines.append(f"copy_measured {copy:.0f} GB/s")
text = "\n".join(lines) + "\n"
print(text)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
