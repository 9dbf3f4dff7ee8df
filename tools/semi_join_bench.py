"""Dev: time the existence joins at the north-star shape (|R| = 128M, |S| = 1024M, q = 0.01, blocked,
m = 2^30, k = 1) against the materializing join, in one process, alternating after a warm-up:

  join_materialize_device (the yardstick), semi_join_device, semi_join_device(anti=True),
  and both kinds with args=None.

Prints every run and writes medians and min-max to the file given as argv[1] (default
profiles/semi_join/northstar.txt); argv[2] = repetitions (default 7, at least 7). Times are the
calls' own device times (events around the pipeline). The counts are checked: R is a primary key, so
SEMI has the north star's 10,240,000 rows and ANTI the other 1,013,760,000."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import hwbloomradixjoin_amd as hw  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "semi_join", "northstar.txt")
reps = max(7, int(sys.argv[2])) if len(sys.argv) > 2 else 7
nR, nS, q = 128000000, 1024000000, 0.01
N_SEMI, N_ANTI, FILTERED = 10240000, 1013760000, 124236515
dR = torch.empty((nR, 2), dtype=torch.int32, device="cuda")
dS = torch.empty((nS, 2), dtype=torch.int32, device="cuda")
hw.generate_device(dR, 2, nR, nR, 1.0, 12345)
hw.generate_device(dS, 2, 2**31 - 1, nR, q, 54321)
args = hw.BloomFilterArgs(hw.BLOCKED, 1 << 30, 1, 1024)


def mat():
    st, pairs, ms = hw.join_materialize_device(dR, dS, args, capacity=N_SEMI)
    assert (st.filtered, pairs.shape[0]) == (FILTERED, N_SEMI), (st.filtered, pairs.shape[0])
    return ms, st


def semi(a, anti):
    want = N_ANTI if anti else N_SEMI
    st, rows, ms = hw.semi_join_device(dR, dS, a, anti=anti, capacity=want)
    assert (st.matches, rows.shape[0]) == (want, want), (st.matches, rows.shape[0])
    assert st.filtered == (FILTERED if a is not None else nS), st.filtered
    return ms, st


def anti_bytes(filtered):
    """HBM bytes the ANTI pipeline moves, from the shapes (4-byte words, 8-byte tuples; F3 of
    DESIGN.md's traffic model): the S scatter reads the tuples and writes words + payloads, the probe
    reads the words and writes the survivors' codes + positions, the R side reads R, writes and re-reads
    its words and writes the join's codes, the join reads those and the survivors, the marks are
    cleared and read (one bit per S position), and the emission pass reads words + payloads and writes
    the rows."""
    s_scatter = 8 * nS + 8 * nS
    probe = 4 * nS + 8 * filtered
    r_side = 8 * nR + 4 * nR + 4 * nR + 4 * nR
    join = 4 * nR + 8 * filtered
    marks = 2 * (nS // 8)
    emit = 8 * nS + 8 * N_ANTI
    return s_scatter + probe + r_side + join + marks + emit


cases = [("materialize (yardstick)", mat),
         ("semi blocked", lambda: semi(args, False)), ("anti blocked", lambda: semi(args, True)),
         ("semi no filter", lambda: semi(None, False)), ("anti no filter", lambda: semi(None, True))]
for name, fn in cases:  # warm-up: code objects, buffers, clocks
    ms, _ = fn()
    print(f"warm-up {name}: {ms:.3f} ms", flush=True)
times = {name: [] for name, _ in cases}
phases = {}
for r in range(reps):
    for name, fn in cases:
        ms, st = fn()
        times[name].append(ms)
        phases[name] = st
        print(f"rep {r} {name}: {ms:.3f} ms", flush=True)
copy = hw.copy_bandwidth()
lines = [f"existence joins at the north star: |R| = {nR}, |S| = {nS}, q = {q}, blocked m = 2^30 k = 1 B = 1024",
         f"{hw.lib().hwbrj_version().decode()}", f"{reps} alternating repetitions after one warm-up each; device ms",
         f"{'case':28s} {'median':>9s} {'min':>9s} {'max':>9s}"]
for name, _ in cases:
    t = times[name]
    lines.append(f"{name:28s} {statistics.median(t):9.3f} {min(t):9.3f} {max(t):9.3f}")
for name, _ in cases:
    st = phases[name]
    lines.append(f"phases (last run) {name}: r_sc {st.ms_r_scatter:.3f} r_ix {st.ms_r_index:.3f} build {st.ms_build:.3f} "
                 f"s_sc {st.ms_s_scatter:.3f} s_ix {st.ms_s_index:.3f} probe {st.ms_probe:.3f} join {st.ms_join:.3f}")
tm, ts = times["materialize (yardstick)"], times["semi blocked"]
spread = max(tm) - min(tm)
lines.append(f"SEMI criterion: median {statistics.median(ts):.3f} ms <= materialize median {statistics.median(tm):.3f} ms "
             f"+ its min-max spread {spread:.3f} ms: {'met' if statistics.median(ts) <= statistics.median(tm) + spread else 'NOT met'}")
ab = anti_bytes(FILTERED)
ta = statistics.median(times["anti blocked"])
lines.append(f"ANTI blocked: {ab / 1e9:.2f} GB moved (from the shapes; {8 * N_ANTI / 1e9:.2f} GB of them output) in {ta:.3f} ms = "
             f"{ab / ta / 1e6:.0f} GB/s; copy_measured {copy:.0f} GB/s ({ab / ta / 1e6 / copy:.2f} of it)")
text = "\n".join(lines) + "\n"
print(text)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
