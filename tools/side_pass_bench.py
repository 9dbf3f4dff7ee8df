"""Dev: time the side passes of the global-bitmap mode: |R| = 2^24 (primary key), |S| = 2^27 at
selectivity 0.05, generated on the device, filter BLOCKED m = 2^28 k = 1 B = 4 (stats.mode == 3
asserted), in one process, alternating after one warm-up each:

  join_materialize_device, semi_join_device (semi, anti), outer_join_device (OUTER_S, OUTER_R,
  OUTER_FULL), group_join_device and group_minmax_join_device (GROUP_MATCHED, GROUP_ALL).

The time of a run is the `ms` its entry returns, which in this mode is the side pass's own device
time (table build to last probe; the counting join before it is not in it). Prints every run and
writes median, min, max and max - min per case to the file given as argv[1] (default
profiles/side_pass/<library stamp>.txt); argv[2] = repetitions (default 7, at least 7). For an A/B of
two libraries run it once per library (HWBRJ_LIB) in separate processes, alternating."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import hwbloomradixjoin_amd as hw  # noqa: E402

version = hw.version()
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "side_pass",
                                                              version.split()[-1] + ".txt")
reps = max(7, int(sys.argv[2])) if len(sys.argv) > 2 else 7
nR, nS, q = 1 << 24, 1 << 27, 0.05
dR = torch.empty((nR, 2), dtype=torch.int32, device="cuda")
dS = torch.empty((nS, 2), dtype=torch.int32, device="cuda")
hw.generate_device(dR, 2, nR, nR, 1.0, 12345)
hw.generate_device(dS, 2, 2**31 - 1, nR, q, 54321)
args = hw.BloomFilterArgs(hw.BLOCKED, 1 << 28, 1, 4)
NULL = -2**31

count = hw.join_device(dR, dS, args)
assert count.mode == 3, count.mode
N_INNER, N_S_ONLY = count.matches, nS - count.matches  # (R is a primary key)
st, rows, _, _ = hw.group_join_device(dR, dS, args, kind=hw.GROUP_MATCHED)
N_MATCHED = rows.r_payload.shape[0]
del rows
N_R_ONLY = nR - N_MATCHED
print(f"{version}\ninner {N_INNER}, S-only {N_S_ONLY}, matched R rows {N_MATCHED}, R-only {N_R_ONLY}", flush=True)
torch.cuda.empty_cache()


def mat():
    st, pairs, ms = hw.join_materialize_device(dR, dS, args, capacity=N_INNER)
    assert (st.mode, pairs.shape[0]) == (3, N_INNER), (st.mode, pairs.shape[0])
    return ms


def semi(anti):
    want = N_S_ONLY if anti else N_INNER
    st, rows, ms = hw.semi_join_device(dR, dS, args, anti=anti, capacity=want)
    assert (st.mode, st.matches, rows.shape[0]) == (3, want, want), (st.mode, st.matches, rows.shape[0])
    return ms


def outer(kind):
    want = (N_INNER, N_S_ONLY if kind != hw.OUTER_R else 0, N_R_ONLY if kind != hw.OUTER_S else 0)
    st, rows, cls, ms = hw.outer_join_device(dR, dS, args, kind=kind, null_payload=NULL, capacity=sum(want))
    assert (st.mode, cls, rows.shape[0]) == (3, want, sum(want)), (st.mode, cls, rows.shape[0])
    return ms


def group(fn, kind):
    want = nR if kind == hw.GROUP_ALL else N_MATCHED
    st, rows, pairs, ms = fn(dR, dS, args, kind=kind, capacity=want)
    assert (st.mode, st.matches, pairs) == (3, want, N_INNER), (st.mode, st.matches, pairs)
    return ms


cases = [("pairs", mat), ("semi", lambda: semi(False)), ("anti", lambda: semi(True)),
         ("outer_s", lambda: outer(hw.OUTER_S)), ("outer_r", lambda: outer(hw.OUTER_R)),
         ("outer_full", lambda: outer(hw.OUTER_FULL)),
         ("group_matched", lambda: group(hw.group_join_device, hw.GROUP_MATCHED)),
         ("group_all", lambda: group(hw.group_join_device, hw.GROUP_ALL)),
         ("minmax_matched", lambda: group(hw.group_minmax_join_device, hw.GROUP_MATCHED)),
         ("minmax_all", lambda: group(hw.group_minmax_join_device, hw.GROUP_ALL))]
for name, fn in cases:  # warm-up: code objects, buffers, clocks
    print(f"warm-up {name}: {fn():.3f} ms", flush=True)
times = {name: [] for name, _ in cases}
for r in range(reps):
    for name, fn in cases:
        times[name].append(fn())
        print(f"rep {r} {name}: {times[name][-1]:.3f} ms", flush=True)
lines = [f"side passes: |R| = {nR}, |S| = {nS}, q = {q}, blocked m = 2^28 k = 1 B = 4 (global-bitmap mode)",
         version, f"{reps} alternating repetitions after one warm-up each; device ms of the side pass",
         f"rows asserted: inner {N_INNER}, S-only {N_S_ONLY}, R-only {N_R_ONLY}, matched R rows {N_MATCHED}",
         f"{'case':16s} {'median':>9s} {'min':>9s} {'max':>9s} {'spread':>9s}"]
for name, _ in cases:
    t = times[name]
    lines.append(f"{name:16s} {statistics.median(t):9.3f} {min(t):9.3f} {max(t):9.3f} {max(t) - min(t):9.3f}")
text = "\n".join(lines) + "\n"
print(text)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
