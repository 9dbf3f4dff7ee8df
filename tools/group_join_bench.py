"""Dev: time the group joins at the north-star shape (|R| = 128M, |S| = 1024M, q = 0.01, blocked,
m = 2^30, k = 1) against OUTER_R, the existing kernel with per-R-tuple LDS state and an end-of-piece
row write, in one process, alternating after a warm-up:

  join_materialize_device, outer_join_device(OUTER_R), group_join_device of GROUP_MATCHED and
  GROUP_ALL, group_minmax_join_device of both kinds (MINMAX_MATCHED, MINMAX_ALL); then one run of
  each group kind of both forms with args=None, and one of each on a Zipf S
  (create_relation_zipf_device, theta = 0.75, q = 0.01).

Prints every run and writes medians, min-max, the phase table, the bytes the shapes move, the
measured copy rate and the yardstick comparisons to the file given as argv[1] (default
profiles/group_join/minmax_northstar.txt; northstar.txt is the run before the min/max form existed);
argv[2] = repetitions (default 7, at least 7). Times are the calls' own device times (events around
the pipeline); the min/max kinds are held against the sum kinds' join phase (Stats.ms_join) of the
same run plus its spread. The counts are asserted, for the min/max kinds the same as for the sum kinds: R is a primary key,
so GROUP_MATCHED has as many rows as R has keys with a partner, which a count-only semi-join of R
against S (arguments swapped) counts; GROUP_ALL has 128,000,000 rows; n_pairs is the north star's
10,240,000 and `filtered` its 124,236,515."""
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import hwbloomradixjoin_amd as hw  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "group_join", "minmax_northstar.txt")
reps = max(7, int(sys.argv[2])) if len(sys.argv) > 2 else 7
nR, nS, q = 128000000, 1024000000, 0.01
N_PAIRS, FILTERED = 10240000, 124236515
dR = torch.empty((nR, 2), dtype=torch.int32, device="cuda")
dS = torch.empty((nS, 2), dtype=torch.int32, device="cuda")
hw.generate_device(dR, 2, nR, nR, 1.0, 12345)
hw.generate_device(dS, 2, 2**31 - 1, nR, q, 54321)
args = hw.BloomFilterArgs(hw.BLOCKED, 1 << 30, 1, 1024)
NULL = -2**31


def matched_r_rows(S):
    """The R rows that have a partner in S (count-only semi-join, arguments swapped)."""
    n = ctypes.c_uint64()
    rc = hw.lib().hwbrj_join_semi_device(S.data_ptr(), S.shape[0], dR.data_ptr(), nR, None, hw.JOIN_SEMI, None, 0,
                                         ctypes.byref(n), None, None, None)
    assert rc in (0, 7), (rc, hw.lib().hwbrj_last_error())
    return n.value


N_MATCHED = matched_r_rows(dS)
N_R_ONLY = nR - N_MATCHED
print(f"matched R rows {N_MATCHED}, R-only rows {N_R_ONLY}", flush=True)
torch.cuda.empty_cache()


def mat():
    st, pairs, ms = hw.join_materialize_device(dR, dS, args, capacity=N_PAIRS)
    assert (st.filtered, pairs.shape[0]) == (FILTERED, N_PAIRS), (st.filtered, pairs.shape[0])
    return ms, st


def outer_r():
    want = N_PAIRS + N_R_ONLY
    st, rows, cls, ms = hw.outer_join_device(dR, dS, args, kind=hw.OUTER_R, null_payload=NULL, capacity=want)
    assert cls == (N_PAIRS, 0, N_R_ONLY) and rows.shape[0] == want, (cls, rows.shape[0])
    return ms, st


def group(S, a, kind, want_rows, want_pairs, want_filtered, fn=hw.group_join_device):
    st, rows, pairs, ms = fn(dR, S, a, kind=kind, capacity=want_rows)
    assert (st.matches, rows.raw.shape[0]) == (want_rows, want_rows), (st.matches, rows.raw.shape[0], want_rows)
    assert pairs == want_pairs, (pairs, want_pairs)
    assert st.filtered == want_filtered, (st.filtered, want_filtered)
    return ms, st


def bytes_moved(kind):
    """HBM bytes of a pipeline from the shapes (tools/outer_join_bench.py's model): the payload
    pipeline's common traffic, R's payloads (scatter, build, join), then the rows: 8 bytes a pair or
    R-only row, 16 bytes a group row; the group joins also read the matching survivors' positions
    and payloads as the materializing join does and write no pair."""
    common = (8 * nS + 8 * nS) + (4 * nS + 8 * FILTERED) + (8 * nR + 4 * nR + 4 * nR + 4 * nR) + (4 * nR + 8 * FILTERED)
    rpay = 4 * nR + 4 * nR + 4 * nR + 4 * nR
    return {"materialize": common + rpay + 8 * N_PAIRS,
            "outer_r": common + rpay + 8 * (N_PAIRS + N_R_ONLY),
            "group_matched": common + rpay + 16 * N_MATCHED,
            "group_all": common + rpay + 16 * nR,
            "minmax_matched": common + rpay + 16 * N_MATCHED,
            "minmax_all": common + rpay + 16 * nR}[kind]


MINMAX = hw.group_minmax_join_device
cases = [("materialize", mat), ("outer_r", outer_r),
         ("group_matched", lambda: group(dS, args, hw.GROUP_MATCHED, N_MATCHED, N_PAIRS, FILTERED)),
         ("group_all", lambda: group(dS, args, hw.GROUP_ALL, nR, N_PAIRS, FILTERED)),
         ("minmax_matched", lambda: group(dS, args, hw.GROUP_MATCHED, N_MATCHED, N_PAIRS, FILTERED, MINMAX)),
         ("minmax_all", lambda: group(dS, args, hw.GROUP_ALL, nR, N_PAIRS, FILTERED, MINMAX))]
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
copy = hw.copy_bandwidth()
extra = {}
KINDS = (("group_matched", hw.GROUP_MATCHED, hw.group_join_device), ("group_all", hw.GROUP_ALL, hw.group_join_device),
         ("minmax_matched", hw.GROUP_MATCHED, MINMAX), ("minmax_all", hw.GROUP_ALL, MINMAX))
for name, kind, fn in KINDS:
    rows = nR if kind == hw.GROUP_ALL else N_MATCHED
    group(dS, None, kind, rows, N_PAIRS, nS, fn)  # (warm-up of the no-filter geometry's buffers)
    extra[name + " no filter"], _ = group(dS, None, kind, rows, N_PAIRS, nS, fn)
    print(f"no filter {name}: {extra[name + ' no filter']:.3f} ms", flush=True)
# a Zipf S over R's keys: hot keys put thousands of LDS atomics on one accumulator
hw.create_relation_zipf_device(dS, nR, 0.75, 54321, q, 16)
cj = hw.join_device(dR, dS, args)
z_matched = matched_r_rows(dS)
print(f"zipf: pairs {cj.matches}, filtered {cj.filtered}, matched R rows {z_matched}", flush=True)
for name, kind, fn in KINDS:
    rows = nR if kind == hw.GROUP_ALL else z_matched
    group(dS, args, kind, rows, cj.matches, cj.filtered, fn)  # (warm-up)
    extra[name + " zipf 0.75"], zst = group(dS, args, kind, rows, cj.matches, cj.filtered, fn)
    phases[name + " zipf 0.75"] = zst
    print(f"zipf {name}: {extra[name + ' zipf 0.75']:.3f} ms", flush=True)

med = {k: statistics.median(v) for k, v in times.items()}
spread = {k: max(v) - min(v) for k, v in times.items()}
lines = [f"group joins at the north star: |R| = {nR}, |S| = {nS}, q = {q}, blocked m = 2^30 k = 1 B = 1024",
         f"{hw.lib().hwbrj_version().decode()}", f"{reps} alternating repetitions after one warm-up each; device ms",
         f"counts asserted: GROUP_MATCHED rows {N_MATCHED} (R rows with a partner), GROUP_ALL rows {nR}, "
         f"n_pairs {N_PAIRS}, filtered {FILTERED} (MINMAX_MATCHED and MINMAX_ALL: the same); OUTER_R rows "
         f"{N_PAIRS + N_R_ONLY}",
         f"{'case':14s} {'median':>9s} {'min':>9s} {'max':>9s} {'GB moved':>9s} {'GB/s':>7s}"]
for name, _ in cases:
    t = times[name]
    gb = bytes_moved(name) / 1e9
    lines.append(f"{name:14s} {med[name]:9.3f} {min(t):9.3f} {max(t):9.3f} {gb:9.2f} {gb / med[name] * 1e3:7.0f}")
lines.append(f"{'join phase':14s} {'median':>9s} {'min':>9s} {'max':>9s}")
for name, _ in cases:
    j = joins[name]
    lines.append(f"{name:14s} {statistics.median(j):9.3f} {min(j):9.3f} {max(j):9.3f}")
for name, ms in extra.items():
    lines.append(f"{name:26s} {ms:9.3f} (one run after one warm-up)")
lines.append(f"zipf 0.75 S: n_pairs {cj.matches}, filtered {cj.filtered}, GROUP_MATCHED rows {z_matched}")
for name, st in phases.items():
    lines.append(f"phases (last run) {name}: r_sc {st.ms_r_scatter:.3f} r_ix {st.ms_r_index:.3f} build {st.ms_build:.3f} "
                 f"s_sc {st.ms_s_scatter:.3f} s_ix {st.ms_s_index:.3f} probe {st.ms_probe:.3f} join {st.ms_join:.3f}")
lines.append(f"copy_measured {copy:.0f} GB/s")
b_m = med["outer_r"] + spread["outer_r"]
lines.append(f"GROUP_MATCHED yardstick: median {med['group_matched']:.3f} ms <= OUTER_R {med['outer_r']:.3f} + its spread "
             f"{spread['outer_r']:.3f} = {b_m:.3f} ms: {'met' if med['group_matched'] <= b_m else 'NOT met'}")
add_gb = (16 * nR - 8 * (N_PAIRS + N_R_ONLY)) / 1e9  # the rows written beyond OUTER_R's
add_ms = add_gb / copy * 1e3
b_a = med["outer_r"] + add_ms + spread["outer_r"] + spread["group_all"]
lines.append(f"GROUP_ALL yardstick: median {med['group_all']:.3f} ms <= OUTER_R {med['outer_r']:.3f} + "
             f"({16 * nR / 1e9:.2f} - {8 * (N_PAIRS + N_R_ONLY) / 1e9:.2f} GB) / copy rate = {add_ms:.3f} ms + the two spreads "
             f"{spread['outer_r'] + spread['group_all']:.3f} = {b_a:.3f} ms: {'met' if med['group_all'] <= b_a else 'NOT met'}")
for mm, sm in (("minmax_matched", "group_matched"), ("minmax_all", "group_all")):  # join phase against the sum form's
    jm, js = statistics.median(joins[mm]), statistics.median(joins[sm])
    sp = max(joins[sm]) - min(joins[sm])
    lines.append(f"{mm.upper()} yardstick: join-phase median {jm:.3f} ms <= {sm.upper()}'s {js:.3f} + its spread {sp:.3f} = "
                 f"{js + sp:.3f} ms: {'met' if jm <= js + sp else f'NOT met (by {jm - js - sp:.3f} ms)'}")
text = "\n".join(lines) + "\n"
print(text)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
