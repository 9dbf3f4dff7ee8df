"""Dev: time the group join on key columns with an S value column (group_join_keys_device) against
the group join on tuples (group_join_device) at the north-star shape (|R| = 128M, |S| = 1024M,
q = 0.01, blocked, m = 2^30, k = 1, B = 1024), in one process: the tuples from generate_device (R's
payload is the row index), S's payloads replaced by a value column (a multiplicative hash of the row
index over the whole int32 range), the three columns cut from the tuples by .contiguous(); one
warm-up of each, then alternating repetitions of the two forms under both kinds, and one run of the
min/max pair (group_minmax_join_device / group_minmax_join_keys_device) per kind.

Prints every run and writes median / min / max of ms_total, ms_s_scatter, ms_r_scatter and ms_join of
both layouts per kind, the phase table of the last run, the measured copy rate, the bytes the S
payload scatter moves under each layout, the time of the interleaving pass the column entry saves
(torch.stack(...).contiguous() of both relations, timed once) and the yardsticks to the file given
as argv[1] (default profiles/keys_group/northstar.txt); argv[2] = repetitions (default 7, at least
7); argv[3] (optional) = a text file appended verbatim (the compiler's resource summary of the new
kernels). The yardsticks hold the column form against the tuple form of the same run, never against
itself. n_out, n_pairs and filtered are asserted equal between the two forms in every run; after the
last repetition the rows with a partner of both forms are compared, and GROUP_ALL's rows without
one are counted."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import hwbloomradixjoin_amd as hw  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "keys_group", "northstar.txt")
reps = max(7, int(sys.argv[2])) if len(sys.argv) > 2 else 7
res_path = sys.argv[3] if len(sys.argv) > 3 else None
nR, nS, q = 128000000, 1024000000, 0.01
dR = torch.empty((nR, 2), dtype=torch.int32, device="cuda")
dS = torch.empty((nS, 2), dtype=torch.int32, device="cuda")
hw.generate_device(dR, 2, nR, nR, 1.0, 12345)
hw.generate_device(dS, 2, 2**31 - 1, nR, q, 54321)
torch.cuda.synchronize()
dR[:, 1] = torch.arange(nR, dtype=torch.int32, device="cuda")  # R.payload = row index (what generate_device wrote)
CH = 1 << 26
for i in range(0, nS, CH):  # the value column: row * 0x9E3779B1 mod 2^32, as int32
    j = min(nS, i + CH)
    v = (torch.arange(i, j, dtype=torch.int64, device="cuda") * 0x9E3779B1) & 0xFFFFFFFF
    dS[i:j, 1] = torch.where(v >= 2**31, v - 2**32, v).to(torch.int32)
del v
kR, kS, vS = dR[:, 0].contiguous(), dS[:, 0].contiguous(), dS[:, 1].contiguous()
torch.cuda.synchronize()
args = hw.BloomFilterArgs(hw.BLOCKED, 1 << 30, 1, 1024)
FIELDS = ("ms_total", "ms_s_scatter", "ms_r_scatter", "ms_join")
KINDS = (("matched", hw.GROUP_MATCHED), ("all", hw.GROUP_ALL))


def run(layout, kind, minmax=False):
    """(Stats, rows, n_pairs) of one group join; capacity |R| bounds the rows of either kind."""
    if layout == "tuples":
        fn = hw.group_minmax_join_device if minmax else hw.group_join_device
        st, rows, pairs, _ = fn(dR, dS, args, kind=kind, capacity=nR)
    else:
        fn = hw.group_minmax_join_keys_device if minmax else hw.group_join_keys_device
        st, rows, pairs, _ = fn(kR, kS, vS, args, kind=kind, capacity=nR)
    return st, rows, pairs


def same_counts(a, b, what):
    (sa, ra, pa), (sb, rb, pb) = a, b
    assert (sa.matches, pa, sa.filtered) == (sb.matches, pb, sb.filtered) and ra.raw.shape == rb.raw.shape, (what, sa, sb)


def matched_rows(rows):
    """The rows with count > 0, as (n, 2) int64 words sorted by word 0 ({r_payload, count}; R payloads
    are distinct). Under GROUP_ALL these must be GROUP_MATCHED's rows."""
    raw = rows.raw.view(torch.int64).reshape(-1, 2)
    raw = raw[rows.count > 0]
    return raw[torch.sort(raw[:, 0]).indices]


def same_rows(a, b):
    """The rows with partners of both forms as equal multisets."""
    return bool(torch.equal(matched_rows(a), matched_rows(b)))


def lone_rows(rows):
    """(rows with count 0, distinct r_payloads among them): GROUP_ALL's rows without a partner."""
    lone = rows.r_payload[rows.count == 0]
    return int(lone.numel()), int(torch.unique(lone).numel())


for layout in ("tuples", "keys"):  # warm-up: code objects, buffers, clocks
    st, _, _ = run(layout, hw.GROUP_ALL)
    print(f"warm-up {layout}: {st.ms_total:.3f} ms", flush=True)
runs = {(k, layout): [] for k, _ in KINDS for layout in ("tuples", "keys")}
last = {}
for r in range(reps):
    for kname, kind in KINDS:
        for layout in ("tuples", "keys"):
            res = run(layout, kind)
            last[kname, layout] = res
            runs[kname, layout].append(res[0])
            st = res[0]
            print(f"rep {r} {kname} {layout}: total {st.ms_total:.3f} s_scatter {st.ms_s_scatter:.3f} r_scatter "
                  f"{st.ms_r_scatter:.3f} join {st.ms_join:.3f} ms, rows {st.matches} pairs {res[2]}", flush=True)
        same_counts(last[kname, "tuples"], last[kname, "keys"], (r, kname))
rows_equal = all(same_rows(last[k, "tuples"][1], last[k, "keys"][1]) for k, _ in KINDS)
assert rows_equal, "the column form's rows differ from the tuple form's"
assert torch.equal(matched_rows(last["all", "keys"][1]), matched_rows(last["matched", "keys"][1]))
lone = {layout: lone_rows(last["all", layout][1]) for layout in ("tuples", "keys")}
counts = {k: (last[k, "keys"][0].matches, last[k, "keys"][2], last[k, "keys"][0].filtered) for k, _ in KINDS}
last.clear()
mm_lines = []
for kname, kind in KINDS:  # the min/max pair, once
    a, b = run("tuples", kind, True), run("keys", kind, True)
    same_counts(a, b, ("minmax", kname))
    assert same_rows(a[1], b[1]), "the column form's min/max rows differ from the tuple form's"
    mm_lines.append(f"min/max {kname}: tuples total {a[0].ms_total:.3f} s_sc {a[0].ms_s_scatter:.3f} r_sc "
                    f"{a[0].ms_r_scatter:.3f} join {a[0].ms_join:.3f}; keys total {b[0].ms_total:.3f} s_sc "
                    f"{b[0].ms_s_scatter:.3f} r_sc {b[0].ms_r_scatter:.3f} join {b[0].ms_join:.3f} ms; rows equal")
    del a, b
copy = hw.copy_bandwidth()
# the pass a columnar caller needs before the tuple entry: both relations interleaved (R with an arange)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
tR = torch.stack([kR, torch.arange(nR, dtype=torch.int32, device="cuda")], 1).contiguous()
tS = torch.stack([kS, vS], 1).contiguous()
e1.record()
torch.cuda.synchronize()
ms_interleave = e0.elapsed_time(e1)
del tR, tS


def stat(kname, layout, f):
    v = [getattr(st, f) for st in runs[kname, layout]]
    return statistics.median(v), min(v), max(v)


# bytes of the S payload scatter: the elements read, one word and one payload per element into
# 32-word chunks, a 16-bit meta per chunk (the workgroup x partition matrices are a few MB: left out)
chunks = (nS + 31) // 32
b_s = 8 * nS + 8 * nS + 2 * chunks  # (both layouts read 8 bytes per element: tuple, or key + value)
b_il = (8 * nS + 8 * nS) + (4 * nR + 8 * nR)  # the interleaving pass: S read + written, R keys read, R tuples written
lines = [f"group join on key columns with an S value column at the north star: |R| = {nR}, |S| = {nS}, q = {q}, blocked "
         "m = 2^30 k = 1 B = 1024",
         f"{hw.lib().hwbrj_version().decode()}",
         f"{reps} alternating repetitions per kind (tuples: group_join_device, keys: group_join_keys_device) after one "
         "warm-up each; device ms",
         "n_out, n_pairs and filtered asserted equal between the two forms in every run; the rows with count > 0 of the "
         f"last repetition equal between the forms, and between the kinds: {rows_equal}",
         "GROUP_ALL's rows with count 0 (reported, not asserted): " +
         ", ".join(f"{layout} {lone[layout][0]} rows with {lone[layout][1]} distinct r_payload" for layout in lone)]
for kname, _ in KINDS:
    lines.append(f"kind {kname}: rows {counts[kname][0]}, n_pairs {counts[kname][1]}, filtered {counts[kname][2]}")
lines.append(f"{'kind':8s} {'layout':8s} {'phase':13s} {'median':>9s} {'min':>9s} {'max':>9s}")
for kname, _ in KINDS:
    for layout in ("tuples", "keys"):
        for f in FIELDS:
            m, lo, hi = stat(kname, layout, f)
            lines.append(f"{kname:8s} {layout:8s} {f:13s} {m:9.3f} {lo:9.3f} {hi:9.3f}")
for kname, _ in KINDS:
    for layout in ("tuples", "keys"):
        st = runs[kname, layout][-1]
        lines.append(f"phases (last run) {kname} {layout}: r_sc {st.ms_r_scatter:.3f} r_ix {st.ms_r_index:.3f} build "
                     f"{st.ms_build:.3f} s_sc {st.ms_s_scatter:.3f} s_ix {st.ms_s_index:.3f} probe {st.ms_probe:.3f} join "
                     f"{st.ms_join:.3f}")
lines += mm_lines
lines.append(f"copy_measured {copy:.0f} GB/s")
lines.append(f"S payload scatter bytes, both layouts: {b_s / 1e9:.2f} GB (read {8 * nS / 1e9:.2f}: tuples, or keys "
             f"{4 * nS / 1e9:.2f} + values {4 * nS / 1e9:.2f}; chunk words {4 * nS / 1e9:.2f} GB, payloads {4 * nS / 1e9:.2f} GB "
             f"and metas {2 * chunks / 1e9:.3f} GB written)")
verdicts = []
for kname, _ in KINDS:
    for f in ("ms_s_scatter", "ms_r_scatter"):
        mt, lo_t, hi_t = stat(kname, "tuples", f)
        mk, _, _ = stat(kname, "keys", f)
        bound = mt + (hi_t - lo_t)
        verdicts.append(mk <= bound)
        lines.append(f"condition ({kname}): keys {f} median {mk:.3f} ms <= tuples {mt:.3f} + its spread {hi_t - lo_t:.3f} = "
                     f"{bound:.3f} ms: {'met' if mk <= bound else f'NOT met (by {mk - bound:.3f} ms)'}")
    mt, mk = stat(kname, "tuples", "ms_join")[0], stat(kname, "keys", "ms_join")[0]
    lines.append(f"join phase ({kname}, no condition: the same kernel on the same pools): tuples {mt:.3f}, keys {mk:.3f} ms")
lines.append(f"verdict: {'met' if all(verdicts) else 'NOT met'}")
mt, mk = stat("matched", "tuples", "ms_total")[0], stat("matched", "keys", "ms_total")[0]
pred_il = b_il / copy / 1e6
lines.append(f"interleaving pass (torch.stack(...).contiguous() of both relations, timed once): {ms_interleave:.3f} ms for "
             f"{b_il / 1e9:.2f} GB ({b_il / ms_interleave / 1e6:.0f} GB/s)")
lines.append(f"prediction (not gated): a columnar caller's whole call falls by the interleaving pass, {b_il / 1e9:.2f} GB at "
             f"the copy rate = {pred_il:.3f} ms, from {mt:.3f} + {pred_il:.3f} = {mt + pred_il:.3f} ms to {mt:.3f} ms; measured: "
             f"interleave {ms_interleave:.3f} + tuples {mt:.3f} = {ms_interleave + mt:.3f} ms against keys {mk:.3f} ms "
             f"({(ms_interleave + mt) / mk:.2f} x)")
if res_path:
    lines.append("compiler resource summary (-Rpass-analysis=kernel-resource-usage) of the new kernels:")
    lines += open(res_path).read().rstrip("\n").split("\n")
text = "\n".join(lines) + "\n"
print(text)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
