"""Dev: time the pair join on key columns (join_keys_pairs_device, row indices as payloads) against
the materializing join on tuples (join_materialize_device) at the north-star shape (|R| = 128M,
|S| = 1024M, q = 0.01, blocked, m = 2^30, k = 1, B = 1024), in one process: the tuples from
generate_device (their payload is the row index), the key columns cut from them by
T[:, 0].contiguous(); one warm-up of each, then alternating repetitions of the two joins.

Prints every run and writes median / min / max of ms_total, ms_s_scatter and ms_r_scatter of both
layouts, the measured copy rate, the bytes the S payload scatter moves under each layout, and the
yardsticks to the file given as argv[1] (default profiles/keys_pairs/northstar.txt); argv[2] =
repetitions (default 7, at least 7); argv[3] (optional) = a text file appended verbatim (the
compiler's resource summary of the key-column kernels). The yardsticks hold the key path against the
tuple path of the same run, never against itself. The counts are asserted in every run (filtered
124,236,515, pairs 10,240,000); after the last repetition the two pair multisets are compared."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import hwbloomradixjoin_amd as hw  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "keys_pairs", "northstar.txt")
reps = max(7, int(sys.argv[2])) if len(sys.argv) > 2 else 7
res_path = sys.argv[3] if len(sys.argv) > 3 else None
nR, nS, q = 128000000, 1024000000, 0.01
N_PAIRS, FILTERED = 10240000, 124236515
dR = torch.empty((nR, 2), dtype=torch.int32, device="cuda")
dS = torch.empty((nS, 2), dtype=torch.int32, device="cuda")
hw.generate_device(dR, 2, nR, nR, 1.0, 12345)
hw.generate_device(dS, 2, 2**31 - 1, nR, q, 54321)
kR, kS = dR[:, 0].contiguous(), dS[:, 0].contiguous()
torch.cuda.synchronize()
args = hw.BloomFilterArgs(hw.BLOCKED, 1 << 30, 1, 1024)
FIELDS = ("ms_total", "ms_s_scatter", "ms_r_scatter")


def run(layout):
    if layout == "tuples":
        st, pairs, _ = hw.join_materialize_device(dR, dS, args, capacity=N_PAIRS)
    else:
        st, pairs, _ = hw.join_keys_pairs_device(kR, kS, args, capacity=N_PAIRS)
    assert (st.filtered, st.matches, pairs.shape[0]) == (FILTERED, N_PAIRS, N_PAIRS), (layout, st)
    return st, pairs


def as_u64(pairs):  # sorted pairs, each as one 64-bit word
    return torch.sort(pairs.contiguous().view(torch.int64).ravel()).values


for layout in ("tuples", "keys"):  # warm-up: code objects, buffers, clocks
    st, _ = run(layout)
    print(f"warm-up {layout}: {st.ms_total:.3f} ms", flush=True)
runs = {"tuples": [], "keys": []}
last = {}
for r in range(reps):
    for layout in ("tuples", "keys"):
        st, last[layout] = run(layout)
        runs[layout].append(st)
        print(f"rep {r} {layout}: total {st.ms_total:.3f} s_scatter {st.ms_s_scatter:.3f} r_scatter {st.ms_r_scatter:.3f} ms",
              flush=True)
same = bool(torch.equal(as_u64(last["tuples"]), as_u64(last["keys"])))
assert same, "the key-column pairs differ from the tuple pairs"
copy = hw.copy_bandwidth()


def stat(layout, f):
    v = [getattr(st, f) for st in runs[layout]]
    return statistics.median(v), min(v), max(v)


# bytes of the S payload scatter: the elements read, one word and one payload per element into
# 32-word chunks, a 16-bit meta per chunk (the workgroup x partition matrices are a few MB: left out)
chunks = (nS + 31) // 32
b_t, b_k = 8 * nS + 8 * nS + 2 * chunks, 4 * nS + 8 * nS + 2 * chunks
lines = [f"row-index pair join on key columns at the north star: |R| = {nR}, |S| = {nS}, q = {q}, blocked m = 2^30 k = 1 B = 1024",
         f"{hw.lib().hwbrj_version().decode()}",
         f"{reps} alternating repetitions (tuples: join_materialize_device, keys: join_keys_pairs_device) after one warm-up each; "
         "device ms",
         f"counts asserted in every run: filtered {FILTERED}, pairs {N_PAIRS}; pair multisets of the last repetition equal: {same}",
         f"{'layout':8s} {'phase':13s} {'median':>9s} {'min':>9s} {'max':>9s}"]
for layout in ("tuples", "keys"):
    for f in FIELDS:
        m, lo, hi = stat(layout, f)
        lines.append(f"{layout:8s} {f:13s} {m:9.3f} {lo:9.3f} {hi:9.3f}")
for layout in ("tuples", "keys"):
    st = runs[layout][-1]
    lines.append(f"phases (last run) {layout}: r_sc {st.ms_r_scatter:.3f} r_ix {st.ms_r_index:.3f} build {st.ms_build:.3f} "
                 f"s_sc {st.ms_s_scatter:.3f} s_ix {st.ms_s_index:.3f} probe {st.ms_probe:.3f} join {st.ms_join:.3f}")
lines.append(f"copy_measured {copy:.0f} GB/s")
lines.append(f"S payload scatter bytes: tuples {b_t / 1e9:.2f} GB (read {8 * nS / 1e9:.2f}), keys {b_k / 1e9:.2f} GB "
             f"(read {4 * nS / 1e9:.2f}); chunk words {4 * nS / 1e9:.2f} GB, payloads {4 * nS / 1e9:.2f} GB and metas "
             f"{2 * chunks / 1e9:.3f} GB written by both")
verdicts = []
for f in ("ms_s_scatter", "ms_r_scatter"):
    mt, lo_t, hi_t = stat("tuples", f)
    mk, _, _ = stat("keys", f)
    bound = mt + (hi_t - lo_t)
    verdicts.append(mk <= bound)
    lines.append(f"condition: keys {f} median {mk:.3f} ms <= tuples {mt:.3f} + its spread {hi_t - lo_t:.3f} = {bound:.3f} ms: "
                 f"{'met' if mk <= bound else f'NOT met (by {mk - bound:.3f} ms)'}")
lines.append(f"verdict: {'met' if all(verdicts) else 'NOT met'}")
mt, mk = stat("tuples", "ms_s_scatter")[0], stat("keys", "ms_s_scatter")[0]
pred = mt * b_k / b_t
lines.append(f"prediction (not gated): tuples {mt:.3f} ms x {b_k / b_t:.3f} (bytes) = {pred:.3f} ms at the tuple kernel's rate "
             f"({b_t / mt / 1e6:.0f} GB/s); keys reach {mk:.3f} ms = {b_k / mk / 1e6:.0f} GB/s, {pred / mk:.2f} of the prediction: "
             f"{'met' if mk <= pred else 'NOT met'}")
if res_path:
    lines.append("compiler resource summary (-Rpass-analysis=kernel-resource-usage) of the key-column kernels:")
    lines += open(res_path).read().rstrip("\n").split("\n")
text = "\n".join(lines) + "\n"
print(text)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
