"""Dev: time a build's filter applied to a key column (filter_keys_device) at the north-star shape (key
columns, |R| = 128M, blocked, m = 2^30, k = 1, B = 1024, q = 0.01) on S batches of 64M and 1024M rows,
in one process.

 yardstick  the counting probe of the same build and batch (probe_keys_device), which streams the same
            key column once and scatters it: its ms_s_scatter.
 new        filter_keys_device's ms: the same stream, one gathered filter word per key, one bit out.

7 alternating repetitions after one warm-up each; n_pass is asserted equal to the probe's `filtered` in
every repetition. Condition, reported and not preset by what the code gives: the filter pass's median
<= the probe's median ms_s_scatter + that probe's own max - min.

Recorded without a threshold: the pass at sectorized k = 2 and at basic k = 1 (same m), and the star
case: two 128M builds over two key columns of a 64M-row S, the second filter ANDed in place into the
first one's bitmap, and build 1's pairs probe with and without the intersected bitmap.

Prints every run and writes the tables to argv[1] (default profiles/runtime_filter/northstar.txt);
argv[2] = repetitions (default 7, at least 7)."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import hwbloomradixjoin_amd as hw  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "runtime_filter", "northstar.txt")
reps = max(7, int(sys.argv[2])) if len(sys.argv) > 2 else 7
nR, nS, q = 128000000, 1024000000, 0.01
BATCH = 64000000
M = 1 << 30


def column(n, maxid, sel, seed):
    t = torch.empty((n, 2), dtype=torch.int32, device="cuda")
    hw.generate_device(t, 2, maxid, nR, sel, seed)
    torch.cuda.synchronize()
    k = t[:, 0].contiguous()
    del t
    torch.cuda.empty_cache()
    return k


lines = [f"a build's filter as a selection bitmap at the north star: |R| = {nR}, q = {q}, m = 2^30, key columns",
         hw.lib().hwbrj_version().decode(), f"{reps} alternating repetitions after one warm-up each; device ms"]


def say(s):
    print(s, flush=True)
    lines.append(s)


def med(v):
    return statistics.median(v)


def mmm(v):
    return f"median {med(v):.3f} (min {min(v):.3f}, max {max(v):.3f})"


kR = column(nR, nR, 1.0, 12345)
kS = column(nS, 2**31 - 1, q, 54321)
SIZES = (("64M", kS[:BATCH]), ("1024M", kS))
out = torch.empty((nS + 31) // 32 * 4, dtype=torch.uint8, device="cuda")

# ---- the condition: blocked k = 1 against the counting probe's S scatter
args = hw.BloomFilterArgs(hw.BLOCKED, M, 1, 1024)
verdicts = []
with hw.build_keys_device(kR, args, hw.BUILD_COUNT) as b:
    say(f"blocked k = 1 B = 1024: build {b.ms:.3f} ms, {b.info()['bytes'] / 2**20:.1f} MiB held")
    for name, S in SIZES:
        n = S.shape[0]
        st = hw.probe_keys_device(b, S)
        _, n_pass, ms = hw.filter_keys_device(b, S, out=out)
        say(f"S = {name} ({n} rows): warm-up probe ms_s_scatter {st.ms_s_scatter:.3f} (ms_total {st.ms_total:.3f}), filter pass {ms:.3f}; "
            f"{n_pass} rows pass ({n_pass / n:.4f})")
        P, T, F = [], [], []
        for r in range(reps):
            st = hw.probe_keys_device(b, S)
            _, n_pass, ms = hw.filter_keys_device(b, S, out=out)
            assert n_pass == st.filtered, (n_pass, st.filtered)
            P.append(st.ms_s_scatter)
            T.append(st.ms_total)
            F.append(ms)
            print(f"rep {r} {name}: probe ms_s_scatter {st.ms_s_scatter:.3f} ms_total {st.ms_total:.3f}; filter {ms:.3f}; n_pass {n_pass}",
                  flush=True)
        spread = max(P) - min(P)
        ok = med(F) <= med(P) + spread
        verdicts.append(ok)
        say(f"{name} probe ms_s_scatter: {mmm(P)}; ms_total {mmm(T)}")
        say(f"{name} filter pass:        {mmm(F)}; {n * 4 / med(F) / 1e6:.0f} GB/s of keys, {n / med(F) / 1e6:.1f} G keys/s")
        say(f"condition ({name}): filter {med(F):.3f} <= ms_s_scatter {med(P):.3f} + its spread {spread:.3f} = {med(P) + spread:.3f} ms: "
            f"{'met' if ok else f'MISSED (by {med(F) - med(P) - spread:.3f} ms)'}")
say(f"verdict: {'met' if all(verdicts) else 'MISSED'}")

# ---- recorded without a threshold: the other kernels' forms
say("")
for label, a in (("sectorized k = 2 B = 1024", hw.BloomFilterArgs(hw.SECTORIZED, M, 2, 1024)),
                 ("basic k = 1", hw.BloomFilterArgs(hw.BASIC, M, 1, 1024))):
    with hw.build_keys_device(kR, a, hw.BUILD_COUNT) as b:
        for name, S in SIZES:
            hw.filter_keys_device(b, S, out=out)
            F, n_pass = [], 0
            for r in range(reps):
                _, n_pass, ms = hw.filter_keys_device(b, S, out=out)
                F.append(ms)
            say(f"{label}, S = {name}: filter pass {mmm(F)}; {n_pass} rows pass")

# ---- the star case
say("")
del kS, SIZES
torch.cuda.empty_cache()
kR2 = column(nR, nR, 1.0, 777)
S1 = column(BATCH, 2**31 - 1, q, 54321)
S2 = column(BATCH, 2**31 - 1, 0.5, 999)
CAP = 4 << 20
with hw.build_keys_device(kR, args, hw.BUILD_ROWS) as b1, hw.build_keys_device(kR2, args, hw.BUILD_COUNT) as b2:
    sel = torch.empty((BATCH + 31) // 32 * 4, dtype=torch.uint8, device="cuda")
    F1, F2, P0, P1 = [], [], [], []
    for r in range(reps + 1):
        _, n1, m1 = hw.filter_keys_device(b1, S1, out=sel)
        _, n2, m2 = hw.filter_keys_device(b2, S2, s_valid=sel, out=sel)
        st0, rows0, _ = hw.probe_keys_pairs_device(b1, S1, capacity=CAP)
        st1, rows1, _ = hw.probe_keys_pairs_device(b1, S1, capacity=CAP, s_valid=sel)
        assert st1.filtered == n2 and n2 <= n1 == st0.filtered and rows1.shape[0] <= rows0.shape[0]
        if r:  # (the first round is the warm-up)
            F1.append(m1), F2.append(m2), P0.append(st0.ms_total), P1.append(st1.ms_total)
    say(f"star, S = 64M rows with two key columns, two builds of {nR}: filter 1 passes {n1}, both {n2}")
    say(f"star filter 1: {mmm(F1)}; filter 2 ANDed in place: {mmm(F2)}")
    say(f"star pairs probe of build 1, ms_total: without a bitmap {mmm(P0)} ({rows0.shape[0]} pairs); with the intersected bitmap "
        f"{mmm(P1)} ({rows1.shape[0]} pairs)")
say(f"copy_measured {hw.copy_bandwidth():.0f} GB/s")
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
