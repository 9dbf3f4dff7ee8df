"""Dev: time the group accumulators of a prepared build (group_accum_probe_keys_device +
Build.group_rows) against the path they replace, at the north-star shape (key columns, |R| = 128M,
blocked, m = 2^30, k = 1, B = 1024, q = 0.01), S streamed as 16 batches of 64M rows with an int32 value
column, both forms, in one process.

 baseline  16 group_probe_keys_device / group_minmax_probe_keys_device (GROUP_MATCHED) calls, each
           batch's rows combined into per-R-row tensors with torch (index_add_ for count and sum,
           scatter_reduce_ amin / amax for min and max). Time: the probes' ms plus CUDA events around
           each combine.
 new       16 accumulating probes and one Build.group_rows(GROUP_MATCHED). Time: their ms.

7 alternating repetitions after one warm-up each; the two results are asserted equal in every
repetition. Reported, not preset: new total <= baseline total + the baseline's own spread (max - min
over its repetitions); and, per batch, the accumulating probe's ms_join against the MATCHED probe's on
the same build and batch.

Prints every run and writes the tables to argv[1] (default profiles/group_accum/northstar.txt);
argv[2] = repetitions (default 7, at least 7)."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import hwbloomradixjoin_amd as hw  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "group_accum", "northstar.txt")
reps = max(7, int(sys.argv[2])) if len(sys.argv) > 2 else 7
nR, nS, q = 128000000, 1024000000, 0.01
NB = 16
BATCH = nS // NB
assert BATCH * NB == nS and BATCH % 32 == 0


def columns(n, maxid, sel, seed, payload=False):
    t = torch.empty((n, 2), dtype=torch.int32, device="cuda")
    hw.generate_device(t, 2, maxid, nR, sel, seed)
    torch.cuda.synchronize()
    return (t[:, 0].contiguous(), t[:, 1].contiguous()) if payload else t[:, 0].contiguous()


kR = columns(nR, nR, 1.0, 12345)
kS, vS = columns(nS, 2**31 - 1, q, 54321, payload=True)
vS -= nS // 2  # (values of both signs)
torch.cuda.synchronize()
torch.cuda.empty_cache()
args = hw.BloomFilterArgs(hw.BLOCKED, 1 << 30, 1, 1024)
CAP = 4 << 20  # rows of one batch (about 0.64M R rows have a partner in a batch at q = 0.01)
lines = [f"group accumulators at the north star: |R| = {nR}, S = {NB} batches of {BATCH}, q = {q}, blocked m = 2^30 k = 1 "
         f"B = 1024, key columns with an int32 value column",
         hw.lib().hwbrj_version().decode(), f"{reps} alternating repetitions after one warm-up each; device ms"]


def say(s):
    print(s, flush=True)
    lines.append(s)


def med(v):
    return statistics.median(v)


batches = [(kS[i * BATCH:(i + 1) * BATCH], vS[i * BATCH:(i + 1) * BATCH]) for i in range(NB)]
b = hw.build_keys_device(kR, args, hw.BUILD_ROWS)
say(f"build: {b.ms:.3f} ms, {b.info()['bytes'] / 2**20:.1f} MiB held before the accumulators")
FORMS = (("sum", hw.AGG_SUM, hw.group_probe_keys_device), ("minmax", hw.AGG_MINMAX, hw.group_minmax_probe_keys_device))


def baseline(form, probe):
    """(ms of the probes, ms of the combines, per-batch ms_join, the combined per-R-row tensors)."""
    cnt = torch.zeros(nR, dtype=torch.int64, device="cuda")
    if form == "sum":
        agg = (torch.zeros(nR, dtype=torch.int64, device="cuda"),)
    else:
        agg = (torch.full((nR,), 2**31 - 1, dtype=torch.int32, device="cuda"),
               torch.full((nR,), -2**31, dtype=torch.int32, device="cuda"))
    t_probe, t_comb, joins = 0.0, 0.0, []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for Sk, Sv in batches:
        st, rows, _, ms = probe(b, Sk, Sv, hw.GROUP_MATCHED, capacity=CAP)
        t_probe += ms
        joins.append(st.ms_join)
        e0.record()
        idx = rows.r_payload.to(torch.int64)
        cnt.index_add_(0, idx, rows.count)
        if form == "sum":
            agg[0].index_add_(0, idx, rows.sum)
        else:
            agg[0].scatter_reduce_(0, idx, rows.min, "amin")
            agg[1].scatter_reduce_(0, idx, rows.max, "amax")
        e1.record()
        e1.synchronize()
        t_comb += e0.elapsed_time(e1)
    return t_probe, t_comb, joins, (cnt,) + agg


def streamed(form, agg):
    """(ms of the accumulating probes, ms of group_rows, per-batch ms_join, the rows)."""
    b.reset_group(agg)
    t_probe, joins = 0.0, []
    for Sk, Sv in batches:
        st, _, _, ms = hw.group_accum_probe_keys_device(b, Sk, Sv, agg)
        t_probe += ms
        joins.append(st.ms_join)
    rows, pairs, ms = b.group_rows(agg, hw.GROUP_MATCHED)
    return t_probe, ms, joins, rows, pairs


def same(form, base, rows, pairs):
    cnt = base[0]
    at = torch.nonzero(cnt).ravel()
    order = torch.argsort(rows.r_payload)
    assert at.numel() == rows.r_payload.numel() and torch.equal(rows.r_payload[order].to(torch.int64), at)
    assert torch.equal(rows.count[order], cnt[at]) and int(cnt.sum()) == pairs
    if form == "sum":
        assert torch.equal(rows.sum[order], base[1][at])
    else:
        assert torch.equal(rows.min[order], base[1][at]) and torch.equal(rows.max[order], base[2][at])
    return at.numel()


verdicts = []
for form, agg, probe in FORMS:
    say("")
    say(f"form {form}")
    wb, wn = baseline(form, probe), streamed(form, agg)
    say(f"warm-up: baseline {wb[0] + wb[1]:.3f} ms, new {wn[0] + wn[1]:.3f} ms; the build holds {b.info()['bytes'] / 2**20:.1f} MiB")
    B, N = [], []
    for r in range(reps):
        x, y = baseline(form, probe), streamed(form, agg)
        n_rows = same(form, x[3], y[3], y[4])
        B.append(x)
        N.append(y)
        print(f"rep {r} {form}: baseline probes {x[0]:.3f} + combine {x[1]:.3f} ms; new probes {y[0]:.3f} + rows {y[1]:.3f} ms; "
              f"{n_rows} rows, {y[4]} pairs", flush=True)
    bt, nt = [x[0] + x[1] for x in B], [y[0] + y[1] for y in N]
    spread = max(bt) - min(bt)
    say(f"{form}: {n_rows} R rows with a partner, {N[-1][4]} pairs over the stream")
    say(f"{form} baseline: {NB} MATCHED probes median {med([x[0] for x in B]):.3f} ms + torch combine median "
        f"{med([x[1] for x in B]):.3f} ms; total median {med(bt):.3f} (min {min(bt):.3f}, max {max(bt):.3f})")
    say(f"{form} new:      {NB} accumulating probes median {med([y[0] for y in N]):.3f} ms + group_rows median "
        f"{med([y[1] for y in N]):.3f} ms; total median {med(nt):.3f} (min {min(nt):.3f}, max {max(nt):.3f})")
    ok = med(nt) <= med(bt) + spread
    verdicts.append(ok)
    say(f"condition ({form}): new {med(nt):.3f} <= baseline {med(bt):.3f} + its spread {spread:.3f} = {med(bt) + spread:.3f} ms: "
        f"{'met' if ok else f'MISSED (by {med(nt) - med(bt) - spread:.3f} ms)'}")
    jb = [med([x[2][i] for x in B]) for i in range(NB)]
    jn = [med([y[2][i] for y in N]) for i in range(NB)]
    say(f"{form} ms_join per batch, medians over the repetitions: MATCHED probe mean {sum(jb) / NB:.4f} (min {min(jb):.4f}, max "
        f"{max(jb):.4f}); accumulating probe mean {sum(jn) / NB:.4f} (min {min(jn):.4f}, max {max(jn):.4f}); difference "
        f"{(sum(jn) - sum(jb)) / NB:+.4f} ms per batch")
    say("  batch    " + " ".join(f"{i:7d}" for i in range(NB)))
    say("  MATCHED  " + " ".join(f"{v:7.4f}" for v in jb))
    say("  accum    " + " ".join(f"{v:7.4f}" for v in jn))
say("")
say(f"verdict: {'met' if all(verdicts) else 'MISSED'}")
say(f"copy_measured {hw.copy_bandwidth():.0f} GB/s")
b.free()
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
