"""Dev: time the prepared builds (build_keys_device + the probes) against the one-shot key-column
entries at the north-star shape (|R| = 128M, |S| = 1024M, q = 0.01, blocked, m = 2^30, k = 1,
B = 1024), in one process, the key columns cut from generate_device's tuples.

1. North star, counting join and pairs join: 7 alternating repetitions of the one-shot entry and the
   probe of a build made once, after one warm-up each. filtered and matches are asserted equal in every
   run. T = the one-shot's median ms_total, R = the median of its ms_r_scatter + ms_r_index + ms_build,
   s = its max - min. The probe runs the same S-pass, probe and join kernels at the same shapes, so the
   condition is: probe median <= T - R + s. A miss is recorded as a miss, with the phase times.
2. Streaming: the same R probed with 16 batches of 64M rows of S, against 16 one-shot joins of the same
   batches: both totals, the per-batch phases, the build's time and bytes. No threshold.
3. Marks, on one 64M batch: the probes' ms_join under OUTER_S, PROBE_MARK_S, pairs and
   PROBE_MARK_INNER (what the marks cost over the kernel without them), and the final
   unmatched_rows pass. No threshold.

Prints every run and writes the tables to argv[1] (default profiles/prepared_build/northstar.txt);
argv[2] = repetitions (default 7, at least 7)."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import hwbloomradixjoin_amd as hw  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "prepared_build", "northstar.txt")
reps = max(7, int(sys.argv[2])) if len(sys.argv) > 2 else 7
nR, nS, q = 128000000, 1024000000, 0.01
NB = 16
BATCH = nS // NB
assert BATCH * NB == nS and BATCH % 32 == 0


def column(n, maxid, sel, seed):
    t = torch.empty((n, 2), dtype=torch.int32, device="cuda")
    hw.generate_device(t, 2, maxid, nR, sel, seed)
    torch.cuda.synchronize()
    return t[:, 0].contiguous()


kR, kS = column(nR, nR, 1.0, 12345), column(nS, 2**31 - 1, q, 54321)
torch.cuda.synchronize()
torch.cuda.empty_cache()
args = hw.BloomFilterArgs(hw.BLOCKED, 1 << 30, 1, 1024)
CAP = 16 << 20  # pairs (about 10.24M at q = 0.01)
PHASES = ("ms_r_scatter", "ms_r_index", "ms_build", "ms_s_scatter", "ms_s_index", "ms_probe", "ms_join", "ms_total")
lines = [f"prepared builds at the north star: |R| = {nR}, |S| = {nS}, q = {q}, blocked m = 2^30 k = 1 B = 1024, key columns",
         hw.lib().hwbrj_version().decode(), f"{reps} alternating repetitions after one warm-up each; device ms"]


def say(s):
    print(s, flush=True)
    lines.append(s)


def phases(st):
    return " ".join(f"{p[3:]} {getattr(st, p):.3f}" for p in PHASES)


def med(v):
    return statistics.median(v)


bc = hw.build_keys_device(kR, args, hw.BUILD_COUNT)
br = hw.build_keys_device(kR, args, hw.BUILD_ROWS)
ic, ir = bc.info(), br.info()
say(f"builds: count {bc.ms:.3f} ms, {ic['bytes'] / 2**20:.1f} MiB held, join-key bits {ic['join_key_bits']}; rows "
    f"{br.ms:.3f} ms, {ir['bytes'] / 2**20:.1f} MiB held")


def one_shot(entry, S):
    if entry == "count":
        return hw.join_keys_device(kR, S, args)
    return hw.join_keys_pairs_device(kR, S, args, capacity=CAP)[0]


def probe(entry, S):
    if entry == "count":
        return hw.probe_keys_device(bc, S)
    return hw.probe_keys_pairs_device(br, S, capacity=CAP)[0]


# ---------------------------------------------------------------- 1. the north star
say("")
say("1. north star (the whole S in one batch)")
verdicts = []
for entry in ("count", "pairs"):
    for name, fn in (("one-shot", one_shot), ("probe", probe)):
        say(f"warm-up {entry} {name}: {fn(entry, kS).ms_total:.3f} ms")
    one, prb = [], []
    for r in range(reps):
        a, b = one_shot(entry, kS), probe(entry, kS)
        assert (a.filtered, a.matches, a.join_key_bits) == (b.filtered, b.matches, b.join_key_bits), (entry, r, a, b)
        assert b.ms_r_scatter == b.ms_r_index == b.ms_build == 0
        one.append(a)
        prb.append(b)
        print(f"rep {r} {entry}: one-shot {a.ms_total:.3f} probe {b.ms_total:.3f} ms, filtered {a.filtered} matches "
              f"{a.matches}", flush=True)
    T = med([s.ms_total for s in one])
    Rm = med([s.ms_r_scatter + s.ms_r_index + s.ms_build for s in one])
    spread = max(s.ms_total for s in one) - min(s.ms_total for s in one)
    P = med([s.ms_total for s in prb])
    bound = T - Rm + spread
    verdicts.append(P <= bound)
    say(f"{entry}: filtered {one[-1].filtered}, matches {one[-1].matches}")
    say(f"{entry} one-shot ms_total median {T:.3f} (min {min(s.ms_total for s in one):.3f}, max "
        f"{max(s.ms_total for s in one):.3f}); its R side (r_scatter + r_index + build) median {Rm:.3f}")
    say(f"{entry} probe    ms_total median {P:.3f} (min {min(s.ms_total for s in prb):.3f}, max "
        f"{max(s.ms_total for s in prb):.3f})")
    for p in PHASES:
        say(f"  {entry} {p[3:]:10s} one-shot {med([getattr(s, p) for s in one]):8.3f}   probe "
            f"{med([getattr(s, p) for s in prb]):8.3f}")
    say(f"condition ({entry}): probe median {P:.3f} <= T {T:.3f} - R {Rm:.3f} + s {spread:.3f} = {bound:.3f} ms: "
        f"{'met' if P <= bound else f'MISSED (by {P - bound:.3f} ms)'}")
say(f"verdict: {'met' if all(verdicts) else 'MISSED'}")

# ---------------------------------------------------------------- 2. streaming
say("")
say(f"2. streaming: {NB} batches of {BATCH} rows of S")
batches = [kS[i * BATCH:(i + 1) * BATCH] for i in range(NB)]
for entry, build in (("count", bc), ("pairs", br)):
    one_shot(entry, batches[0]), probe(entry, batches[0])  # warm-up at the batch shape
    tot_one, tot_prb = [], []
    for r in range(reps):
        a = [one_shot(entry, b) for b in batches]
        p = [probe(entry, b) for b in batches]
        for x, y in zip(a, p):
            assert (x.filtered, x.matches) == (y.filtered, y.matches), (entry, r, x, y)
        tot_one.append(sum(s.ms_total for s in a))
        tot_prb.append(sum(s.ms_total for s in p))
        print(f"rep {r} {entry}: {NB} one-shot joins {tot_one[-1]:.3f} ms, {NB} probes {tot_prb[-1]:.3f} ms", flush=True)
    matches = sum(s.matches for s in a)
    say(f"{entry}: matches over the batches {matches}")
    say(f"{entry} {NB} one-shot joins: total median {med(tot_one):.3f} ms (min {min(tot_one):.3f}, max {max(tot_one):.3f})")
    say(f"{entry} build + {NB} probes: build {build.ms:.3f} ms + probes median {med(tot_prb):.3f} ms (min "
        f"{min(tot_prb):.3f}, max {max(tot_prb):.3f}) = {build.ms + med(tot_prb):.3f} ms; the build holds "
        f"{build.info()['bytes'] / 2**20:.1f} MiB")
    say(f"  per batch, last repetition, batch {NB // 2}: one-shot {phases(a[NB // 2])}")
    say(f"  per batch, last repetition, batch {NB // 2}: probe    {phases(p[NB // 2])}")

# ---------------------------------------------------------------- 3. marks
say("")
say(f"3. marks: one batch of {BATCH} rows; probes of the rows build")
S0 = batches[0]
OCAP = BATCH + (4 << 20)
KINDS = (("pairs", None), ("OUTER_S", hw.OUTER_S), ("PROBE_MARK_INNER", hw.PROBE_MARK_INNER), ("PROBE_MARK_S", hw.PROBE_MARK_S))


def outer(kind):
    if kind is None:
        return hw.probe_keys_pairs_device(br, S0, capacity=OCAP)[0]
    return hw.outer_probe_keys_device(br, S0, kind, capacity=OCAP)[0]


for name, kind in KINDS:
    outer(kind)
mk = {name: [] for name, _ in KINDS}
for r in range(reps):
    for name, kind in KINDS:
        mk[name].append(outer(kind))
for name, _ in KINDS:
    v = mk[name]
    say(f"{name:17s} rows {v[-1].matches:10d}  ms_join median {med([s.ms_join for s in v]):.3f} (min "
        f"{min(s.ms_join for s in v):.3f}, max {max(s.ms_join for s in v):.3f})  ms_total median "
        f"{med([s.ms_total for s in v]):.3f}")
un = [br.unmatched_rows(capacity=nR) for _ in range(reps)]
say(f"unmatched_rows after the batch: {un[-1][0].shape[0]} of {nR} R rows, median {med([u[1] for u in un]):.3f} ms (min "
    f"{min(u[1] for u in un):.3f}, max {max(u[1] for u in un):.3f})")
pairs_rows = mk["pairs"][-1].matches
assert mk["PROBE_MARK_INNER"][-1].matches == pairs_rows and mk["PROBE_MARK_S"][-1].matches == mk["OUTER_S"][-1].matches
say(f"copy_measured {hw.copy_bandwidth():.0f} GB/s")
bc.free()
br.free()
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
