"""Dev: time the key-column joins with validity bitmaps (r_valid / s_valid of join_keys_device and
join_keys_pairs_device) against the same entries without bitmaps at the north-star shape (|R| = 128M,
|S| = 1024M, q = 0.01, blocked, m = 2^30, k = 1, B = 1024), in one process: the key columns cut from
generate_device's tuples, all-valid bitmaps on both sides (every byte 0xFF), one warm-up of each form,
then alternating repetitions of the unmasked and the masked form, for the counting join and for the
pairs. filtered and matches are asserted equal between the two forms in every run (and the pairs as
multisets after the last repetition). Then one run of each entry with 10 % of S's rows NULL, for the
record.

The baseline is the unmasked entry in the same run: unchanged code ("Key columns: validity
bitmaps", unchanged code). Conditions, per entry and per side: the masked scatter's median <= the
unmasked median x (1 + b) + the unmasked spread (max - min), b = the share of bytes the bitmap adds to
that kernel: 1/8 byte per element against 8 (the counting scatter: 4 read, 4 written) or about 12 (the
payload scatter: 4 read, 8 written).

Prints every run and writes medians, ranges, the phase times of the last runs and the arithmetic of
each condition to the file given as argv[1] (default profiles/keys_nulls/northstar.txt); argv[2] =
repetitions (default 7, at least 7); argv[3] (optional) = a text file appended verbatim (the
compiler's resource summary of the new kernels)."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import hwbloomradixjoin_amd as hw  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "keys_nulls", "northstar.txt")
reps = max(7, int(sys.argv[2])) if len(sys.argv) > 2 else 7
res_path = sys.argv[3] if len(sys.argv) > 3 else None
nR, nS, q = 128000000, 1024000000, 0.01


def column(n, maxid, sel, seed):
    t = torch.empty((n, 2), dtype=torch.int32, device="cuda")
    hw.generate_device(t, 2, maxid, nR, sel, seed)
    torch.cuda.synchronize()
    return t[:, 0].contiguous()


kR, kS = column(nR, nR, 1.0, 12345), column(nS, 2**31 - 1, q, 54321)
torch.cuda.synchronize()
torch.cuda.empty_cache()
allR = torch.full(((nR + 31) // 32 * 4,), 255, dtype=torch.uint8, device="cuda")
allS = torch.full(((nS + 31) // 32 * 4,), 255, dtype=torch.uint8, device="cuda")
args = hw.BloomFilterArgs(hw.BLOCKED, 1 << 30, 1, 1024)
CAP = 16 << 20  # pairs (about 10.24M at q = 0.01)
FIELDS = ("ms_total", "ms_s_scatter", "ms_r_scatter")
ENTRIES = ("count", "pairs")
SHARE = {"count": (1 / 8) / 8, "pairs": (1 / 8) / 12}


def run(entry, masks):
    kw = dict(r_valid=masks[0], s_valid=masks[1]) if masks is not None else {}
    if entry == "count":
        return hw.join_keys_device(kR, kS, args, **kw), None
    st, pairs, _ = hw.join_keys_pairs_device(kR, kS, args, capacity=CAP, **kw)
    return st, pairs


def words(pairs):
    return torch.sort(pairs.contiguous().view(torch.int64).ravel()).values


for entry in ENTRIES:  # warm-up: code objects, buffers, clocks
    for form, masks in (("plain", None), ("masked", (allR, allS))):
        st, _ = run(entry, masks)
        print(f"warm-up {entry} {form}: {st.ms_total:.3f} ms", flush=True)
runs = {(e, f): [] for e in ENTRIES for f in ("plain", "masked")}
last = {}
for r in range(reps):
    for entry in ENTRIES:
        for form, masks in (("plain", None), ("masked", (allR, allS))):
            st, pairs = run(entry, masks)
            runs[entry, form].append(st)
            last[entry, form] = (st, pairs)
            print(f"rep {r} {entry} {form}: total {st.ms_total:.3f} s_scatter {st.ms_s_scatter:.3f} r_scatter "
                  f"{st.ms_r_scatter:.3f} ms, filtered {st.filtered} matches {st.matches}", flush=True)
        a, b = last[entry, "plain"][0], last[entry, "masked"][0]
        assert (a.filtered, a.matches) == (b.filtered, b.matches), (r, entry, a, b)
pairs_equal = bool(torch.equal(words(last["pairs", "plain"][1]), words(last["pairs", "masked"][1])))
assert pairs_equal, "the masked form's pairs differ from the unmasked form's"
counts = {e: (last[e, "plain"][0].filtered, last[e, "plain"][0].matches) for e in ENTRIES}
last.clear()

# 10 % of S NULL, for the record: every pair must name a valid S row
CH = 1 << 27
vS = torch.empty(nS, dtype=torch.bool, device="cuda")
g = torch.Generator(device="cuda")
g.manual_seed(7)
for i in range(0, nS, CH):
    j = min(nS, i + CH)
    vS[i:j] = torch.rand(j - i, device="cuda", generator=g) >= 0.1
mS = hw.pack_validity(vS)
n_null = int(nS - vS.sum().item())
null_lines = []
for entry in ENTRIES:
    st, pairs = run(entry, (None, mS))
    ok = "" if pairs is None else f", every pair's S row valid: {bool(vS[pairs[:, 1].long()].all())}"
    null_lines.append(f"10 % NULLs in S ({n_null} rows), {entry}: total {st.ms_total:.3f} s_scatter {st.ms_s_scatter:.3f} "
                      f"r_scatter {st.ms_r_scatter:.3f} ms, filtered {st.filtered} matches {st.matches}{ok}")
    assert st.matches <= counts[entry][1]
    if pairs is not None:
        assert bool(vS[pairs[:, 1].long()].all())
    del pairs
print("\n".join(null_lines), flush=True)
copy = hw.copy_bandwidth()


def stat(entry, form, f):
    v = [getattr(st, f) for st in runs[entry, form]]
    return statistics.median(v), min(v), max(v)


lines = [f"key columns with validity bitmaps at the north star: |R| = {nR}, |S| = {nS}, q = {q}, blocked m = 2^30 k = 1 "
         "B = 1024",
         f"{hw.lib().hwbrj_version().decode()}",
         f"{reps} alternating repetitions per entry (plain: no bitmaps; masked: all-valid bitmaps on both sides) after one "
         "warm-up each; device ms",
         f"filtered and matches asserted equal between the two forms in every run; the pairs of the last repetition equal "
         f"as multisets: {pairs_equal}"]
for e in ENTRIES:
    lines.append(f"{e}: filtered {counts[e][0]}, matches {counts[e][1]}")
lines.append(f"{'entry':6s} {'form':7s} {'phase':13s} {'median':>9s} {'min':>9s} {'max':>9s}")
for e in ENTRIES:
    for form in ("plain", "masked"):
        for f in FIELDS:
            m, lo, hi = stat(e, form, f)
            lines.append(f"{e:6s} {form:7s} {f:13s} {m:9.3f} {lo:9.3f} {hi:9.3f}")
for e in ENTRIES:
    for form in ("plain", "masked"):
        st = runs[e, form][-1]
        lines.append(f"phases (last run) {e} {form}: r_sc {st.ms_r_scatter:.3f} r_ix {st.ms_r_index:.3f} build "
                     f"{st.ms_build:.3f} s_sc {st.ms_s_scatter:.3f} s_ix {st.ms_s_index:.3f} probe {st.ms_probe:.3f} join "
                     f"{st.ms_join:.3f}")
lines += null_lines
lines.append(f"copy_measured {copy:.0f} GB/s")
verdicts = []
for e in ENTRIES:
    b = SHARE[e]
    for f in ("ms_s_scatter", "ms_r_scatter"):
        mp, lo, hi = stat(e, "plain", f)
        mm, _, _ = stat(e, "masked", f)
        bound = mp * (1 + b) + (hi - lo)
        verdicts.append(mm <= bound)
        lines.append(f"condition ({e}): masked {f} median {mm:.3f} ms <= plain {mp:.3f} x (1 + {b:.5f}) + its spread "
                     f"{hi - lo:.3f} = {bound:.3f} ms: {'met' if mm <= bound else f'NOT met (by {mm - bound:.3f} ms)'}")
lines.append(f"verdict: {'met' if all(verdicts) else 'NOT met'}")
if res_path:
    lines.append("compiler resource summary (-Rpass-analysis=kernel-resource-usage) of the new kernels:")
    lines += open(res_path).read().rstrip("\n").split("\n")
text = "\n".join(lines) + "\n"
print(text)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
