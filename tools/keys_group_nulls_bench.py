"""Dev: time the group joins on key columns with validity bitmaps (r_valid / s_valid / sv_valid of
group_join_keys_device and group_minmax_join_keys_device) against the same entries without bitmaps
at the north-star shape (|R| = 128M, |S| = 1024M, q = 0.01, blocked, m = 2^30, k = 1, B = 1024), in
one process: the key columns cut from generate_device's tuples, S's value column a multiplicative
hash of the row index, all-valid bitmaps (every byte 0xFF). Per aggregate (sum, minmax) three forms:
"plain" (no bitmap), "skey" (S's key bitmap only: the one-bitmap scatter) and "all3" (R's keys, S's
keys and S's values: the masked R scatter, the two-bitmap S scatter, and k_null_group_rows under
GROUP_ALL). One warm-up per form, then alternating repetitions under GROUP_MATCHED; n_pairs,
filtered and the sorted rows are asserted equal between the forms in every run. Then one GROUP_ALL
run per form (counts asserted equal), and one run per aggregate with 10 % of S's values NULL.

The baseline is the unmasked entry in the same run: unchanged code ("Key columns: group
joins with validity bitmaps"). Conditions, per aggregate and masked form: the masked scatter's median
<= the plain median x (1 + b) + the plain spread (max - min), b the bitmaps' share of the scatter's
bytes per element: for the value-column S scatter 1/8 byte per bitmap against 8 read + 8 written
(1/128 with one bitmap, 1/64 with two), for the R scatter 1/8 against 4 read + 8 written (1/96).

Prints every run and writes medians, ranges, the phase times of the last runs and the arithmetic of
each condition to the file given as argv[1] (default profiles/keys_group_nulls/northstar.txt);
argv[2] = repetitions (default 7, at least 7); argv[3] (optional) = a text file appended verbatim
(the compiler's resource summary of the new kernels)."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import hwbloomradixjoin_amd as hw  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "keys_group_nulls", "northstar.txt")
reps = max(7, int(sys.argv[2])) if len(sys.argv) > 2 else 7
res_path = sys.argv[3] if len(sys.argv) > 3 else None
nR, nS, q = 128000000, 1024000000, 0.01


def column(n, maxid, sel, seed):
    t = torch.empty((n, 2), dtype=torch.int32, device="cuda")
    hw.generate_device(t, 2, maxid, nR, sel, seed)
    torch.cuda.synchronize()
    return t[:, 0].contiguous()


kR, kS = column(nR, nR, 1.0, 12345), column(nS, 2**31 - 1, q, 54321)
vS = torch.empty(nS, dtype=torch.int32, device="cuda")
CH = 1 << 26
for i in range(0, nS, CH):  # the value column: row * 0x9E3779B1 mod 2^32, as int32
    j = min(nS, i + CH)
    v = (torch.arange(i, j, dtype=torch.int64, device="cuda") * 0x9E3779B1) & 0xFFFFFFFF
    vS[i:j] = torch.where(v >= 2**31, v - 2**32, v).to(torch.int32)
del v
torch.cuda.synchronize()
torch.cuda.empty_cache()
allR = torch.full(((nR + 31) // 32 * 4,), 255, dtype=torch.uint8, device="cuda")
allS = torch.full(((nS + 31) // 32 * 4,), 255, dtype=torch.uint8, device="cuda")
allV = torch.full(((nS + 31) // 32 * 4,), 255, dtype=torch.uint8, device="cuda")
args = hw.BloomFilterArgs(hw.BLOCKED, 1 << 30, 1, 1024)
FIELDS = ("ms_total", "ms_s_scatter", "ms_r_scatter", "ms_join")
AGGS = ("sum", "minmax")
FORMS = (("plain", {}), ("skey", dict(s_valid=allS)), ("all3", dict(r_valid=allR, s_valid=allS, sv_valid=allV)))
SHARE_S = {"skey": 1 / 128, "all3": 1 / 64}
SHARE_R = 1 / 96


def run(agg, kw, kind=hw.GROUP_MATCHED):
    """(Stats, rows, n_pairs) of one group join; capacity |R| bounds the rows of either kind."""
    fn = hw.group_minmax_join_keys_device if agg == "minmax" else hw.group_join_keys_device
    st, rows, pairs, _ = fn(kR, kS, vS, args, kind=kind, capacity=nR, **kw)
    return st, rows, pairs


def sorted_rows(rows):
    """The rows as (n, 2) int64 words sorted by word 0 ({r_payload, count}; r_payload is distinct)."""
    raw = rows.raw.contiguous().view(torch.int64).reshape(-1, 2)
    return raw[torch.sort(raw[:, 0]).indices]


for agg in AGGS:  # warm-up: code objects, buffers, clocks
    for form, kw in FORMS:
        st, _, _ = run(agg, kw)
        print(f"warm-up {agg} {form}: {st.ms_total:.3f} ms", flush=True)
runs = {(a, f): [] for a in AGGS for f, _ in FORMS}
counts = {}
for r in range(reps):
    for agg in AGGS:
        base = None
        for form, kw in FORMS:
            st, rows, pairs = run(agg, kw)
            runs[agg, form].append(st)
            print(f"rep {r} {agg} {form}: total {st.ms_total:.3f} s_scatter {st.ms_s_scatter:.3f} r_scatter "
                  f"{st.ms_r_scatter:.3f} join {st.ms_join:.3f} ms, rows {st.matches} pairs {pairs} filtered {st.filtered}",
                  flush=True)
            srt = sorted_rows(rows)
            if base is None:
                base = (st.matches, pairs, st.filtered, srt)
            else:
                assert (st.matches, pairs, st.filtered) == base[:3], (r, agg, form, st, base[:3])
                assert torch.equal(srt, base[3]), f"rep {r} {agg} {form}: rows differ from the plain form's"
            del rows, srt
        counts[agg] = base[:3]
        del base
all_lines = []
for agg in AGGS:  # GROUP_ALL once per form: k_null_group_rows runs in the all3 form (and finds no NULL row)
    base = None
    for form, kw in FORMS:
        st, rows, pairs = run(agg, kw, hw.GROUP_ALL)
        lone = int((rows.count == 0).sum().item())
        all_lines.append(f"GROUP_ALL {agg} {form}: total {st.ms_total:.3f} s_scatter {st.ms_s_scatter:.3f} r_scatter "
                         f"{st.ms_r_scatter:.3f} join {st.ms_join:.3f} ms, rows {st.matches} (count 0: {lone}) pairs {pairs} "
                         f"filtered {st.filtered}")
        print(all_lines[-1], flush=True)
        assert st.matches == nR
        base = base or (st.matches, pairs, st.filtered, lone)
        assert (st.matches, pairs, st.filtered, lone) == base and (pairs, st.filtered) == counts[agg][1:]
        del rows

# 10 % of S's values NULL, for the record
vv = torch.empty(nS, dtype=torch.bool, device="cuda")
g = torch.Generator(device="cuda")
g.manual_seed(7)
CHB = 1 << 27
for i in range(0, nS, CHB):
    j = min(nS, i + CHB)
    vv[i:j] = torch.rand(j - i, device="cuda", generator=g) >= 0.1
mV = hw.pack_validity(vv)
n_null = int(nS - vv.sum().item())
del vv
null_lines = []
for agg in AGGS:
    st, rows, pairs = run(agg, dict(sv_valid=mV))
    null_lines.append(f"10 % NULL values in S ({n_null} rows), {agg}: total {st.ms_total:.3f} s_scatter {st.ms_s_scatter:.3f} "
                      f"r_scatter {st.ms_r_scatter:.3f} join {st.ms_join:.3f} ms, rows {st.matches} pairs {pairs} filtered "
                      f"{st.filtered}")
    assert pairs < counts[agg][1] and st.filtered < counts[agg][2] and st.matches <= counts[agg][0]
    del rows
print("\n".join(null_lines), flush=True)
copy = hw.copy_bandwidth()


def stat(agg, form, f):
    v = [getattr(st, f) for st in runs[agg, form]]
    return statistics.median(v), min(v), max(v)


lines = [f"group joins on key columns with validity bitmaps at the north star: |R| = {nR}, |S| = {nS}, q = {q}, blocked "
         "m = 2^30 k = 1 B = 1024",
         f"{hw.lib().hwbrj_version().decode()}",
         f"{reps} alternating repetitions per aggregate under GROUP_MATCHED (plain: no bitmap; skey: S's key bitmap; all3: "
         "R's keys, S's keys, S's values; every bitmap all valid) after one warm-up each; device ms",
         "n_pairs, filtered and the sorted rows asserted equal to the plain form's in every run"]
for a in AGGS:
    lines.append(f"{a}: rows {counts[a][0]}, n_pairs {counts[a][1]}, filtered {counts[a][2]}")
lines.append(f"{'agg':6s} {'form':6s} {'phase':13s} {'median':>9s} {'min':>9s} {'max':>9s}")
for a in AGGS:
    for form, _ in FORMS:
        for f in FIELDS:
            m, lo, hi = stat(a, form, f)
            lines.append(f"{a:6s} {form:6s} {f:13s} {m:9.3f} {lo:9.3f} {hi:9.3f}")
for a in AGGS:
    for form, _ in FORMS:
        st = runs[a, form][-1]
        lines.append(f"phases (last run) {a} {form}: r_sc {st.ms_r_scatter:.3f} r_ix {st.ms_r_index:.3f} build "
                     f"{st.ms_build:.3f} s_sc {st.ms_s_scatter:.3f} s_ix {st.ms_s_index:.3f} probe {st.ms_probe:.3f} join "
                     f"{st.ms_join:.3f}")
lines += all_lines + null_lines
lines.append(f"copy_measured {copy:.0f} GB/s")
verdicts = []
for a in AGGS:
    for form in ("skey", "all3"):
        for f, b in (("ms_s_scatter", SHARE_S[form]), ("ms_r_scatter", SHARE_R)):
            mp, lo, hi = stat(a, "plain", f)
            mk, _, _ = stat(a, form, f)
            bound = mp * (1 + b) + (hi - lo)
            verdicts.append(mk <= bound)
            lines.append(f"condition ({a}, {form}): masked {f} median {mk:.3f} ms <= plain {mp:.3f} x (1 + {b:.5f}) + its "
                         f"spread {hi - lo:.3f} = {bound:.3f} ms: "
                         f"{f'met (by {bound - mk:.3f} ms)' if mk <= bound else f'MISSED (by {mk - bound:.3f} ms)'}")
lines.append(f"verdict: {'every condition met' if all(verdicts) else 'NOT every condition met'}")
if res_path:
    lines.append("compiler resource summary (-Rpass-analysis=kernel-resource-usage) of the new kernels:")
    lines += open(res_path).read().rstrip("\n").split("\n")
text = "\n".join(lines) + "\n"
print(text)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
