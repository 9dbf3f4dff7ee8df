"""Dev: do two builds of libhwbrj.so launch the same kernels? One synchronous join of every family of
tests/seq_catalog.py under every config of its smallest relation set (each checked as in
tests/test_gpu_sequences.py), three back-to-back async counting joins, and one host BPRO with
materialized pairs (reserve, then the join). Run it once per library (HWBRJ_LIB) under a kernel trace,
    rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python3 tools/enqueue_trace.py
then compare the two traces section by section (a family, the async joins, BPRO), per queue in
dispatch order, on kernel name, grid, workgroup size and LDS bytes (durations are not compared):
    python3 tools/enqueue_trace.py DIR_A DIR_B"""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import seq_catalog as sc  # noqa: E402

SECTIONS = sc.FAMILY_NAMES + ("async_x3", "host_bpro")
MARK = "sin_kernel_cuda"  # the section boundary: a dispatch no join makes, between two synchronisations


def run():
    import torch
    import hwbloomradixjoin_amd as hw
    import test_gpu_sequences as tg
    from oracle import pyoracle as orc
    sc.SET_NAMES = ("A",)  # (the references and device inputs of the smallest set only)
    env, mark, prev = tg.Env(hw, torch, orc), torch.zeros(1, dtype=torch.float64, device="cuda:0"), None
    for name in SECTIONS:
        torch.cuda.synchronize()
        mark.sin_()
        torch.cuda.synchronize()
        if name == "async_x3":
            for c in ("blocked_packed", "nobloom", "basic_k3"):
                tg.enqueue(env, ("count_t_async", c, "A"))
            assert len(hw.join_wait_all()) == 3
        elif name == "host_bpro":
            s = sc.relset("A")
            hw.set_materialize(True)
            res = hw.BPRO(hw.Relation(s.R), hw.Relation(s.S), 8, env.args["blocked_packed"])
            assert res.totalresults == res.pairs.shape[0] == sc.expect(orc, "pairs_t", "A").n
        else:
            for c in (c for c in sc.CONFIG_NAMES if sc.is_step(name, c)):
                tg.run_step(env, (name, c, "A"), prev)
                prev = (name, c, "A")
    torch.cuda.synchronize()
    print("enqueue_trace: ran", len(SECTIONS), "sections on", os.environ.get("HWBRJ_LIB") or "the tree's library")


def sections(d):
    """The trace of directory d: per section, per queue (numbered by first appearance), its dispatches."""
    path, = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    rows = sorted(csv.DictReader(open(path)), key=lambda r: (int(r["Start_Timestamp"]), int(r["Dispatch_Id"])))
    out, queues = [], {}
    for r in rows:
        if MARK in r["Kernel_Name"]:
            out.append({})
        elif out:
            q = queues.setdefault(r["Queue_Id"], len(queues))
            shape = tuple(int(r[k + a]) for k in ("Grid_Size_", "Workgroup_Size_") for a in "XYZ")
            out[-1].setdefault(q, []).append((r["Kernel_Name"], shape, int(r["LDS_Block_Size"])))
    assert len(out) == len(SECTIONS), f"{path}: {len(out)} sections"
    return out


def compare(a, b):
    same = True
    for name, sa, sb in zip(SECTIONS, sections(a), sections(b)):
        n = sum(len(v) for v in sa.values())
        diff = next(((q, i, x, y) for q in sorted(set(sa) | set(sb))
                     for i, (x, y) in enumerate(zip(sa.get(q, []) + [None], sb.get(q, []) + [None])) if x != y), None)
        if diff or sorted(sa) != sorted(sb):
            same = False
        print(f"{name:14s} {n:5d} dispatches on {len(sa)} queues  " +
              ("identical" if not diff else "FIRST DIFFERENCE queue %d dispatch %d: %s | %s" % diff))
    print("ALL IDENTICAL" if same else "DIFFERENT")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(compare(*sys.argv[1:3]) if len(sys.argv) > 2 else run())
