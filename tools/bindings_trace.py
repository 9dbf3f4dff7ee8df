"""Dev: do two versions of hwbloomradixjoin_amd/__init__.py make the same C calls? One-off A/B record of
the Python bindings ("Python bindings"; results in profiles/py_bindings/). No kernel is
launched: the library is replaced by a recording stand-in that answers with scripted codes.
    python3 tools/bindings_trace.py [--pkg DIR] trace OUT       every wrapper under every scenario (8-row
                                                               tensors on a GPU, so that the checks pass)
    python3 tools/bindings_trace.py [--pkg DIR] signatures OUT  restype / argtypes of all that lib() declares
                                                               (needs the built library, no GPU)
    python3 tools/bindings_trace.py [--pkg DIR] api OUT         __all__, inspect.signature and a hash of
                                                               __doc__ of every public callable
    python3 tools/bindings_trace.py diff A B OUT                two trace files, scenario by scenario
A trace has one line per scenario: wrapper: scenario | the C calls in order | what the wrapper returned or raised.
--pkg DIR: the directory that holds the hwbloomradixjoin_amd package to look at (default: this tree)."""
import ctypes
import hashlib
import inspect
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HANDLE, STREAM = 0x1000, 0x5000  # a build's handle and a stream's: never dereferenced
SHORT = {"c_ulong": "u64", "c_double": "f64", "c_int": "int", "c_void_p": "ptr"}  # ctypes names in the log
ANSWERED = ("hwbrj_set_device", "hwbrj_last_error", "hwbrj_build_info", "hwbrj_build_free")
GROUP = ("group_join_device", "group_minmax_join_device", "group_join_keys_device", "group_minmax_join_keys_device",
         "group_probe_keys_device", "group_minmax_probe_keys_device", "Build.group_rows[sum]",
         "Build.group_rows[minmax]")


class Recorder:
    """Stands in for the CDLL: every attribute is a callable that logs its name and arguments and answers
    from the script, a list of (code, n) for the calls that are not in ANSWERED, (0, 3) after its end."""

    def __init__(self):
        self.lines, self.calls, self.script, self.names = [], [], [], {HANDLE: "handle", STREAM: "stream"}
        self.allocs, self.bitmaps = {}, {}  # of the scenario that runs: they name pointers while they are alive

    def __getattr__(self, name):
        return lambda *a: self.call(name, a)

    def pointer(self, p):
        if p in self.names or p in self.bitmaps:
            return self.names.get(p) or self.bitmaps[p]
        if p in self.allocs:
            t = self.allocs[p]
            return f"new{tuple(t.shape)}{str(t.dtype)[6:]}"  # a fresh output buffer: rows, columns, dtype
        return None

    def show(self, a):
        if isinstance(a, int) and not isinstance(a, bool) and a >= 0x1000:
            return self.pointer(a) or f"int {a:#x}"
        if isinstance(a, ctypes.c_void_p):
            return self.pointer(a.value) or f"c_void_p({a.value})"
        if type(a).__name__ == "CArgObject":
            return "&" + SHORT.get(type(a._obj).__name__, type(a._obj).__name__)
        if isinstance(a, ctypes.Array):
            return f"{SHORT.get(a._type_.__name__, a._type_.__name__)}[{len(a)}]"
        return repr(a)

    def call(self, name, args):
        self.calls.append(f"{name}({', '.join(self.show(a) for a in args)})")
        if name == "hwbrj_last_error":
            return b"scripted error"
        if name == "hwbrj_build_info":
            args[1][0] = 8  # nR
            return 0
        if name in ANSWERED:
            return 0
        rc, n = self.script.pop(0) if self.script else (0, 3)
        if rc in (0, 7):
            seen = 0
            for a in args:
                t = a._obj if type(a).__name__ == "CArgObject" else a
                if isinstance(t, ctypes.c_uint64):
                    t.value = n if not seen else 2 * n  # n_out, then n_pairs
                    seen += 1
                elif isinstance(t, ctypes.c_int):
                    t.value = 2  # hwbrj_join_wait_all's n_joins
                elif isinstance(t, ctypes.c_double):
                    t.value = 1.5
                elif isinstance(t, ctypes.c_void_p) and type(a).__name__ == "CArgObject":
                    t.value = HANDLE  # hwbrj_build_keys_device's build
                elif isinstance(t, ctypes.Array) and t._type_ is ctypes.c_uint64:
                    t[0], t[1], t[2] = n, 1, 2
                elif isinstance(t, ctypes.Structure) and hasattr(t, "matches"):
                    t.filtered, t.matches = 8, n
        return rc


def load(pkg):
    sys.path.insert(0, pkg)
    import hwbloomradixjoin_amd as hw
    assert os.path.dirname(os.path.dirname(os.path.abspath(hw.__file__))) == os.path.abspath(pkg), hw.__file__
    return hw


def result(rec, v):
    """A returned value, tensors by dtype, shape and (*) whether they are views of the last output buffer."""
    import torch
    if isinstance(v, torch.Tensor):
        base = next(reversed(rec.allocs.values()), None) if rec.allocs else None
        shared = base is not None and v.untyped_storage().data_ptr() == base.untyped_storage().data_ptr()
        return f"{str(v.dtype)[6:]}{tuple(v.shape)}{'*' if shared else ''}"
    if isinstance(v, tuple):
        return f"{type(v).__name__}({', '.join(result(rec, x) for x in v)})"
    if type(v).__name__ == "Stats":
        return f"Stats({v.filtered}, {v.matches})"
    if type(v).__name__ == "Build":
        h, v._h = v._h, 0  # (never a real handle: nothing to free)
        return f"Build({h:#x}, ms={v.ms})"
    if isinstance(v, list):
        return f"[{', '.join(result(rec, x) for x in v)}]"
    return repr(v)


def trace(hw, out, device):
    import torch
    rec = Recorder()
    hw._LIB = rec
    assert hw.lib() is rec
    dev = torch.device(device)
    R, S = (torch.zeros((8, 2), dtype=torch.int32, device=dev) for _ in range(2))
    Rk, Sk, Sv = (torch.zeros(8, dtype=torch.int32, device=dev) for _ in range(3))
    valid = {k: torch.ones(8, dtype=torch.bool, device=dev) for k in ("r_valid", "s_valid", "sv_valid")}
    for name, t in (("R", R), ("S", S), ("Rk", Rk), ("Sk", Sk), ("Sv", Sv)):
        rec.names[t.data_ptr()] = name
    build = hw.Build(HANDLE, dev)
    bitmaps = []

    # what the wrappers allocate and pack, so that a pointer can be named; the wait for torch's stream
    empty, pack = torch.empty, hw.pack_validity

    def rec_empty(*a, **kw):
        t = empty(*a, **kw)
        if t.numel():
            rec.allocs[t.data_ptr()] = t
        return t

    def rec_pack(v):
        b = pack(v)
        bitmaps.append(b)
        rec.bitmaps[b.data_ptr()] = next(k for k, t in valid.items() if t is v) + " bitmap"
        return b

    def rec_current_stream(d=None):
        return types.SimpleNamespace(
            synchronize=lambda: rec.calls.append("torch.cuda.current_stream().synchronize()"))

    torch.empty, hw.pack_validity, torch.cuda.current_stream = rec_empty, rec_pack, rec_current_stream

    tup = lambda f: lambda a, s, **kw: f(R, S, args=a, stream=s, **kw)  # noqa: E731
    key = lambda f: lambda a, s, **kw: f(Rk, Sk, args=a, stream=s, **kw)  # noqa: E731
    keyv = lambda f: lambda a, s, **kw: f(Rk, Sk, Sv, args=a, stream=s, **kw)  # noqa: E731
    prb = lambda f: lambda a, s, **kw: f(build, Sk, stream=s, **kw)  # noqa: E731
    prbv = lambda f: lambda a, s, **kw: f(build, Sk, Sv, stream=s, **kw)  # noqa: E731
    wrappers = [(n, form(getattr(hw, n)), inspect.signature(getattr(hw, n)).parameters) for form, names in (
        (tup, ("join_materialize_device", "semi_join_device", "outer_join_device", "group_join_device",
               "group_minmax_join_device", "join_device", "join_device_async")),
        (key, ("join_keys_pairs_device", "semi_join_keys_device", "outer_join_keys_device", "join_keys_device",
               "join_keys_device_async")),
        (keyv, ("group_join_keys_device", "group_minmax_join_keys_device")),
        (prb, ("probe_keys_pairs_device", "semi_probe_keys_device", "outer_probe_keys_device", "probe_keys_device")),
        (prbv, ("group_probe_keys_device", "group_minmax_probe_keys_device", "group_accum_probe_keys_device")),
    ) for n in names]
    def group_rows(agg, s, kind=hw.GROUP_MATCHED, **kw):  # (MATCHED unless the scenario says GROUP_ALL)
        return build.group_rows(agg, kind, stream=s, **kw)

    wrappers += [
        ("Build.unmatched_rows", lambda a, s, **kw: build.unmatched_rows(stream=s, **kw), ("capacity",)),
        ("Build.group_rows[sum]", lambda a, s, **kw: group_rows(hw.AGG_SUM, s, **kw), ("capacity",)),
        ("Build.group_rows[minmax]", lambda a, s, **kw: group_rows(hw.AGG_MINMAX, s, **kw), ("capacity",)),
        ("build_keys_device", lambda a, s, **kw: hw.build_keys_device(Rk, a, stream=s, **kw), ("r_valid",)),
        ("join_wait", lambda a, s: hw.join_wait(), ()),
        ("join_wait_all", lambda a, s: hw.join_wait_all(4), ()),
    ]

    bloom, stream = hw.BloomFilterArgs(hw.BLOCKED, 1 << 20, 1, 512), types.SimpleNamespace(cuda_stream=STREAM)
    ALL, RETRY, FAIL = {"kind": hw.GROUP_ALL}, [(7, 5), (0, 5)], [(5, 0)]
    scenarios = [  # (name, the wrapper needs these parameters, args, stream, keywords, script)
        ("capacity=None, code 0, no filter, no stream", (), None, None, {}, []),
        ("capacity=None under GROUP_ALL", ("capacity", "GROUP"), bloom, stream, ALL, []),
        ("capacity=6, sufficient", ("capacity",), bloom, stream, {"capacity": 6}, []),
        ("capacity=2 answered by 7 with n=5, then 0", ("capacity",), bloom, stream, {"capacity": 2}, RETRY),
        ("first call answered by 5", (), bloom, stream, {}, FAIL),
    ] + [(f"masked {m}", (m,), bloom, stream, {m: valid[m]}, []) for m in valid] + [
        # (every mask the wrapper takes at once: the entry named in an error, the bitmaps over a retry)
        ("all masks, first call answered by 5", ("MASKS",), bloom, stream, {}, FAIL),
        ("all masks, capacity=2 answered by 7 with n=5, then 0", ("MASKS", "capacity"), bloom, stream, {"capacity": 2},
         RETRY),
    ]

    for wname, fn, params in wrappers:
        mine = {m: valid[m] for m in valid if m in params}
        for sname, needs, a, s, kw, script in scenarios:
            if not all(p in params or (p == "GROUP" and wname in GROUP) or (p == "MASKS" and mine) for p in needs):
                continue
            rec.script, rec.calls, rec.allocs, rec.bitmaps = list(script), [], {}, {}
            del bitmaps[:]
            try:
                end = f"-> {result(rec, fn(a, s, **kw, **(mine if 'MASKS' in needs else {})))}"
            except Exception as e:  # noqa: BLE001 (the text is the record)
                end = f"raised {type(e).__name__}: {e}"
            rec.lines.append(f"{wname}: {sname} | {'; '.join(rec.calls)} | {end}")
    build._h = 0
    torch.empty, hw.pack_validity = empty, pack
    with open(out, "w") as f:
        f.write("\n".join(rec.lines) + "\n")
    print(f"bindings_trace: {len(rec.lines)} scenarios of {len(wrappers)} wrappers -> {out}")


def signatures(hw, out):
    L = hw.lib()
    nm = lambda t: getattr(t, "__name__", repr(t))  # noqa: E731
    with open(out, "w") as f:
        for name, fn in sorted(vars(L).items()):
            if isinstance(fn, ctypes._CFuncPtr):
                at = "unset" if fn.argtypes is None else f"[{', '.join(nm(t) for t in fn.argtypes)}]"
                f.write(f"{name}: restype {nm(fn.restype)}, argtypes {at}\n")


def api(hw, out):
    def line(name, fn):
        doc = hashlib.sha1((fn.__doc__ or "").encode()).hexdigest()[:12]
        try:
            sig = str(inspect.signature(fn))
        except (TypeError, ValueError):
            sig = "(no signature)"
        return f"{name}{sig}  doc {doc}\n"

    with open(out, "w") as f:
        f.write(f"__all__ = {hw.__all__}\n")
        for name, v in sorted(vars(hw).items()):
            if name.startswith("_") or getattr(v, "__module__", None) != hw.__name__ or not callable(v):
                continue
            f.write(line(name, v))
            if inspect.isclass(v):
                for m, fn in sorted(vars(v).items()):
                    if callable(fn) or isinstance(fn, (property, classmethod, staticmethod)):
                        fn = fn.fget if isinstance(fn, property) else getattr(fn, "__func__", fn)
                        f.write(line(f"{name}.{m}", fn))


def diff(a, b, out):
    """Two traces, scenario by scenario (a line each: name | calls | outcome): the calls and outcomes that differ."""
    import difflib
    sa, sb = ({ln.split(" | ")[0]: ln.split(" | ")[1:] for ln in open(p).read().splitlines()} for p in (a, b))
    with open(out, "w") as f:
        f.write(f"--- {a}\n+++ {b}\n{len(sa)} / {len(sb)} scenarios\n")
        for head in list(sa) + [h for h in sb if h not in sa]:
            if head not in sa or head not in sb:
                f.write(f"{head}\n  only in {b if head not in sa else a}\n")
            elif sa[head] != sb[head]:
                la, lb = (x[0].split("; ") + x[1:] for x in (sa[head], sb[head]))
                f.write(head + "\n" + "".join(f"{d}\n" for d in difflib.ndiff(la, lb) if d[0] in "+-"))
    print(open(out).read(), end="")


if __name__ == "__main__":
    argv = sys.argv[1:]
    pkg, device = ROOT, "cuda:0"
    while argv and argv[0] in ("--pkg", "--device"):
        if argv[0] == "--pkg":
            pkg = argv[1]
        else:
            device = argv[1]  # (dev: another device for the 8-row tensors)
        argv = argv[2:]
    if argv[0] == "diff":
        diff(*argv[1:4])
    else:
        {"trace": lambda hw, o: trace(hw, o, device), "signatures": signatures, "api": api}[argv[0]](load(pkg), argv[1])
