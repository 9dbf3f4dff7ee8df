"""hwbloomradixjoin_amd -- MI355X-native bloom-filtered radix hash join.

Python mirror of the reference's operator interface for the BPRO path
(Briimbo/HwBloomRadixJoin src/parallel_radix_join_bloom.h:34-36, src/parallel_radix_join.h:33-34,
src/bloom_filter.h:10,50-55, src/types.h:37-63), bound over ctypes to the C-ABI library
``libhwbrj.so`` (include/hwbrj.h). The join runs only in the HIP kernels of that library: if the
library is missing this package raises instead of falling back to anything on the CPU.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
from dataclasses import dataclass
from typing import NamedTuple, Optional

import numpy as np

__all__ = [
    "BASIC", "BLOCKED", "SECTORIZED", "BloomFilterArgs", "Relation", "Result", "Stats",
    "BPRO", "PRO", "join_materialize_device", "semi_join_device", "JOIN_SEMI", "JOIN_ANTI", "outer_join_device", "OUTER_S", "OUTER_R", "OUTER_FULL", "group_join_device", "GROUP_MATCHED", "GROUP_ALL", "GroupRows", "group_minmax_join_device", "GroupMinMaxRows", "group_join_keys_device", "group_minmax_join_keys_device", "set_materialize", "set_gpus", "BPRH", "BPRHO", "BRJ", "PRH", "PRHO", "RJ", "assert_args", "join_device", "join_device_async", "join_keys_device", "join_keys_device_async", "join_keys_pairs_device", "semi_join_keys_device", "outer_join_keys_device", "join_wait", "join_wait_all", "set_async_timing", "generate_device", "generate_device_range",
    "pack_validity", "generate_host", "nonunique_threshold", "create_relation_nonunique",
    "create_relation_nonunique_from_pk", "create_relation_fk_from_pk", "create_relation_zipf",
    "rand_stream", "reference_relations", "create_relation_zipf_device",
    "Build", "build_keys_device", "BUILD_COUNT", "BUILD_ROWS", "PROBE_MARK_INNER", "PROBE_MARK_S",
    "probe_keys_device", "probe_keys_pairs_device", "semi_probe_keys_device", "outer_probe_keys_device",
    "group_probe_keys_device", "group_minmax_probe_keys_device",
    "AGG_SUM", "AGG_MINMAX", "group_accum_probe_keys_device",
    "filter_keys_device",
    "export_filter", "tables_info", "tables_read", "hash_crc", "hash_crapwow", "lib", "LIB_PATH", "shard_range", "write_relation",
]

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HWBRJ_LIB") or os.path.join(PKG_DIR, "libhwbrj.so")  # HWBRJ_LIB: dev-only variant builds
CLI_PATH = os.path.join(PKG_DIR, "mchashjoins")

# src/bloom_filter.h:10 (BASIC, BLOCKED) + this build's SECTORIZED
BASIC, BLOCKED, SECTORIZED = 0, 1, 2
_VARIANTS = {"basic": BASIC, "blocked": BLOCKED, "sectorized": SECTORIZED}


class _Tuple(ctypes.Structure):  # src/types.h:37-40
    _fields_ = [("key", ctypes.c_int32), ("payload", ctypes.c_int32)]


class _Relation(ctypes.Structure):  # src/types.h:46-49
    _fields_ = [("tuples", ctypes.POINTER(_Tuple)), ("num_tuples", ctypes.c_uint64)]


class _Result(ctypes.Structure):  # src/types.h:59-63
    _fields_ = [("totalresults", ctypes.c_int64), ("resultlist", ctypes.c_void_p),
                ("nthreads", ctypes.c_int)]


class _BloomArgs(ctypes.Structure):  # src/bloom_filter.h:50-55
    _fields_ = [("variant", ctypes.c_int), ("m", ctypes.c_uint64), ("k", ctypes.c_uint64),
                ("B", ctypes.c_uint64)]


class _Stats(ctypes.Structure):  # include/hwbrj.h hwbrj_stats_t
    _fields_ = [("filtered", ctypes.c_uint64), ("matches", ctypes.c_int64), ("mode", ctypes.c_int),
                ("format", ctypes.c_int), ("partitions", ctypes.c_uint32),
                ("subparts", ctypes.c_uint32), ("slice_segments", ctypes.c_uint32)] + [
                    (n, ctypes.c_double) for n in (
                        "ms_total", "ms_r_scatter", "ms_r_index", "ms_build", "ms_s_scatter",
                        "ms_s_index", "ms_probe", "ms_surv", "ms_join", "ms_join_probe")] + [
                    ("join_keys", ctypes.c_int), ("unstaged_items", ctypes.c_uint32),
                    ("join_key_bits", ctypes.c_uint32)]

# hwbrj_stats_t.join_keys (include/hwbrj.h): the key format between the build / probe and the join
JOIN_KEYS_32, JOIN_KEYS_PACKED, JOIN_KEYS_MIXED = 0, 1, 2


def _signatures():
    """What lib() declares: one (entry, restype, argtypes) row per entry; argtypes None leaves them unset.
    A wrong row corrupts memory silently on the first call: tests/test_bindings_abi.py holds every
    hwbrj_* row against its prototype in include/hwbrj.h."""
    P = ctypes.POINTER
    ci, i32, u32, i64, u64 = ctypes.c_int, ctypes.c_int32, ctypes.c_uint32, ctypes.c_int64, ctypes.c_uint64
    dbl, vp, cstr = ctypes.c_double, ctypes.c_void_p, ctypes.c_char_p
    pu64, pdb, pst, pba, prel, pres = P(u64), P(dbl), P(_Stats), P(_BloomArgs), P(_Relation), P(_Result)

    def valid(a):  # the validity-bitmap form: d_Rvalid before nR, d_Svalid before nS
        return [a[0], vp, a[1], a[2], vp] + a[3:]

    def values(a, masked=False):  # the value column of a group join: d_Svals (and its bitmap) before nS
        i = 5 if masked else 3
        return a[:i] + ([vp, vp] if masked else [vp]) + a[i:]

    rel = [vp, u64, vp, u64]                       # d_R, nR, d_S, nS: tuples or key columns
    out, tail = [vp, u64, pu64], [vp, pst, pdb]    # d_out, capacity, n_out; stream, stats, ms
    count, enqueue = rel + [pba, ci, vp, pst], rel + [vp, vp]   # (args, algorithm); args, stream
    pairs, semi = rel + [pba] + out + tail, rel + [pba, ci] + out + tail   # (kind)
    outer = rel + [pba, ci] + out + [pu64] + tail  # (kind, n_class); the group joins' too (kind, n_pairs)
    probe, vprobe = [vp, vp, vp, u64], [vp, vp, vp, vp, vp, u64]   # build, d_Skeys, d_Svalid(, d_Svals, its bitmap), nS
    bpro, pro, from_pk = [prel, prel, ci, pba], [prel, prel, ci], [vp, u64, vp, u64, i64, dbl, u32]
    return [
        ("BPRO", pres, bpro), ("BPRH", pres, bpro), ("BPRHO", pres, bpro), ("BRJ", pres, bpro),
        ("PRO", pres, pro), ("PRH", pres, pro), ("PRHO", pres, pro), ("RJ", pres, pro),
        ("assert_args", ci, [pba]),
        ("hwbrj_join_device", ci, rel + [pba, vp, pst]),
        ("hwbrj_join_device_algo", ci, count),
        ("hwbrj_join_device_async", ci, enqueue),
        ("hwbrj_join_wait", ci, [vp]),
        ("hwbrj_join_wait_all", ci, [vp, ci, P(ci)]),
        ("hwbrj_set_async_timing", ci, [ci]),
        ("hwbrj_join_materialize_device", ci, pairs),
        ("hwbrj_join_semi_device", ci, semi),
        ("hwbrj_join_outer_device", ci, rel + [pba, ci, i32] + out + [pu64] + tail),   # (null_payload)
        ("hwbrj_join_group_device", ci, outer),
        ("hwbrj_join_group_minmax_device", ci, outer),
        ("hwbrj_join_keys_device", ci, count),
        ("hwbrj_join_keys_device_async", ci, enqueue),
        ("hwbrj_join_keys_pairs_device", ci, pairs),
        ("hwbrj_join_keys_semi_device", ci, semi),
        ("hwbrj_join_keys_outer_device", ci, outer),
        ("hwbrj_join_keys_group_device", ci, values(outer)),
        ("hwbrj_join_keys_group_minmax_device", ci, values(outer)),
        ("hwbrj_join_keys_nulls_device", ci, valid(count)),
        ("hwbrj_join_keys_pairs_nulls_device", ci, valid(pairs)),
        ("hwbrj_join_keys_semi_nulls_device", ci, valid(semi)),
        ("hwbrj_join_keys_outer_nulls_device", ci, valid(outer)),
        ("hwbrj_join_keys_group_nulls_device", ci, values(valid(outer), masked=True)),
        ("hwbrj_join_keys_group_minmax_nulls_device", ci, values(valid(outer), masked=True)),
        # prepared builds: the build's handle first, then the counterpart's S-side arguments
        ("hwbrj_build_keys_device", ci, [vp, vp, u64, pba, ci, vp, P(vp), pdb]),
        ("hwbrj_build_free", ci, [vp]),
        ("hwbrj_build_info", ci, [vp, pu64, ci]),
        ("hwbrj_build_export_filter", ci, [vp, vp, u64]),
        ("hwbrj_build_unmatched_device", ci, [vp] + out + [vp, pdb]),
        ("hwbrj_build_reset_marks", ci, [vp]),
        ("hwbrj_probe_keys_device", ci, probe + [ci, vp, pst]),
        ("hwbrj_probe_keys_pairs_device", ci, probe + out + tail),
        ("hwbrj_probe_keys_semi_device", ci, probe + [ci] + out + tail),
        ("hwbrj_probe_keys_outer_device", ci, probe + [ci] + out + [pu64] + tail),
        ("hwbrj_probe_keys_group_device", ci, vprobe + [ci] + out + [pu64] + tail),
        ("hwbrj_probe_keys_group_minmax_device", ci, vprobe + [ci] + out + [pu64] + tail),
        ("hwbrj_probe_keys_group_accum_device", ci, vprobe + [ci, pu64, pu64] + tail),
        ("hwbrj_build_group_rows_device", ci, [vp, ci, ci] + out + [pu64, vp, pdb]),
        ("hwbrj_build_group_reset", ci, [vp, ci]),
        ("hwbrj_build_filter_keys_device", ci, probe + [vp, pu64, vp, pdb]),   # d_out, n_pass, stream, ms
        ("hwbrj_set_materialize", None, [ci]),
        ("hwbrj_set_gpus", ci, [ci]),
        ("hwbrj_generate_device", ci, [vp, u64, u32, u64, u64, dbl, u64, vp]),
        ("hwbrj_generate_device_range", ci, [vp, u64, u64, u64, u32, u64, u64, dbl, u64, vp]),
        ("hwbrj_generate_host", ci, [vp, u64, u32, u64, u64, dbl, u64, ci]),
        ("hwbrj_nonunique_threshold", u64, [u64, dbl, ci]),
        ("hwbrj_create_relation_nonunique", ci, [vp, u64, i64, u32]),
        ("hwbrj_create_relation_nonunique_from_pk", ci, from_pk),
        ("hwbrj_create_relation_fk_from_pk", ci, from_pk),
        ("hwbrj_create_relation_zipf", ci, [vp, u64, u64, dbl, u32, ci]),
        ("hwbrj_create_relation_zipf_device", ci, [vp, u64, u64, dbl, u32, dbl, ci, vp]),
        ("hwbrj_rand_stream", ci, [u32, vp, u64]),
        ("hwbrj_write_relation", ci, [prel, cstr]),
        ("hwbrj_write_result_relation", ci, [vp, cstr]),
        ("hwbrj_export_filter", ci, [vp, u64]),
        ("hwbrj_hash_crc", u32, [u32, i32]),
        ("hwbrj_hash_crapwow", u32, [u32, i32]),
        ("hwbrj_device_count", ci, None),
        ("hwbrj_set_device", ci, [ci]),
        ("hwbrj_last_error", cstr, None),
        ("hwbrj_version", cstr, None),
        ("hwbrj_set_test_hook", ci, [ci, i64]),
        ("hwbrj_tsc_hz", u64, None),
        ("hwbrj_copy_bandwidth", ci, [u64, ci, pdb]),
        ("hwbrj_release", None, None),
    ]


_LIB = None


def lib() -> ctypes.CDLL:
    """Load libhwbrj.so (built by __graft_entry__.build()). Raises if it is missing."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; "
                              "g.build()'` (the MI355X HIP library is required; there is no CPU "
                              "fallback)")
        # torch-ROCm ships its own HIP runtime. If libhwbrj.so (linked against /opt/rocm's) is
        # loaded first, torch's later device init leaves this library's runtime with no devices
        # ("no ROCm-capable device"); loading torch's libraries first makes the two coexist.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        for name, restype, argtypes in _signatures():
            fn = getattr(L, name)
            fn.restype = restype
            if argtypes is not None:
                fn.argtypes = argtypes
        _LIB = L
    return _LIB


def _err(code: int, what: str):
    if code != 0:
        raise RuntimeError(f"{what} failed ({code}): {lib().hwbrj_last_error().decode()}")


@dataclass
class BloomFilterArgs:
    """src/bloom_filter.h:50-55. Defaults are src/main.c:389-393 (variant BASIC, m=256 Mi, k=8,
    B=1024)."""
    variant: int = BASIC
    m: int = 256 << 20
    k: int = 8
    B: int = 1024

    @classmethod
    def from_flag(cls, b: str, m: int, k: int, B: int = 1024) -> Optional["BloomFilterArgs"]:
        """The CLI's -b parsing (src/main.c:692-698): 'no' -> None; unknown -> BASIC, except
        'sectorized' which selects this build's SECTORIZED variant."""
        if b == "no":
            return None
        return cls(_VARIANTS.get(b, BASIC), m, k, B)

    def _c(self) -> _BloomArgs:
        return _BloomArgs(int(self.variant), int(self.m), int(self.k), int(self.B))


@dataclass
class Result:
    """src/types.h:59-63. `pairs` holds the materialized {R.payload, S.payload} result
    (JOIN_RESULT_MATERIALIZE, see set_materialize), else None (the reference's default build)."""
    totalresults: int
    nthreads: int
    pairs: Optional[np.ndarray] = None


class _TupleBuffer(ctypes.Structure):  # src/tuple_buffer.h:27-30
    pass


_TupleBuffer._fields_ = [("tuples", ctypes.POINTER(_Tuple)), ("next", ctypes.POINTER(_TupleBuffer))]


class _ChainedTupleBuffer(ctypes.Structure):  # src/tuple_buffer.h:32-40
    _fields_ = [("buf", ctypes.POINTER(_TupleBuffer)), ("readcursor", ctypes.POINTER(_TupleBuffer)),
                ("writecursor", ctypes.POINTER(_TupleBuffer)), ("writepos", ctypes.c_uint32),
                ("readpos", ctypes.c_uint32), ("readlen", ctypes.c_uint32),
                ("numbufs", ctypes.c_uint32)]


class _ThreadResult(ctypes.Structure):  # src/types.h:51-56
    _fields_ = [("nresults", ctypes.c_int64), ("results", ctypes.c_void_p),
                ("threadid", ctypes.c_uint32)]


_CB_TUPLES = 1024 * 1024  # CHAINEDBUFF_NUMTUPLESPERBUF


def _take_result(r) -> Result:
    """Copy a result_t (and its chained result buffers, if materialized) and free it."""
    libc = ctypes.CDLL(None)
    res = r.contents
    pairs = None
    if res.resultlist:
        tl = ctypes.cast(res.resultlist, ctypes.POINTER(_ThreadResult))
        parts = []
        for t in range(res.nthreads):
            cb = ctypes.cast(tl[t].results, ctypes.POINTER(_ChainedTupleBuffer)).contents
            n, b, first = tl[t].nresults, cb.buf, True
            while b and n > 0:  # cb_begin / cb_read_next order: newest buffer first
                take = min(n, cb.writepos if first else _CB_TUPLES)
                a = np.ctypeslib.as_array(ctypes.cast(b.contents.tuples, ctypes.POINTER(ctypes.c_int32)),
                                          shape=(take * 2,))
                parts.append(a.reshape(-1, 2).copy())
                n -= take
                b, first = b.contents.next, False
            addr = ctypes.cast(cb.buf, ctypes.c_void_p).value
            while addr:  # (plain addresses: a ctypes field view would read freed memory)
                b = ctypes.cast(addr, ctypes.POINTER(_TupleBuffer)).contents
                nxt = ctypes.cast(b.next, ctypes.c_void_p).value
                libc.free(ctypes.cast(b.tuples, ctypes.c_void_p))
                libc.free(ctypes.c_void_p(addr))
                addr = nxt
            libc.free(ctypes.c_void_p(tl[t].results))
        libc.free(ctypes.cast(res.resultlist, ctypes.c_void_p))
        pairs = np.concatenate(parts) if parts else np.empty((0, 2), dtype=np.int32)
    out = Result(res.totalresults, res.nthreads, pairs)
    libc.free(r)
    return out


# include/hwbrj.h hwbrj_set_test_hook
HOOK_JOIN_SPLIT, HOOK_PJ_FAIL_RANK, HOOK_BCAST_NONROOT, HOOK_PJ_PLAN_DIV, HOOK_PJ_ASYNC_FAIL = 1, 2, 3, 4, 5
_HOOK_OFF = {HOOK_JOIN_SPLIT: 0, HOOK_PJ_FAIL_RANK: -1, HOOK_BCAST_NONROOT: 0, HOOK_PJ_PLAN_DIV: 0,
             HOOK_PJ_ASYNC_FAIL: 0}


def version() -> str:
    """hwbrj_version(): name, version and every non-default compile-time knob ("knobs: ...")."""
    return lib().hwbrj_version().decode()


def set_test_hook(hook: int, value: int) -> None:
    """hwbrj_set_test_hook: force a rarely taken path or inject a failure (tests only)."""
    _err(lib().hwbrj_set_test_hook(hook, int(value)), "hwbrj_set_test_hook")


@contextlib.contextmanager
def hooked(hook: int, value: int):
    """set_test_hook for the duration of a with-block (then off again)."""
    set_test_hook(hook, value)
    try:
        yield
    finally:
        set_test_hook(hook, _HOOK_OFF[hook])


def set_gpus(gpus: int) -> None:
    """Shards of S for host BPRO/PRO (hwbrj_set_gpus): shard g on visible device g mod
    device_count, R replicated, counts summed. 0 restores the default (HWBRJ_GPUS, else 1)."""
    _err(lib().hwbrj_set_gpus(int(gpus)), "hwbrj_set_gpus")


def set_materialize(on: bool) -> None:
    """Materialize {R.payload, S.payload} pairs in BPRO/PRO results (JOIN_RESULT_MATERIALIZE)."""
    lib().hwbrj_set_materialize(1 if on else 0)


@dataclass
class Stats:
    filtered: int
    matches: int
    mode: int
    format: int
    partitions: int
    subparts: int
    slice_segments: int
    ms_total: float
    ms_r_scatter: float
    ms_r_index: float
    ms_build: float
    ms_s_scatter: float
    ms_s_index: float
    ms_probe: float
    ms_surv: float
    ms_join: float
    ms_join_probe: float
    join_keys: int = 0       # JOIN_KEYS_32 / _PACKED / _MIXED
    unstaged_items: int = 0  # probe items whose survivors overflowed the LDS stage
    join_key_bits: int = 32  # bits per packed join key (18 at the north star, 24, or 32: codes)


class Relation:
    """relation_t over a contiguous (N, 2) int32 array of {key, payload} (src/types.h:37-49)."""

    def __init__(self, tuples: np.ndarray):
        t = np.ascontiguousarray(tuples, dtype=np.int32)
        if t.ndim != 2 or t.shape[1] != 2:
            raise ValueError("tuples must have shape (N, 2): key, payload")
        self.tuples = t
        self._c = _Relation(t.ctypes.data_as(ctypes.POINTER(_Tuple)), t.shape[0])

    @property
    def num_tuples(self) -> int:
        return self.tuples.shape[0]


def write_relation(rel: "Relation | np.ndarray", filename: str) -> None:
    """src/generator.c:250-263 write_relation (hwbrj_write_relation): a "#KEY, VAL" header, then
    "key payload" lines; the CLI's -R / -S read it back."""
    r = rel if isinstance(rel, Relation) else Relation(rel)
    _err(lib().hwbrj_write_relation(ctypes.byref(r._c), os.fsencode(filename)), "hwbrj_write_relation")


def assert_args(args: BloomFilterArgs) -> bool:
    """src/bloom_filter.c:25-34 without the exit(1): True when the reference would accept."""
    m, B = int(args.m), int(args.B)
    if m & (m - 1):
        return False
    if args.variant != BASIC and (B <= 0 or B & (B - 1) or m % B):
        return False
    return True


def BPRO(relR: Relation, relS: Relation, nthreads: int, args: BloomFilterArgs) -> Result:
    """src/parallel_radix_join_bloom.c:1781-1787 on the MI355X (prints the reference's lines)."""
    a = args._c()
    return _take_result(lib().BPRO(ctypes.byref(relR._c), ctypes.byref(relS._c), int(nthreads),
                                   ctypes.byref(a)))


def PRO(relR: Relation, relS: Relation, nthreads: int) -> Result:
    """src/parallel_radix_join.c:1697-1700 (no filter) on the MI355X."""
    return _take_result(lib().PRO(ctypes.byref(relR._c), ctypes.byref(relS._c), int(nthreads)))


def _run(name: str, relR: Relation, relS: Relation, nthreads: int, args=None) -> Result:
    fn = getattr(lib(), name)
    r = (fn(ctypes.byref(relR._c), ctypes.byref(relS._c), int(nthreads), ctypes.byref(args._c()))
         if args is not None else fn(ctypes.byref(relR._c), ctypes.byref(relS._c), int(nthreads)))
    return _take_result(r)


def BPRH(relR, relS, nthreads, args):
    """src/parallel_radix_join_bloom.c:1789-1795 (same MI355X operator as BPRO)."""
    return _run("BPRH", relR, relS, nthreads, args)


def BPRHO(relR, relS, nthreads, args):
    """src/parallel_radix_join_bloom.c:1797-1804 (same MI355X operator as BPRO)."""
    return _run("BPRHO", relR, relS, nthreads, args)


def BRJ(relR, relS, nthreads, args):
    """src/parallel_radix_join_bloom.c:1806-1930 (same MI355X operator as BPRO)."""
    return _run("BRJ", relR, relS, nthreads, args)


def PRH(relR, relS, nthreads):
    return _run("PRH", relR, relS, nthreads)


def PRHO(relR, relS, nthreads):
    return _run("PRHO", relR, relS, nthreads)


def RJ(relR, relS, nthreads):
    return _run("RJ", relR, relS, nthreads)


def _ptr(t) -> int:
    return int(t.data_ptr())


def _sp(stream):
    """An entry's stream argument: the caller's torch.cuda.Stream as a pointer; None is the library's own."""
    return ctypes.c_void_p(stream.cuda_stream) if stream is not None else None


def _ap(args: Optional[BloomFilterArgs]):
    """An entry's filter argument: a pointer to args as a _BloomArgs; None runs without a filter. The
    byref object owns a reference to the struct it points to, so the struct lives as long as the pointer:
    a wrapper converts once and hands the same pointer to every call it makes, a retry's included."""
    return ctypes.byref(args._c()) if args is not None else None


def _stats(st) -> Stats:
    return Stats(**{f: getattr(st, f) for f, _ in _Stats._fields_})


def _check_rel(R, S):
    """Both relations: contiguous (N, 2) torch.int32 tensors ({key, payload}) on one GPU. The
    library's current HIP device is switched to that GPU (the join runs on its Engine)."""
    import torch
    for name, t in (("R", R), ("S", S)):
        if (not t.is_cuda or t.dtype != torch.int32 or t.dim() != 2 or t.shape[1] != 2
                or not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous (N, 2) torch.int32 tensor on the GPU")
    if R.device != S.device:
        raise ValueError(f"R is on {R.device} but S is on {S.device}")
    _err(lib().hwbrj_set_device(R.device.index or 0), "hwbrj_set_device")


def join_device_async(R, S, args: Optional[BloomFilterArgs] = None, stream=None) -> None:
    """Enqueue the join of device tensors R, S without waiting (hwbrj_join_device_async);
    join_wait() returns the Stats of the last join enqueued on this device (counts; an async join
    records no phase events, so its ms_* fields are 0)."""
    _check_rel(R, S)
    _err(lib().hwbrj_join_device_async(_ptr(R), R.shape[0], _ptr(S), S.shape[0], _ap(args), _sp(stream)),
         "hwbrj_join_device_async")


def join_wait() -> Stats:
    """Wait for the last enqueued join on this device and return its Stats."""
    st = _Stats()
    _err(lib().hwbrj_join_wait(ctypes.byref(st)), "hwbrj_join_wait")
    return _stats(st)


def set_async_timing(on: bool) -> None:
    """hwbrj_set_async_timing: async joins time their S scatter on the side stream that runs it
    (Stats.ms_s_scatter of every async join); off by default."""
    _err(lib().hwbrj_set_async_timing(1 if on else 0), "hwbrj_set_async_timing")


def join_wait_all(capacity: int = 256) -> list:
    """Wait for the last enqueued join and return the Stats of EVERY join enqueued on this device
    since the last join_wait / join_wait_all, oldest first (hwbrj_join_wait_all: each join keeps its
    own counts in a device ring). Raises if more than `capacity` joins are pending."""
    arr = (_Stats * max(1, capacity))()
    n = ctypes.c_int(0)
    _err(lib().hwbrj_join_wait_all(arr, capacity, ctypes.byref(n)), "hwbrj_join_wait_all")
    return [_stats(arr[i]) for i in range(n.value)]


ALGO_PRO, ALGO_PRH, ALGO_PRHO = 0, 1, 2  # include/hwbrj.h HWBRJ_ALGO_* (per-partition join)


def join_device(R, S, args: Optional[BloomFilterArgs] = None, stream=None,
                algorithm: int = ALGO_PRO) -> Stats:
    """Join device-resident torch int32 tensors of shape (N, 2) ({key, payload}) in HBM.
    args=None runs PRO. `stream` is a torch.cuda.Stream (default: the library's own stream).
    algorithm: the per-partition join (ALGO_PRO bucket chaining's role, ALGO_PRH / ALGO_PRHO the
    histogram joins of src/parallel_radix_join_bloom.c:350-555)."""
    _check_rel(R, S)
    st = _Stats()
    _err(lib().hwbrj_join_device_algo(*_rel_head(R, S), _ap(args), int(algorithm), _sp(stream), ctypes.byref(st)),
         "hwbrj_join_device_algo")
    return _stats(st)


def _check_keys(Rk, Sk, stream, Sv=None):
    """Both key columns (and Sv, S's value column of a group join, of Sk's length): contiguous 1-D
    torch.int32 tensors on one GPU, each (when non-empty) starting at a 16-byte boundary. Switches
    the library's HIP device as _check_rel does. Without a stream of the caller's, waits for torch's
    current stream (the columns' producer)."""
    import torch
    for name, t in (("Rk", Rk), ("Sk", Sk)) + ((("Sv", Sv),) if Sv is not None else ()):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch tensor")
        if not t.is_cuda or t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous 1-D torch.int32 tensor on the GPU "
                             "(a strided view such as T[:, 0]: call .contiguous() first)")
        if t.numel() and t.data_ptr() % 16:
            raise ValueError(f"{name} must start at a 16-byte boundary (a slice of a column: cut at "
                             "multiples of 4 keys)")
    if Rk.device != Sk.device:
        raise ValueError(f"Rk is on {Rk.device} but Sk is on {Sk.device}")
    if Sv is not None and Sv.device != Sk.device:
        raise ValueError(f"Sv is on {Sv.device} but Sk is on {Sk.device}")
    if Sv is not None and Sv.shape[0] != Sk.shape[0]:
        raise ValueError(f"Sv has {Sv.shape[0]} values for the {Sk.shape[0]} keys of Sk")
    _err(lib().hwbrj_set_device(Rk.device.index or 0), "hwbrj_set_device")
    if stream is None:
        # a column is typically cut by a torch kernel (.contiguous()) that may still be running on
        # torch's current stream, and the library's own stream does not wait for that stream
        torch.cuda.current_stream(Rk.device).synchronize()


def pack_validity(valid):
    """The validity bitmap of a 1-D torch.bool tensor (True = valid), packed on its device with torch
    ops: a torch.uint8 tensor in Arrow's layout (row i is bit i & 7 of byte i >> 3, LSB first),
    padded with zero bits to a multiple of 4 bytes. What r_valid / s_valid of the join_keys_*
    functions accept as is."""
    import torch
    if not isinstance(valid, torch.Tensor) or valid.dtype != torch.bool or valid.dim() != 1:
        raise ValueError("pack_validity takes a 1-D torch.bool tensor")
    n = valid.shape[0]
    nbytes = (n + 31) // 32 * 4
    bits = torch.zeros(nbytes * 8, dtype=torch.uint8, device=valid.device)
    bits[:n] = valid
    weights = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device=valid.device)
    return (bits.view(nbytes, 8) * weights).sum(dim=1, dtype=torch.uint8)


def _check_valid(name: str, valid, keys):
    """r_valid / s_valid of a key column `keys`: None, a torch.bool tensor of len(keys) entries (packed
    here by pack_validity) or a contiguous 1-D torch.uint8 bitmap of at least ceil(len(keys) / 8)
    bytes on the keys' device, starting at a 4-byte boundary. Returns the bitmap tensor (the caller
    keeps it alive over the call) or None."""
    import torch
    if valid is None:
        return None
    n = keys.shape[0] if isinstance(keys, torch.Tensor) and keys.dim() == 1 else 0
    if not isinstance(valid, torch.Tensor) or valid.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"{name} must be a torch.uint8 bitmap or a torch.bool tensor")
    if valid.dim() != 1 or not valid.is_contiguous():
        raise ValueError(f"{name} must be a contiguous 1-D tensor")
    if isinstance(keys, torch.Tensor) and valid.device != keys.device:
        raise ValueError(f"{name} is on {valid.device} but its key column is on {keys.device}")
    if valid.dtype == torch.bool:
        if valid.shape[0] != n:
            raise ValueError(f"{name} has {valid.shape[0]} entries for {n} keys")
        return pack_validity(valid)
    if valid.shape[0] < (n + 7) // 8:
        raise ValueError(f"{name} has {valid.shape[0]} bytes, {n} keys need {(n + 7) // 8}")
    if n and valid.data_ptr() % 4:
        raise ValueError(f"{name} must start at a 4-byte boundary (a slice of a masked column: cut at "
                         "multiples of 32 rows)")
    return valid


def _vptr(valid):
    return _ptr(valid) if valid is not None and valid.numel() else None


def _rel_head(R, S):
    """The leading arguments of a join of tuple relations."""
    return [_ptr(R), R.shape[0], _ptr(S), S.shape[0]]


def _s_side(Sk, vs, Sv, vv):
    """The S side where bitmaps are taken: S keys, bitmap, a group join's value column and its bitmap, nS."""
    return [_ptr(Sk), _vptr(vs)] + ([] if Sv is None else [_ptr(Sv), _vptr(vv)]) + [Sk.shape[0]]


def _keys_head(entry: str, Rk, vr, Sk, vs, Sv=None, vv=None):
    """(entry, head) of a join on key columns: its leading arguments (R keys, nR, S keys, a group join's
    value column, nS) and, when a bitmap was given, the entry's _nulls_ form with each bitmap after its
    column. vr, vs, vv are what _check_valid returned. The head holds plain addresses: the wrapper keeps
    vr, vs and vv bound until its last call of the entry has returned (a bool mask was packed into a
    tensor that nothing else references)."""
    if vr is None and vs is None and vv is None:
        return entry, [_ptr(Rk), Rk.shape[0], _ptr(Sk)] + ([] if Sv is None else [_ptr(Sv)]) + [Sk.shape[0]]
    return entry.replace("_device", "_nulls_device"), [_ptr(Rk), _vptr(vr), Rk.shape[0]] + _s_side(Sk, vs, Sv, vv)


def _probe_head(h, Sk, vs, Sv=None, vv=None):
    """_keys_head's sibling for the probes of the build with handle h, whose entries always take the
    bitmaps. The keep-alive rule for vs and vv is _keys_head's."""
    return [h] + _s_side(Sk, vs, Sv, vv)


_ROWS, _GROUP, _MINMAX = (2, "int32"), (2, "int64"), (4, "int32")  # row formats: columns, dtype


def _rows(entry: str, head, mid, stream, device, fmt, capacity, known=None, extra=(), stats=True):
    """The protocol of every entry that writes rows: (Stats, rows, ms) of
    entry(*head, *mid, d_out, capacity, &n, *extra, stream, &stats, &ms); stats=False for an entry
    without a stats argument (Stats is then None).
    capacity None is resolved first. known None: by one count-only call (d_out NULL, capacity 0; 0 and 7
    both leave the count in n). A callable known: by known(), a row count that needs no call (nR under
    GROUP_ALL). A wrapper that sizes by a counting join resolves capacity itself and passes the number.
    Then max(capacity, 1) rows of format fmt are allocated on device while capacity itself is passed;
    code 7 (too small, n = the full count) runs the entry once more at that size, and any other failure
    raises under the entry's name. rows is the buffer cut to n."""
    import torch
    fn = getattr(lib(), entry)
    n, st, ms = ctypes.c_uint64(), _Stats(), ctypes.c_double()
    tail = [ctypes.byref(n), *extra, _sp(stream)] + ([ctypes.byref(st)] if stats else []) + [ctypes.byref(ms)]
    if capacity is None and known is not None:
        capacity = known()
    elif capacity is None:
        rc = fn(*head, *mid, None, 0, *tail)  # count only
        if rc not in (0, 7):
            _err(rc, entry)
        capacity = n.value
    for _ in range(2):
        out = torch.empty((max(int(capacity), 1), fmt[0]), dtype=getattr(torch, fmt[1]), device=device)
        rc = fn(*head, *mid, _ptr(out), int(capacity), *tail)
        if rc != 7:
            break
        capacity = n.value
    _err(rc, entry)
    return _stats(st) if stats else None, out[: n.value], ms.value


def join_keys_device(Rk, Sk, args: Optional[BloomFilterArgs] = None, stream=None,
                     algorithm: int = ALGO_PRO, *, r_valid=None, s_valid=None) -> Stats:
    """The counting join of join_device on key columns (hwbrj_join_keys_device): Rk, Sk are
    contiguous 1-D torch.int32 GPU tensors of keys, 16-byte aligned. No payloads are read, so a
    columnar caller needs no (N, 2) interleaving pass. A strided view such as T[:, 0] of a tuple
    tensor is refused: call .contiguous() first. args, stream, algorithm and the returned Stats
    are join_device's. With stream=None the join runs on the library's own stream after torch's
    current stream has finished (the kernel that cut the columns may still be running there); a
    caller who passes a stream orders the columns' producers before the join on it.
    r_valid, s_valid: the columns' validity (hwbrj_join_keys_nulls_device): None (no NULL keys), a
    torch.bool tensor with one entry per key (True = valid), or a torch.uint8 bitmap as pack_validity
    returns it (Arrow's layout, 4-byte aligned). A NULL key matches nothing, and Stats are the join's
    on the valid rows. Partition-slice filters and no filter only."""
    vr, vs = _check_valid("r_valid", r_valid, Rk), _check_valid("s_valid", s_valid, Sk)
    _check_keys(Rk, Sk, stream)
    entry, head = _keys_head("hwbrj_join_keys_device", Rk, vr, Sk, vs)
    st = _Stats()
    _err(getattr(lib(), entry)(*head, _ap(args), int(algorithm), _sp(stream), ctypes.byref(st)), entry)
    return _stats(st)


def join_keys_device_async(Rk, Sk, args: Optional[BloomFilterArgs] = None, stream=None) -> None:
    """Enqueue join_keys_device without waiting (hwbrj_join_keys_device_async); collected by
    join_wait / join_wait_all, in any mix with join_device_async. A strided view such as T[:, 0]
    is refused: call .contiguous() first. The stream rule is join_keys_device's: a stream of the
    caller's must already order whatever wrote the columns."""
    _check_keys(Rk, Sk, stream)
    _err(lib().hwbrj_join_keys_device_async(_ptr(Rk), Rk.shape[0], _ptr(Sk), Sk.shape[0], _ap(args), _sp(stream)),
         "hwbrj_join_keys_device_async")


def join_materialize_device(R, S, args: Optional[BloomFilterArgs] = None, stream=None,
                            capacity: Optional[int] = None):
    """(Stats, pairs, ms): the join of device tensors R, S with its result materialized as a (n, 2)
    int32 GPU tensor of {R.payload, S.payload} pairs, unordered (JOIN_RESULT_MATERIALIZE); ms is
    the device time of the materializing pipeline. capacity: output rows to allocate (None: sized
    by a counting join first; too small: the pipeline runs again at the exact size)."""
    if capacity is None:
        capacity = join_device(R, S, args, stream).matches  # (checks R and S first, as the else branch does)
    else:
        _check_rel(R, S)
    # (this wrapper has always passed the rows it allocates, so 1 where the others pass a capacity of 0)
    return _rows("hwbrj_join_materialize_device", _rel_head(R, S), [_ap(args)], stream, R.device, _ROWS,
                 max(int(capacity), 1))


JOIN_SEMI, JOIN_ANTI = 0, 1  # include/hwbrj.h HWBRJ_JOIN_SEMI / HWBRJ_JOIN_ANTI


def semi_join_device(R, S, args: Optional[BloomFilterArgs] = None, anti: bool = False, stream=None,
                     capacity: Optional[int] = None):
    """(Stats, rows, ms): the semi-join of device tensors S against R (hwbrj_join_semi_device) as a
    (n, 2) int32 GPU tensor of whole S tuples {key, payload}, unordered: the S rows whose key occurs
    in R, each once (anti=True: the S rows whose key does not). Stats.filtered is the counting join's
    "S-tuples after filter", Stats.matches the row count; ms the device time. capacity: output rows
    to allocate (None: one count-only call first; too small: the pipeline runs again at the exact
    size)."""
    _check_rel(R, S)
    return _rows("hwbrj_join_semi_device", _rel_head(R, S), [_ap(args), JOIN_ANTI if anti else JOIN_SEMI], stream,
                 R.device, _ROWS, capacity)


OUTER_S, OUTER_R, OUTER_FULL = 0, 1, 2  # include/hwbrj.h HWBRJ_OUTER_S / _R / _FULL


def outer_join_device(R, S, args: Optional[BloomFilterArgs] = None, kind: int = OUTER_S,
                      null_payload: int = -2**31, stream=None, capacity: Optional[int] = None):
    """(Stats, rows, (n_inner, n_s_only, n_r_only), ms): the outer join of device tensors R and S
    (hwbrj_join_outer_device) as a (n, 2) int32 GPU tensor of rows {R.payload, S.payload}, unordered:
    every matching pair (join_materialize_device's multiset) and, under OUTER_S, a row
    {null_payload, S.payload} for every S row whose key is not in R; under OUTER_R, a row
    {R.payload, null_payload} for every R row whose key is not in S; under OUTER_FULL, both.
    null_payload is the caller's marker and is not checked against the payloads. Stats.filtered is
    the counting join's "S-tuples after filter", Stats.matches the row count; ms the device time.
    capacity: output rows to allocate (None: one count-only call first; too small: the pipeline runs
    again at the exact size)."""
    _check_rel(R, S)
    cls = (ctypes.c_uint64 * 3)()
    stats, rows, ms = _rows("hwbrj_join_outer_device", _rel_head(R, S), [_ap(args), int(kind), int(null_payload)],
                            stream, R.device, _ROWS, capacity, extra=[cls])
    return stats, rows, tuple(int(c) for c in cls), ms


def join_keys_pairs_device(Rk, Sk, args: Optional[BloomFilterArgs] = None, stream=None,
                           capacity: Optional[int] = None, *, r_valid=None, s_valid=None):
    """(Stats, pairs, ms): join_materialize_device on key columns (hwbrj_join_keys_pairs_device).
    Rk, Sk are join_keys_device's columns; pairs is a (n, 2) int32 GPU tensor of {R row, S row},
    unordered: the gather maps into the caller's other columns, exactly the pairs
    join_materialize_device returns on {key, arange} tuples, without that interleaving pass. Both
    columns must have fewer than 2^31 rows. The stream rule is join_keys_device's. capacity: output
    rows to allocate (None: sized by a counting join_keys_device first; too small: the pipeline runs
    again at the exact size). r_valid, s_valid: join_keys_device's (hwbrj_join_keys_pairs_nulls_device):
    the pairs of the valid rows, as positions in the caller's columns."""
    vr, vs = _check_valid("r_valid", r_valid, Rk), _check_valid("s_valid", s_valid, Sk)
    _check_keys(Rk, Sk, stream)
    if capacity is None:
        capacity = join_keys_device(Rk, Sk, args, stream, r_valid=vr, s_valid=vs).matches
    entry, head = _keys_head("hwbrj_join_keys_pairs_device", Rk, vr, Sk, vs)
    return _rows(entry, head, [_ap(args)], stream, Rk.device, _ROWS, capacity)


def semi_join_keys_device(Rk, Sk, args: Optional[BloomFilterArgs] = None, anti: bool = False, stream=None,
                          capacity: Optional[int] = None, *, r_valid=None, s_valid=None):
    """(Stats, rows, ms): semi_join_device on key columns (hwbrj_join_keys_semi_device). rows is a
    (n, 2) int32 GPU tensor of {key, S row}, unordered: rows[:, 1] is the gather map of the S rows
    whose key occurs in Rk (anti=True: does not occur). Stats, ms and capacity as in
    semi_join_device (None: one count-only call first); columns and the stream rule as in
    join_keys_device, fewer than 2^31 rows each. r_valid, s_valid: join_keys_device's
    (hwbrj_join_keys_semi_nulls_device): the valid S rows with a partner among the valid R rows;
    anti=True: every other S row, the NULL ones included (their key field is what the column stores)."""
    vr, vs = _check_valid("r_valid", r_valid, Rk), _check_valid("s_valid", s_valid, Sk)
    _check_keys(Rk, Sk, stream)
    entry, head = _keys_head("hwbrj_join_keys_semi_device", Rk, vr, Sk, vs)
    return _rows(entry, head, [_ap(args), JOIN_ANTI if anti else JOIN_SEMI], stream, Rk.device, _ROWS, capacity)


def outer_join_keys_device(Rk, Sk, args: Optional[BloomFilterArgs] = None, kind: int = OUTER_S, stream=None,
                           capacity: Optional[int] = None, *, r_valid=None, s_valid=None):
    """(Stats, rows, (n_inner, n_s_only, n_r_only), ms): outer_join_device on key columns
    (hwbrj_join_keys_outer_device). rows is a (n, 2) int32 GPU tensor of {R row, S row}, unordered,
    the missing side of an S-only or R-only row being -1 (a row index is never negative, so there is
    no null_payload). Stats, the class counts, ms and capacity as in outer_join_device (None: one
    count-only call first); columns and the stream rule as in join_keys_device, fewer than 2^31
    rows each. r_valid, s_valid: join_keys_device's (hwbrj_join_keys_outer_nulls_device): a NULL S row
    is an S-only row under OUTER_S / OUTER_FULL, a NULL R row an R-only row under OUTER_R / OUTER_FULL,
    counted in their classes."""
    vr, vs = _check_valid("r_valid", r_valid, Rk), _check_valid("s_valid", s_valid, Sk)
    _check_keys(Rk, Sk, stream)
    entry, head = _keys_head("hwbrj_join_keys_outer_device", Rk, vr, Sk, vs)
    cls = (ctypes.c_uint64 * 3)()
    stats, rows, ms = _rows(entry, head, [_ap(args), int(kind)], stream, Rk.device, _ROWS, capacity, extra=[cls])
    return stats, rows, tuple(int(c) for c in cls), ms


GROUP_MATCHED, GROUP_ALL = 0, 1  # include/hwbrj.h HWBRJ_GROUP_MATCHED / _ALL


class _GroupRow(ctypes.Structure):  # include/hwbrj.h hwbrj_group_row_t
    _fields_ = [("r_payload", ctypes.c_int32), ("count", ctypes.c_uint32), ("sum", ctypes.c_int64)]


class GroupRows(NamedTuple):
    """The rows of a group join as GPU tensors of one length: r_payload (int32, a view of raw),
    count (int64, the 32-bit count zero-extended), sum (int64, a view of raw) and raw, the (n, 2)
    int64 buffer of hwbrj_group_row_t rows they come from."""
    r_payload: object
    count: object
    sum: object
    raw: object


def group_join_device(R, S, args: Optional[BloomFilterArgs] = None, kind: int = GROUP_MATCHED, stream=None,
                      capacity: Optional[int] = None):
    """(Stats, GroupRows, n_pairs, ms): the group join of device tensors R and S
    (hwbrj_join_group_device), one row per R row (not per key), unordered: the R row's payload, the
    number of S rows with its key and the sum of their payloads (each sign-extended from int32, exact
    in int64; 0 if there are none). R rows sharing a key each carry the full count and sum.
    GROUP_ALL returns every R row (len(R) rows, count 0 and sum 0 without a partner), GROUP_MATCHED
    only the rows with count > 0. n_pairs is the sum of the counts: join_device's `matches`.
    Stats.filtered is the counting join's "S-tuples after filter", Stats.matches the row count; ms the
    device time. capacity: output rows to allocate (None: one count-only call first, or len(R) rows
    under GROUP_ALL without that call; too small: the pipeline runs again at the exact size)."""
    _check_rel(R, S)
    return _group("hwbrj_join_group_device", False, _rel_head(R, S), [_ap(args)], kind, stream, R.device, capacity,
                  lambda: R.shape[0])


class _GroupMinMaxRow(ctypes.Structure):  # include/hwbrj.h hwbrj_group_minmax_row_t
    _fields_ = [("r_payload", ctypes.c_int32), ("count", ctypes.c_uint32), ("min", ctypes.c_int32),
                ("max", ctypes.c_int32)]


class GroupMinMaxRows(NamedTuple):
    """The rows of a min/max group join as GPU tensors of one length: r_payload, min and max (int32,
    views of raw), count (int64, the 32-bit count zero-extended) and raw, the (n, 4) int32 buffer of
    hwbrj_group_minmax_row_t rows they come from."""
    r_payload: object
    count: object
    min: object
    max: object
    raw: object


def group_minmax_join_device(R, S, args: Optional[BloomFilterArgs] = None, kind: int = GROUP_MATCHED, stream=None,
                             capacity: Optional[int] = None):
    """(Stats, GroupMinMaxRows, n_pairs, ms): the group join's MIN / MAX form
    (hwbrj_join_group_minmax_device), one row per R row (not per key), unordered: the R row's payload,
    the number of S rows with its key and the smallest and the largest of their payloads, compared as
    signed int32. R rows sharing a key each carry the full count, min and max. GROUP_ALL returns every
    R row (len(R) rows; without a partner count 0 and the identities min = 2**31 - 1, max = -2**31, so
    min > max marks an empty group and partial rows over batches of S combine with a plain min and
    max), GROUP_MATCHED only the rows with count > 0. n_pairs, Stats, ms and capacity are
    group_join_device's."""
    _check_rel(R, S)
    return _group("hwbrj_join_group_minmax_device", True, _rel_head(R, S), [_ap(args)], kind, stream, R.device,
                  capacity, lambda: R.shape[0])


def _group_view(raw, minmax: bool):
    """The GroupRows (GroupMinMaxRows) of a raw buffer of hwbrj_group_row_t (hwbrj_group_minmax_row_t)
    rows: views of raw, except the zero-extended count."""
    import torch
    if minmax:
        return GroupMinMaxRows(raw[:, 0], raw[:, 1].to(torch.int64) & 0xFFFFFFFF, raw[:, 2], raw[:, 3], raw)
    return GroupRows(raw.view(torch.int32)[:, 0], (raw[:, 0] >> 32) & 0xFFFFFFFF, raw[:, 1], raw)


def _group(entry: str, minmax: bool, head, mid, kind, stream, device, capacity, nR, stats=True):
    """_rows for a group entry, whose kind follows mid and whose n_pairs follows n: (Stats, GroupRows |
    GroupMinMaxRows, n_pairs, ms). Under GROUP_ALL every R row comes back, so capacity None means nR()
    rows without a count-only call."""
    pairs = ctypes.c_uint64()
    stats, raw, ms = _rows(entry, head, mid + [int(kind)], stream, device, _MINMAX if minmax else _GROUP, capacity,
                           nR if int(kind) == GROUP_ALL else None, [ctypes.byref(pairs)], stats)
    return stats, _group_view(raw, minmax), int(pairs.value), ms


def _group_keys(entry: str, minmax: bool, Rk, Sk, Sv, args, kind, stream, capacity, r_valid=None, s_valid=None,
                sv_valid=None):
    """group_join_keys_device / group_minmax_join_keys_device: (Stats, rows, n_pairs, ms) of
    `entry`, with the capacity behaviour of the tuple wrappers. With a validity argument the entry is
    its _nulls_ form (hwbrj_join_keys_group_nulls_device / _minmax_nulls_device)."""
    vr, vs = _check_valid("r_valid", r_valid, Rk), _check_valid("s_valid", s_valid, Sk)
    vv = _check_valid("sv_valid", sv_valid, Sk)  # (a value per key: the key column's length)
    _check_keys(Rk, Sk, stream, Sv)
    entry, head = _keys_head(entry, Rk, vr, Sk, vs, Sv, vv)
    return _group(entry, minmax, head, [_ap(args)], kind, stream, Rk.device, capacity, lambda: Rk.shape[0])


def group_join_keys_device(Rk, Sk, Sv, args: Optional[BloomFilterArgs] = None, kind: int = GROUP_MATCHED, stream=None,
                           capacity: Optional[int] = None, *, r_valid=None, s_valid=None, sv_valid=None):
    """(Stats, GroupRows, n_pairs, ms): group_join_device on key columns with S's aggregated value in
    a third column (hwbrj_join_keys_group_device). Rk, Sk are join_keys_device's columns and Sv a
    column of Sk's length and kind: Sv[i] is the value of S row i. GroupRows.r_payload is the R row
    index (the gather map for R's other columns), count and sum are over Sv of the S rows with the R
    row's key: exactly group_join_device's rows on stack(Rk, arange) and stack(Sk, Sv), without that
    interleaving pass. len(Rk) < 2^31, len(Sk) < 2^32. kind, capacity, n_pairs, Stats and ms are
    group_join_device's; the stream rule is join_keys_device's.
    r_valid, s_valid, sv_valid: the validity of Rk, Sk and Sv (hwbrj_join_keys_group_nulls_device), each
    in join_keys_device's forms (None, a torch.bool tensor, a torch.uint8 bitmap). An S row takes part
    iff its key and its value are valid: count is COUNT(Sv), sum over the same rows, and n_pairs their
    total. A NULL R row matches nothing and, under GROUP_ALL, still gets its row with count 0.
    r_payload stays the position in the caller's column. Partition-slice filters and no filter only."""
    return _group_keys("hwbrj_join_keys_group_device", False, Rk, Sk, Sv, args, kind, stream, capacity, r_valid,
                       s_valid, sv_valid)


def group_minmax_join_keys_device(Rk, Sk, Sv, args: Optional[BloomFilterArgs] = None, kind: int = GROUP_MATCHED,
                                  stream=None, capacity: Optional[int] = None, *, r_valid=None, s_valid=None,
                                  sv_valid=None):
    """(Stats, GroupMinMaxRows, n_pairs, ms): group_minmax_join_device on key columns
    (hwbrj_join_keys_group_minmax_device): group_join_keys_device's arguments, r_payload the R row
    index, min and max over Sv of the S rows with the R row's key, compared as signed int32.
    r_valid, s_valid, sv_valid: group_join_keys_device's (hwbrj_join_keys_group_minmax_nulls_device); a
    row with count 0 carries min = INT32_MAX and max = INT32_MIN."""
    return _group_keys("hwbrj_join_keys_group_minmax_device", True, Rk, Sk, Sv, args, kind, stream, capacity, r_valid,
                       s_valid, sv_valid)


# ---- prepared builds (include/hwbrj.h "Prepared builds"): build R once, probe it with S batches ----
BUILD_COUNT, BUILD_ROWS = 0, 1          # include/hwbrj.h HWBRJ_BUILD_COUNT / _ROWS
PROBE_MARK_INNER, PROBE_MARK_S = 3, 4   # HWBRJ_PROBE_MARK_INNER / _S (outer_probe_keys_device)
AGG_SUM, AGG_MINMAX = 0, 1              # HWBRJ_AGG_SUM / _MINMAX (the group accumulators' two forms)
_BI_NAMES = ("nR", "purpose", "mode", "F", "NSUB", "join_key_bits", "device", "bytes", "masked")


class Build:
    """A prepared build (hwbrj_build_t): the R side of the joins on key columns, made once by
    build_keys_device and probed by the *_probe_keys_device functions. Owns its device buffers and
    keeps no reference to the column it was made from. A context manager; freed by free(), on exit
    and on garbage collection."""

    def __init__(self, handle: int, device, ms: float = 0.0):
        self._h = handle
        self.device = device
        self.ms = ms  # the build's device time

    def _handle(self) -> int:
        if not self._h:
            raise ValueError("the build has been freed")
        _err(lib().hwbrj_set_device(self.device.index or 0), "hwbrj_set_device")
        return self._h

    def free(self) -> None:
        if self._h:
            h, self._h = self._h, 0
            _err(lib().hwbrj_set_device(self.device.index or 0), "hwbrj_set_device")
            _err(lib().hwbrj_build_free(h), "hwbrj_build_free")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def __del__(self):
        try:
            self.free()
        except Exception:  # (interpreter shutdown: the library may be gone)
            pass

    def info(self) -> dict:
        """hwbrj_build_info: nR, purpose, mode, F, NSUB, join_key_bits, device, bytes (the device
        memory the build holds), masked (R had a validity bitmap)."""
        out = (ctypes.c_uint64 * len(_BI_NAMES))()
        _err(lib().hwbrj_build_info(self._handle(), out, len(_BI_NAMES)), "hwbrj_build_info")
        return {n: int(out[i]) for i, n in enumerate(_BI_NAMES)}

    def export_filter(self, m_bits: int) -> np.ndarray:
        """The build's filter in the reference layout (hwbrj_build_export_filter), as export_filter
        returns the one-shot join's."""
        out = np.zeros(m_bits // 8, dtype=np.uint8)
        _err(lib().hwbrj_build_export_filter(self._handle(), out.ctypes.data, out.nbytes), "hwbrj_build_export_filter")
        return out

    def unmatched_rows(self, capacity: Optional[int] = None, stream=None):
        """(rows, ms): {R row, -1} of every R row no marking probe (PROBE_MARK_INNER / PROBE_MARK_S)
        has matched since the build or the last reset_marks(), NULL R rows included, unordered
        (hwbrj_build_unmatched_device). capacity None: one count-only call first."""
        h = self._handle()
        _, rows, ms = _rows("hwbrj_build_unmatched_device", [h], [], stream, self.device, _ROWS, capacity, stats=False)
        return rows, ms

    def reset_marks(self) -> None:
        _err(lib().hwbrj_build_reset_marks(self._handle()), "hwbrj_build_reset_marks")

    def group_rows(self, agg: int = AGG_SUM, kind: int = GROUP_ALL, capacity: Optional[int] = None, stream=None):
        """(GroupRows | GroupMinMaxRows, n_pairs, ms): the rows of everything the accumulating probes
        (group_accum_probe_keys_device) of form agg have folded in since the build or the last
        reset_group(agg), unordered (hwbrj_build_group_rows_device). GROUP_ALL: every R row, NULL R rows
        and rows without a partner with the identities; GROUP_MATCHED: the rows with count > 0. The
        accumulators stay as they are. capacity None: nR rows under GROUP_ALL, else one count-only call
        first."""
        h = self._handle()
        _, rows, pairs, ms = _group("hwbrj_build_group_rows_device", int(agg) == AGG_MINMAX, [h], [int(agg)], kind,
                                    stream, self.device, capacity, lambda: self.info()["nR"], stats=False)
        return rows, pairs, ms

    def reset_group(self, agg: int = AGG_SUM) -> None:
        """The accumulators of form agg back to the identity rows (hwbrj_build_group_reset)."""
        _err(lib().hwbrj_build_group_reset(self._handle(), int(agg)), "hwbrj_build_group_reset")


def build_keys_device(Rk, args: Optional[BloomFilterArgs] = None, purpose: int = BUILD_ROWS, r_valid=None,
                      stream=None) -> Build:
    """The R side of the joins on key columns, run once (hwbrj_build_keys_device): Rk and r_valid are
    join_keys_device's. purpose BUILD_COUNT serves probe_keys_device, BUILD_ROWS the probes that
    return rows. Partition-slice filters and no filter only. Synchronous; Rk and r_valid are not
    read again afterwards and the Build keeps no reference to them."""
    import torch
    vr = _check_valid("r_valid", r_valid, Rk)
    _check_keys(Rk, torch.empty(0, dtype=torch.int32, device=Rk.device) if isinstance(Rk, torch.Tensor) else Rk, stream)
    h, ms = ctypes.c_void_p(), ctypes.c_double()
    _err(lib().hwbrj_build_keys_device(_ptr(Rk), _vptr(vr), Rk.shape[0], _ap(args), int(purpose), _sp(stream),
                                       ctypes.byref(h), ctypes.byref(ms)), "hwbrj_build_keys_device")
    return Build(h.value, Rk.device, ms.value)


def _check_probe(build, Sk, stream, Sv=None):
    """A probe's arguments: a live Build and S's columns on its device (_check_keys' rules)."""
    import torch
    if not isinstance(build, Build):
        raise ValueError("build must be a Build (build_keys_device)")
    h = build._handle()
    if isinstance(Sk, torch.Tensor) and Sk.device != build.device:
        raise ValueError(f"Sk is on {Sk.device} but the build is on {build.device}")
    _check_keys(Sk, Sk, stream, Sv)
    return h


def probe_keys_device(build: Build, Sk, stream=None, algorithm: int = ALGO_PRO, *, s_valid=None) -> Stats:
    """join_keys_device of the build's R and this S batch (hwbrj_probe_keys_device; a BUILD_COUNT
    build): the same Stats, the R phases 0."""
    vs = _check_valid("s_valid", s_valid, Sk)
    h = _check_probe(build, Sk, stream)
    st = _Stats()
    _err(lib().hwbrj_probe_keys_device(*_probe_head(h, Sk, vs), int(algorithm), _sp(stream), ctypes.byref(st)),
         "hwbrj_probe_keys_device")
    return _stats(st)


def _probe_rows(entry: str, build, Sk, s_valid, stream, capacity, mid=(), extra=()):
    """(Stats, rows, ms) of a probe that returns (n, 2) rows, with the one-shot wrappers' capacity
    behaviour (None: one count-only call first; too small: run again at the exact size)."""
    vs = _check_valid("s_valid", s_valid, Sk)
    h = _check_probe(build, Sk, stream)
    return _rows(entry, _probe_head(h, Sk, vs), mid, stream, build.device, _ROWS, capacity, extra=extra)


def probe_keys_pairs_device(build: Build, Sk, stream=None, capacity: Optional[int] = None, *, s_valid=None):
    """(Stats, pairs, ms): join_keys_pairs_device of the build's R and this S batch
    (hwbrj_probe_keys_pairs_device; a BUILD_ROWS build). S rows are positions in this batch."""
    return _probe_rows("hwbrj_probe_keys_pairs_device", build, Sk, s_valid, stream, capacity)


def semi_probe_keys_device(build: Build, Sk, anti: bool = False, stream=None, capacity: Optional[int] = None, *,
                           s_valid=None):
    """(Stats, rows, ms): semi_join_keys_device of the build's R and this S batch
    (hwbrj_probe_keys_semi_device; a BUILD_ROWS build)."""
    return _probe_rows("hwbrj_probe_keys_semi_device", build, Sk, s_valid, stream, capacity,
                       mid=[JOIN_ANTI if anti else JOIN_SEMI])


def outer_probe_keys_device(build: Build, Sk, kind: int = OUTER_S, stream=None, capacity: Optional[int] = None, *,
                            s_valid=None):
    """(Stats, rows, (n_inner, n_s_only, n_r_only), ms): outer_join_keys_device of the build's R and
    this S batch (hwbrj_probe_keys_outer_device; a BUILD_ROWS build). kind also takes
    PROBE_MARK_INNER (the batch's inner pairs) and PROBE_MARK_S (plus its S-only rows): both mark the
    R rows matched, for Build.unmatched_rows() after the last batch, and write no R-only row."""
    cls = (ctypes.c_uint64 * 3)()
    stats, rows, ms = _probe_rows("hwbrj_probe_keys_outer_device", build, Sk, s_valid, stream, capacity,
                                  mid=[int(kind)], extra=[cls])
    return stats, rows, tuple(int(c) for c in cls), ms


def _group_probe(entry: str, minmax: bool, build, Sk, Sv, kind, stream, capacity, s_valid, sv_valid):
    """_group_keys for a probe: (Stats, rows, n_pairs, ms)."""
    vs, vv = _check_valid("s_valid", s_valid, Sk), _check_valid("sv_valid", sv_valid, Sk)
    h = _check_probe(build, Sk, stream, Sv)
    return _group(entry, minmax, _probe_head(h, Sk, vs, Sv, vv), [], kind, stream, build.device, capacity,
                  lambda: build.info()["nR"])


def group_probe_keys_device(build: Build, Sk, Sv, kind: int = GROUP_MATCHED, stream=None,
                            capacity: Optional[int] = None, *, s_valid=None, sv_valid=None):
    """(Stats, GroupRows, n_pairs, ms): group_join_keys_device of the build's R and this S batch
    (hwbrj_probe_keys_group_device; a BUILD_ROWS build). The rows are this batch's partial
    aggregates: the caller combines the batches' rows per R row."""
    return _group_probe("hwbrj_probe_keys_group_device", False, build, Sk, Sv, kind, stream, capacity, s_valid,
                        sv_valid)


def group_minmax_probe_keys_device(build: Build, Sk, Sv, kind: int = GROUP_MATCHED, stream=None,
                                   capacity: Optional[int] = None, *, s_valid=None, sv_valid=None):
    """(Stats, GroupMinMaxRows, n_pairs, ms): group_minmax_join_keys_device of the build's R and this
    S batch (hwbrj_probe_keys_group_minmax_device; a BUILD_ROWS build)."""
    return _group_probe("hwbrj_probe_keys_group_minmax_device", True, build, Sk, Sv, kind, stream, capacity, s_valid,
                        sv_valid)


def group_accum_probe_keys_device(build: Build, Sk, Sv, agg: int = AGG_SUM, stream=None, *, s_valid=None,
                                  sv_valid=None):
    """(Stats, n_rows, n_pairs, ms): this S batch folded into the build's group accumulators of form
    agg (hwbrj_probe_keys_group_accum_device; a BUILD_ROWS build). No row is returned: n_rows is the
    number of R rows with a partner in this batch and n_pairs the batch's pairs, as the GROUP_MATCHED
    probe of the same batch counts them. Build.group_rows(agg) returns the rows after the last batch.
    The arguments are group_probe_keys_device's."""
    vs, vv = _check_valid("s_valid", s_valid, Sk), _check_valid("sv_valid", sv_valid, Sk)
    h = _check_probe(build, Sk, stream, Sv)
    n, pairs, st, ms = ctypes.c_uint64(), ctypes.c_uint64(), _Stats(), ctypes.c_double()
    _err(lib().hwbrj_probe_keys_group_accum_device(*_probe_head(h, Sk, vs, Sv, vv), int(agg), ctypes.byref(n),
                                                   ctypes.byref(pairs), _sp(stream), ctypes.byref(st),
                                                   ctypes.byref(ms)),
         "hwbrj_probe_keys_group_accum_device")
    return _stats(st), int(n.value), int(pairs.value), ms.value


def filter_keys_device(build: Build, Sk, stream=None, *, s_valid=None, out=None):
    """(bitmap, n_pass, ms): the build's Bloom filter applied to the key column Sk in one streaming
    pass (hwbrj_build_filter_keys_device; a build of either purpose, made with a filter). bitmap is a
    torch.uint8 validity bitmap of (len(Sk) + 31) // 32 * 4 bytes on the build's device (pack_validity's
    padding, the padding bits 0): bit i is set iff row i is valid under s_valid and Sk[i] passes the
    filter. No false negatives, so it serves as s_valid of any probe of the build without changing its
    rows; n_pass, its set bits, is what that probe reports as Stats.filtered. out: a contiguous 1-D
    torch.uint8 tensor on that device of at least that many bytes, starting at a 4-byte boundary,
    written in place of a new tensor and returned cut to the size; it may be the s_valid tensor itself
    (a star join ANDs one column's filter after another into one bitmap)."""
    import torch
    vs = _check_valid("s_valid", s_valid, Sk)
    n = Sk.shape[0] if isinstance(Sk, torch.Tensor) and Sk.dim() == 1 else 0
    nbytes = (n + 31) // 32 * 4
    # Order: what can be said of s_valid and out alone (type, shape, size for Sk's length, alignment) comes
    # first, as _check_valid's checks do, so that it needs neither a live build nor a GPU; a bad Sk (n = 0
    # here) is reported by _check_probe next; out's device is compared last, once the build's is known.
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8:
            raise ValueError("out must be a torch.uint8 tensor")
        if out.dim() != 1 or not out.is_contiguous():
            raise ValueError("out must be a contiguous 1-D tensor")
        if out.shape[0] < nbytes:
            raise ValueError(f"out has {out.shape[0]} bytes, {n} keys need {nbytes}")
        if n and out.data_ptr() % 4:
            raise ValueError("out must start at a 4-byte boundary")
    h = _check_probe(build, Sk, stream)
    if out is None:
        out = torch.empty(nbytes, dtype=torch.uint8, device=build.device)
    elif out.device != build.device:
        raise ValueError(f"out is on {out.device} but the build is on {build.device}")
    n_pass, ms = ctypes.c_uint64(), ctypes.c_double()
    _err(lib().hwbrj_build_filter_keys_device(h, _ptr(Sk), _vptr(vs), n, _ptr(out) if n else None,
                                              ctypes.byref(n_pass), _sp(stream), ctypes.byref(ms)),
         "hwbrj_build_filter_keys_device")
    return out[:nbytes], int(n_pass.value), ms.value


def copy_bandwidth(nbytes: int = 4 << 30, reps: int = 5) -> float:
    """GB/s of a streaming device copy ((read + write) bytes / median time; hwbrj_copy_bandwidth):
    the measured copy rate the roofline reports beside the 8 TB/s spec peak."""
    g = ctypes.c_double()
    _err(lib().hwbrj_copy_bandwidth(int(nbytes), int(reps), ctypes.byref(g)), "hwbrj_copy_bandwidth")
    return g.value


def generate_device(out, nthreads: int, maxid: int, threshold: int, selectivity: float,
                    seed: int, stream=None) -> None:
    """Fill a (N, 2) int32 GPU tensor with the reference generator's multiset
    (src/generator.c:304-415), seeded permuted order, payload = row index."""
    _err(lib().hwbrj_generate_device(_ptr(out), out.shape[0], nthreads, maxid, threshold,
                                     selectivity, seed, _sp(stream)), "hwbrj_generate_device")


def generate_device_range(out, n: int, offset: int, nthreads: int, maxid: int, threshold: int,
                          selectivity: float, seed: int, stream=None) -> None:
    """Rows [offset, offset + out.shape[0]) of the n-row relation generate_device would build."""
    _err(lib().hwbrj_generate_device_range(_ptr(out), n, offset, out.shape[0], nthreads, maxid,
                                           threshold, selectivity, seed, _sp(stream)),
         "hwbrj_generate_device_range")


def generate_host(n: int, nthreads: int, maxid: int, threshold: int, selectivity: float,
                  seed: int, host_threads: int = 0) -> np.ndarray:
    """The same relation as generate_device, on the host: (n, 2) int32."""
    out = np.empty((n, 2), dtype=np.int32)
    _err(lib().hwbrj_generate_host(out.ctypes.data, n, nthreads, maxid, threshold, selectivity,
                                   seed, host_threads), "hwbrj_generate_host")
    return out


def nonunique_threshold(r_size: int, selectivity: float, full_range: bool) -> int:
    """src/main.c:421-427: the key bound of --non-unique / --full-range relations."""
    return int(lib().hwbrj_nonunique_threshold(r_size, selectivity, 1 if full_range else 0))


def create_relation_nonunique(n: int, maxid: int, seed: int) -> np.ndarray:
    """src/generator.c:585-605 after srand(seed): n random keys in [0, maxid), payload = row."""
    out = np.empty((n, 2), dtype=np.int32)
    _err(lib().hwbrj_create_relation_nonunique(out.ctypes.data, n, maxid, seed),
         "hwbrj_create_relation_nonunique")
    return out


def _from_pk(fn, name, n, pk, threshold, selectivity, seed):
    pk = np.ascontiguousarray(pk, dtype=np.int32)
    out = np.empty((n, 2), dtype=np.int32)
    _err(fn(out.ctypes.data, n, pk.ctypes.data, pk.shape[0], threshold, selectivity, seed), name)
    return out


def create_relation_nonunique_from_pk(n: int, pk: np.ndarray, threshold: int, selectivity: float,
                                      seed: int) -> np.ndarray:
    """src/generator.c:608-646 (the --non-unique S relation)."""
    return _from_pk(lib().hwbrj_create_relation_nonunique_from_pk,
                    "hwbrj_create_relation_nonunique_from_pk", n, pk, threshold, selectivity, seed)


def create_relation_fk_from_pk(n: int, pk: np.ndarray, threshold: int, selectivity: float,
                               seed: int) -> np.ndarray:
    """src/generator.c:531-582 (the --full-range S relation)."""
    return _from_pk(lib().hwbrj_create_relation_fk_from_pk, "hwbrj_create_relation_fk_from_pk",
                    n, pk, threshold, selectivity, seed)


def create_relation_zipf(n: int, alphabet_size: int, theta: float, seed: int,
                         host_threads: int = 0) -> np.ndarray:
    """src/generator.c:659-676 + src/genzipf.c:28-158 (the -z S relation), payload = row."""
    out = np.empty((n, 2), dtype=np.int32)
    _err(lib().hwbrj_create_relation_zipf(out.ctypes.data, n, alphabet_size, theta, seed,
                                          host_threads), "hwbrj_create_relation_zipf")
    return out


def create_relation_zipf_device(out, alphabet_size: int, theta: float, seed: int,
                                selectivity: float = 1.0, host_threads: int = 0) -> None:
    """The -z relation into a (n, 2) int32 GPU tensor (binary searches on the GPU). selectivity=1:
    bit-exact create_relation_zipf; < 1: this build's selectivity extension (BASELINE config 5)."""
    _err(lib().hwbrj_create_relation_zipf_device(_ptr(out), out.shape[0], alphabet_size, theta,
                                                 seed, selectivity, host_threads, None),
         "hwbrj_create_relation_zipf_device")


def rand_stream(seed: int, n: int) -> np.ndarray:
    """The first n values of glibc rand() after srand(seed), from the library's restatement."""
    out = np.empty(n, dtype=np.int32)
    _err(lib().hwbrj_rand_stream(seed, out.ctypes.data, n), "hwbrj_rand_stream")
    return out


def reference_relations(r_size: int, s_size: int, selectivity: float = 1.0, skew: float = 0.0,
                        non_unique: bool = False, full_range: bool = False, r_seed: int = 12345,
                        s_seed: int = 54321, nthreads: int = 2, host_threads: int = 0):
    """(R, S) as the reference's main() builds them (src/main.c:410-466), on the host:
    --full-range, --non-unique and -z are bit-exact (keys and order) to the reference for the same
    seeds; the default PK/FK relations have the reference's key multiset in a seeded order."""
    if full_range or non_unique:
        thr = nonunique_threshold(r_size, selectivity, full_range)
        R = create_relation_nonunique(r_size, thr, r_seed)
        mk = create_relation_fk_from_pk if full_range else create_relation_nonunique_from_pk
        return R, mk(s_size, R, thr, selectivity, s_seed)
    R = generate_host(r_size, nthreads, r_size, r_size, 1.0, r_seed, host_threads)
    if skew > 0:
        return R, create_relation_zipf(s_size, r_size, skew, s_seed, host_threads)
    return R, generate_host(s_size, nthreads, 2**31 - 1, r_size, selectivity, s_seed, host_threads)


def export_filter(m_bits: int) -> np.ndarray:
    """The last join's filter in the reference's byte layout (m/8 uint8)."""
    out = np.empty(m_bits // 8, dtype=np.uint8)
    _err(lib().hwbrj_export_filter(out.ctypes.data, out.nbytes), "hwbrj_export_filter")
    return out


# include/hwbrj.h HWBRJ_TI_* (the words of hwbrj_tables_info, in order) and HWBRJ_TAB_*
_TI_NAMES = ("mode", "format", "F", "NSUB", "sub_shift", "hash_shift", "nseg", "bitmap", "jkind",
             "key_bits", "G", "CH", "BSW", "slot", "stage_cap", "sweeps", "items", "jobs", "mat",
             "split", "sc_round", "sc_flushes", "j_fused", "j_fw", "j_fs", "j_waves", "j_desc",
             "j_piece", "j_task_surv", "j_extra", "j_tail_u", "j_tail_s", "j_rw", "j_sw", "m_piece",
             "m_desc", "m_rcap")
(TAB_R_ELEM_START, TAB_S_ELEM_START, TAB_R_SWEEP_START, TAB_R_RUN_CNT, TAB_R_RUN_OFF, TAB_R_KEYS,
 TAB_S_LIST_START, TAB_S_ITEM_START, TAB_SURV_CNT, TAB_SURV_OFF, TAB_NPARTS) = range(11)
TAB_SURV_ITEM = 64
_TAB_U64 = (TAB_R_ELEM_START, TAB_S_ELEM_START)
# return codes of hwbrj_tables_info / hwbrj_tables_read
TABLES_NONE, TABLES_PENDING, TABLES_OTHER_PIPELINE, TABLES_TOO_SMALL = 6, 12, 13, 7


class TablesError(RuntimeError):
    """hwbrj_tables_info / hwbrj_tables_read refused: .code is the library's return code."""

    def __init__(self, code: int, what: str):
        super().__init__(f"{what} failed ({code}): {lib().hwbrj_last_error().decode()}")
        self.code = code


def tables_info() -> dict:
    """hwbrj_tables_info (test-only): the geometry, launch shape and kernel constants of the last
    collected synchronous join on this device, by the names of _TI_NAMES. Raises TablesError."""
    L = lib()
    L.hwbrj_tables_info.restype = ctypes.c_int
    L.hwbrj_tables_info.argtypes = [ctypes.c_void_p, ctypes.c_int]
    out = np.zeros(len(_TI_NAMES), dtype=np.uint64)
    rc = L.hwbrj_tables_info(out.ctypes.data, out.shape[0])
    if rc:
        raise TablesError(rc, "hwbrj_tables_info")
    return {n: int(v) for n, v in zip(_TI_NAMES, out)}


def tables_read(which: int, item: Optional[int] = None) -> np.ndarray:
    """hwbrj_tables_read (test-only): table `which` (TAB_*) of the last collected synchronous join as
    a flat array (uint64 for the element starts, else uint32); TAB_SURV_ITEM with `item`: that probe
    item's survivor region, raw. Raises TablesError."""
    L = lib()
    L.hwbrj_tables_read.restype = ctypes.c_int
    L.hwbrj_tables_read.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64,
                                    ctypes.POINTER(ctypes.c_uint64)]
    w = which + (int(item) if which == TAB_SURV_ITEM else 0)
    need = ctypes.c_uint64()
    rc = L.hwbrj_tables_read(w, None, 0, ctypes.byref(need))
    if rc not in (0, TABLES_TOO_SMALL):
        raise TablesError(rc, "hwbrj_tables_read")
    out = np.zeros(need.value // 8 if which in _TAB_U64 else need.value // 4,
                   dtype=np.uint64 if which in _TAB_U64 else np.uint32)
    if need.value:
        rc = L.hwbrj_tables_read(w, out.ctypes.data, out.nbytes, ctypes.byref(need))
        if rc:
            raise TablesError(rc, "hwbrj_tables_read")
    return out


def shard_range(n: int, rank: int, world: int) -> tuple[int, int]:
    """Rows [lo, hi) of an n-row relation owned by `rank` of `world` (range sharding of S, the
    multi-GPU analogue of the reference's per-thread chunking,
    src/parallel_radix_join_bloom.c:1646-1670: equal chunks, the remainder spread evenly)."""
    return rank * n // world, (rank + 1) * n // world


def hash_crc(seed: int, key: int) -> int:
    return lib().hwbrj_hash_crc(seed, key)


def hash_crapwow(seed: int, key: int) -> int:
    return lib().hwbrj_hash_crapwow(seed, key)
