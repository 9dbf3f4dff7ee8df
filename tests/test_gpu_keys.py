"""The counting join on key columns (hw.join_keys_device / join_keys_device_async) against the
oracle on the tuples the columns were cut from.

Every test builds (N, 2) relations as the other GPU tests do, uploads them, and uploads
T[:, 0].contiguous() as the key column. Every count is compared with orc.bpro on the tuples, never
with the code under test alone; the tuple join (hw.join_device) is run beside it where the issue is
that the two layouts leave the same tables: launch shape, pass-1 element starts, every job's R keys.
Fuzz cases, scatter cells and the table decoders are imported from the tests that own them."""
import numpy as np
import pytest

import shapes
import test_gpu_fuzz as fz
import test_gpu_shapes as gs
from test_gpu_shapes import BLK512, geometry, scatter_codes

pytestmark = pytest.mark.gpu

NSEEDS = 64
INT_MIN, INT_MAX = -2**31, 2**31 - 1
_TUPLE = {}  # seed -> (Stats of hw.join_device, nR, basic k) for the coverage test


def _dev(cuda, a):
    return cuda.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _col(dT):
    """The key column of an uploaded (N, 2) relation."""
    return dT[:, 0].contiguous()


def _tuple_stats(hw, cuda, seed):
    if seed not in _TUPLE:
        R, S, args, algorithm = fz._inputs(hw, seed)
        st = hw.join_device(_dev(cuda, R), _dev(cuda, S), args, algorithm=algorithm)
        _TUPLE[seed] = (st, R.shape[0], args.k if args is not None and args.variant == hw.BASIC else 0)
    return _TUPLE[seed]


# ----------------------------------------------------------------------------------- 1. fuzz
@pytest.mark.parametrize("seed", range(NSEEDS))
def test_fuzz_key_columns_vs_oracle(hw, cuda, orc, seed):
    R, S, args, algorithm = fz._inputs(hw, seed)
    dR, dS = _dev(cuda, R), _dev(cuda, S)
    st = hw.join_keys_device(_col(dR), _col(dS), args, algorithm=algorithm)
    filt, res = fz._oracle(orc, seed, R, S, args)
    assert (st.filtered, st.matches) == (filt, res), (seed, fz.case(seed)[:5], st)
    tu = _tuple_stats(hw, cuda, seed)[0]
    assert (st.mode, st.format, st.partitions, st.subparts) == (tu.mode, tu.format, tu.partitions, tu.subparts)


def test_fuzz_seeds_cover_every_pipeline(hw, cuda):
    """Seed-independent: what the 64 seeds reach, from the tuple join's own stats."""
    sts = [_tuple_stats(hw, cuda, s) for s in range(NSEEDS)]
    assert {st.mode for st, _, _ in sts} >= {0, 1, 2, 3}
    assert {st.format for st, _, _ in sts} == {0, 1}
    assert any(k >= 2 and nR > 0 for _, nR, k in sts), "no basic k >= 2 case"
    assert any(nR == 0 for _, nR, _ in sts), "no empty R"


# --------------------------------------------------------------------------- 2. scatter cells
def _r_keys_by_job(hw, info, T):
    """Sorted (job << 32 | job key) of every R run of the last join (as test_gpu_shapes.run_case)."""
    F, NSUB = info["F"], info["NSUB"]
    sweep_q = np.repeat(np.arange(F), np.diff(T["r_sweep_start"].astype(np.int64)))
    unit, sub, v = shapes.decode_slots(hw.tables_read(hw.TAB_R_KEYS), info["slot"], T["r_cnt"], T["r_off"],
                                       info["key_bits"], info["hash_shift"])
    return np.sort(((sweep_q[unit] * NSUB + sub).astype(np.uint64) << np.uint64(32)) | v.astype(np.uint64))


@pytest.mark.parametrize("how", ["R-F1024", "S-F1024", "R-F512", "S-F512"])
@pytest.mark.parametrize("cell", gs.S_CELLS)
def test_scatter_cells_key_columns(hw, cuda, orc, crc, cell, how):
    """S1-S5 of test_gpu_shapes (see test_scatter_cells for what each shape reaches) crafted on the R
    side and on the S side, at F = 1024 (PRO) and F = 512: counts against the oracle; element starts
    and every job's R keys equal to those the tuple join leaves."""
    side, kind = how.split("-")
    cfg = BLK512 if kind == "F512" else None
    info0 = geometry(hw, cuda, cfg, 8)
    for codes in scatter_codes(cell, info0):
        n = codes.size
        keys = crc.key_of(codes)
        big = np.stack([keys, np.arange(n, dtype=np.int32)], 1)
        m = min(n, 3000)
        other = np.concatenate([keys[:: max(1, n // max(m, 1))][:m], crc.key_of(shapes.filler_codes(info0, 500, (), 99))])
        small = np.stack([other, np.arange(other.size, dtype=np.int32)], 1)
        R, S = (big, small) if side == "R" else (small, big)
        dR, dS = _dev(cuda, R), _dev(cuda, S)
        hw.join_device(dR, dS, gs.mk(hw, cfg))
        info_t = hw.tables_info()
        T_t = gs.read_tables(hw, info_t)
        keys_t = _r_keys_by_job(hw, info_t, T_t)
        st = hw.join_keys_device(_col(dR), _col(dS), gs.mk(hw, cfg))
        info_k = hw.tables_info()
        T_k = gs.read_tables(hw, info_k)
        assert (st.filtered, st.matches) == gs.ref_counts(orc, hw, R, S, cfg), (cell, how, n)
        assert {k: info_k[k] for k in gs.GEOM} == {k: info_t[k] for k in gs.GEOM}
        assert np.array_equal(T_k["r_elem_start"], T_t["r_elem_start"])
        assert np.array_equal(T_k["s_elem_start"], T_t["s_elem_start"])
        assert np.array_equal(_r_keys_by_job(hw, info_k, T_k), keys_t)


@pytest.fixture(scope="module")
def crc(orc):
    return shapes.Crc(orc.crc)


# ----------------------------------------------------------------------- 3. round edges by byte
EDGE_N = ["1", "2", "3", "4", "5", "4G-1", "4G", "4G+1"]


@pytest.mark.parametrize("side", ["R", "S"])
@pytest.mark.parametrize("nspec", EDGE_N)
def test_column_ends_inside_a_16_byte_load(hw, cuda, orc, nspec, side):
    """A column of exactly n keys (torch.empty(n), no padding) whose last 16-byte group is partial
    or just full, with INT32_MIN, INT32_MAX, 0 and -1 among the keys; PRO and a blocked filter."""
    G = geometry(hw, cuda, None, 8)["G"]
    n = {"4G-1": 4 * G - 1, "4G": 4 * G, "4G+1": 4 * G + 1}.get(nspec) or int(nspec)
    special = np.array([INT_MIN, INT_MAX, 0, -1], dtype=np.int32)
    rng = np.random.default_rng(n)
    k = rng.integers(INT_MIN, INT_MAX, size=n, endpoint=True).astype(np.int32)
    k[-min(n, 4):] = np.roll(special, n)[-min(n, 4):]  # the column ends in the extreme keys
    big = fz._rel(k, rng)
    small = fz._rel(np.concatenate([special, k[:50], np.array([7, 8, 9], dtype=np.int32)]), rng)
    R, S = (big, small) if side == "R" else (small, big)

    def exact(T):  # the column in an allocation of exactly its size
        c = cuda.empty(T.shape[0], dtype=cuda.int32, device="cuda:0")
        c.copy_(cuda.from_numpy(np.ascontiguousarray(T[:, 0])))
        return c
    cR, cS = exact(R), exact(S)
    for cfg in (None, BLK512):
        st = hw.join_keys_device(cR, cS, gs.mk(hw, cfg))
        assert (st.filtered, st.matches) == gs.ref_counts(orc, hw, R, S, cfg), (nspec, side, cfg)


# ------------------------------------------------------------------------------ 4. async mix
MIX = [3, 4, 34, 37, 10, 7, 26, 12]  # odd positions run on key columns
SMALL = [12, 42]


def test_async_mix_of_tuples_and_key_columns(hw, cuda, orc):
    """8 joins back to back, tuples and key columns alternating: a global-bitmap case, a basic k >= 2
    case and an empty R in each layout's half; then 70 small key-column joins across the 64-slot
    ring. Every entry of join_wait_all against its own oracle counts."""
    cfgs = [fz.case(s) for s in MIX]
    for half in (cfgs[0::2], cfgs[1::2]):
        assert any(v in ("blocked", "sectorized") and B < 8 for v, _, _, B, _, _, _ in half)
        assert any(v == "basic" and k >= 2 and Rk.size for v, _, k, _, _, Rk, _ in half)
        assert any(Rk.size == 0 for *_, Rk, _ in half)
    ins = [fz._inputs(hw, s) for s in MIX]
    want = [fz._oracle(orc, s, R, S, a) for s, (R, S, a, _) in zip(MIX, ins)]
    dev = [(_dev(cuda, R), _dev(cuda, S)) for R, S, _, _ in ins]
    cols = [(_col(dR), _col(dS)) if i % 2 else None for i, (dR, dS) in enumerate(dev)]
    cuda.cuda.synchronize()  # (the columns were cut on torch's stream; the joins run on `stream`)
    stream = cuda.cuda.Stream()
    for i, ((dR, dS), (_, _, a, _)) in enumerate(zip(dev, ins)):
        if i % 2:
            hw.join_keys_device_async(cols[i][0], cols[i][1], a, stream=stream)
        else:
            hw.join_device_async(dR, dS, a, stream=stream)
    sts = hw.join_wait_all()
    assert len(sts) == len(MIX)
    got = [(st.filtered, st.matches) for st in sts]
    assert got == want, [(s, g, w) for s, g, w in zip(MIX, got, want) if g != w]

    ins = [fz._inputs(hw, s) for s in SMALL]
    want = [fz._oracle(orc, s, R, S, a) for s, (R, S, a, _) in zip(SMALL, ins)]
    cols = [(_col(_dev(cuda, R)), _col(_dev(cuda, S))) for R, S, _, _ in ins]
    cuda.cuda.synchronize()
    for i in range(70):
        hw.join_keys_device_async(cols[i % 2][0], cols[i % 2][1], ins[i % 2][2], stream=stream)
    sts = hw.join_wait_all()
    assert len(sts) == 70
    assert [(st.filtered, st.matches) for st in sts] == [want[i % 2] for i in range(70)]


# ------------------------------------------------------------------------ 5. Python refusals
def test_python_refusals(hw, cuda, orc):
    R, S, args, _ = fz._inputs(hw, 12)
    dR, dS = _dev(cuda, R), _dev(cuda, S)
    cR, cS = _col(dR), _col(dS)
    bad = {"(N, 2) tensor": dR, "int64 column": cR.to(cuda.int64), "CPU tensor": cR.cpu(),
           "strided view": dR[:, 0], "misaligned slice": cR[1:]}
    assert cR[1:].data_ptr() % 16 and not dR[:, 0].is_contiguous()
    for what, t in bad.items():
        for fn in (hw.join_keys_device, hw.join_keys_device_async):
            with pytest.raises(ValueError):
                fn(t, cS, args)
            with pytest.raises(ValueError):
                fn(cR, t, args)
    st = hw.join_device(dR, dS, args)
    assert (st.filtered, st.matches) == fz._oracle(orc, 12, R, S, args)
