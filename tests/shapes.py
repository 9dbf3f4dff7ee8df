"""Plain-numpy references and key crafting for the path tests (tests/test_gpu_shapes.py).

Nothing here touches the GPU or the library's own tables: the CRC matrix is rebuilt from 33 oracle
calls, the key stream format is restated from DESIGN.md s3, and `classify` restates which branch of
`join_job` / `k_join_mat` (hwbrj_kernels.hip) a (job, part) must take, from the tables the join left
behind (hwbrj_tables_read) and the kernel constants (hwbrj_tables_info). No constant of the kernels
is written down here: every threshold comes from the `info` dict.

The last section builds the crafted relations that the outer-join and the materializing-join tests
share (mat_geometry there is the one function that runs a join: it asks the library for the
geometry the keys are crafted for).
"""
from __future__ import annotations

import numpy as np

U32 = np.uint32
SEED = 42  # the reference's hash seed (parallel_radix_join_bloom.c:1583)


# ------------------------------------------------------------------------------------ Crc
class Crc:
    """code(key) = crc32c(42, key) on 4-byte keys is affine over GF(2): code = M key ^ c.

    `crc(seed, key)` is the oracle's scalar hash (orc.crc, key as int32). 33 calls give c (key 0)
    and the 32 columns of M (keys 1 << i); Gaussian elimination inverts M."""

    def __init__(self, crc):
        as_i32 = lambda x: int(np.array(x, dtype=np.uint32).astype(np.int32))
        self.c = int(crc(SEED, 0)) & 0xFFFFFFFF
        self.cols = [(int(crc(SEED, as_i32(1 << i))) & 0xFFFFFFFF) ^ self.c for i in range(32)]
        # pairs (M e, e), reduced until M e = 1 << b: then M^-1 (1 << b) = e
        v, e = list(self.cols), [1 << i for i in range(32)]
        for b in range(32):
            p = next((i for i in range(b, 32) if (v[i] >> b) & 1), None)
            if p is None:
                raise ValueError("the CRC matrix is singular")
            v[b], v[p], e[b], e[p] = v[p], v[b], e[p], e[b]
            for i in range(32):
                if i != b and (v[i] >> b) & 1:
                    v[i] ^= v[b]
                    e[i] ^= e[b]
        assert v == [1 << i for i in range(32)]
        self.icols = e
        self._fwd = self._byte_tables(self.cols)
        self._inv = self._byte_tables(self.icols)

    @staticmethod
    def _byte_tables(cols):
        t = np.zeros((4, 256), dtype=np.uint32)
        for j in range(4):
            for b in range(256):
                r = 0
                for i in range(8):
                    if (b >> i) & 1:
                        r ^= cols[8 * j + i]
                t[j, b] = r
        return t

    @staticmethod
    def _apply(t, x):
        x = np.asarray(x).astype(np.uint32)
        return t[0][x & U32(255)] ^ t[1][(x >> U32(8)) & U32(255)] ^ t[2][(x >> U32(16)) & U32(255)] ^ t[3][x >> U32(24)]

    def code(self, keys) -> np.ndarray:
        """uint32 codes of int32 (or uint32) keys."""
        k = np.asarray(keys)
        if k.dtype != np.uint32:
            k = k.astype(np.int64).astype(np.uint32)  # (two's complement of negative keys)
        return self._apply(self._fwd, k) ^ U32(self.c)

    def key_of(self, codes) -> np.ndarray:
        """The int32 keys whose codes are `codes` (any bits may be chosen)."""
        c = np.asarray(codes).astype(np.uint32) ^ U32(self.c)
        return self._apply(self._inv, c).view(np.int32)


# ---------------------------------------------------------------------------------- job_of
def job_of(codes, info):
    """(q, sub, v) of codes for the modes whose partition digit is a code digit (sub_shift > 0)."""
    if info["sub_shift"] == 0:
        raise ValueError("the partition is no code digit in this mode (basic filters)")
    c = np.asarray(codes).astype(np.uint32)
    q = c & U32(info["F"] - 1)
    sub = (c >> U32(info["sub_shift"])) & U32(info["NSUB"] - 1)
    v = c >> U32(info["hash_shift"])
    return q, sub, v


def crapwow(keys, seed=SEED):
    """CrapWow(seed, key) of src/hash.c:26-47 on 4-byte keys, vectorised (uint32)."""
    N = np.uint64(0x5052ACDB)
    M = np.uint64(0xFFFFFFFF)
    k = np.asarray(keys)
    key = (k if k.dtype == np.uint32 else k.astype(np.int64).astype(np.uint32)).astype(np.uint64)
    h = np.full(key.shape, 4, dtype=np.uint64)
    kk = (h + np.uint64(seed) + N) & M
    p = key * N
    h, kk = h ^ (p & M), kk ^ (p >> np.uint64(32))
    p = (h ^ ((kk + N) & M)) * N
    h, kk = h ^ (p & M), kk ^ (p >> np.uint64(32))
    return (kk ^ h).astype(np.uint32)


def job_of_basic(keys, info, m):
    """(q, sub, v) of keys under a basic filter of m bits (sub_shift = 0): the partition is the slice
    of the key's first filter bit, q = (CrapWow(42, key) mod m) mod F, and the join compares the
    words bmix(key) = h ^ (h >> 16), h = key * 0x9E3779B1 (Modes)."""
    assert info["sub_shift"] == 0
    k = np.asarray(keys)
    key = k if k.dtype == np.uint32 else k.astype(np.int64).astype(np.uint32)
    q = (crapwow(key) & U32((m - 1) & 0xFFFFFFFF)) & U32(info["F"] - 1)
    h = (key.astype(np.uint64) * np.uint64(0x9E3779B1)).astype(np.uint32)
    w = h ^ (h >> U32(16))
    return q, w & U32(info["NSUB"] - 1), w >> U32(info["hash_shift"])


def job_codes(info, q, sub, v):
    """Codes of job (q, sub) with job keys v (the inverse of job_of)."""
    v = np.asarray(v, dtype=np.uint64)
    assert info["sub_shift"] > 0 and 0 <= q < info["F"] and 0 <= sub < info["NSUB"]
    assert v.size == 0 or int(v.max()) < (1 << (32 - info["hash_shift"]))
    return (U32(q) | U32(sub << info["sub_shift"]) | (v << np.uint64(info["hash_shift"])).astype(np.uint32))


def wg_range(n, G, w):
    """Input elements [lo, hi) of scatter workgroup w of G over n tuples (scatter_body: units of 4
    tuples split evenly, e0 = 4 (w units / G))."""
    units = (n + 3) // 4
    return min(n, 4 * (w * units // G)), min(n, 4 * ((w + 1) * units // G))


def filler_codes(info, n, avoid_q, salt=0):
    """n distinct codes whose partition is not in avoid_q (a fixed odd stride through the
    (high bits, allowed partition) space: no two alike, no random collisions)."""
    F = info["F"]
    allowed = np.array([q for q in range(F) if q not in set(avoid_q)], dtype=np.uint64)
    assert allowed.size, "every partition is under test"
    hi_bits = 32 - (F.bit_length() - 1)
    space = allowed.size << hi_bits
    assert n <= space
    stride = 2654435761  # prime: coprime to space unless it divides len(allowed)
    assert np.gcd(stride, space) == 1
    idx = (np.arange(n, dtype=np.uint64) * np.uint64(stride % space) + np.uint64(salt % space)) % np.uint64(space)
    hi, qi = idx // np.uint64(allowed.size), idx % np.uint64(allowed.size)
    return ((hi << np.uint64(F.bit_length() - 1)) | allowed[qi]).astype(np.uint32)


def craft(crc, info, spec):
    """An (n, 2) int32 relation {key, payload = row} from spec:

      n        tuples
      G        scatter workgroups (info["G"])
      place    [(w, codes)]: these codes, contiguous, from the start of workgroup w's input range
               (several placements of one w follow each other), so they land in consecutive chunks
               of w's region and, per partition, next to each other in the chunk list
      avoid_q  partitions the filler stays out of (the partitions under test)
      salt     shifts the filler codes (R and S fillers that must not match: different salts do
               not guarantee it; callers that need disjoint fillers pass disjoint avoid sets)
    """
    n, G = spec["n"], spec.get("G", info["G"])
    codes = filler_codes(info, n, spec.get("avoid_q", ()), spec.get("salt", 0))
    used = {}
    for w, cs in spec.get("place", ()):
        cs = np.asarray(cs, dtype=np.uint32)
        lo, hi = wg_range(n, G, w)
        at = used.get(w, lo)
        assert at + cs.size <= hi, f"workgroup {w} holds {hi - lo} tuples, placement needs {at - lo + cs.size}"
        codes[at:at + cs.size] = cs
        used[w] = at + cs.size
    rel = np.empty((n, 2), dtype=np.int32)
    rel[:, 0] = crc.key_of(codes)
    rel[:, 1] = np.arange(n, dtype=np.int64).astype(np.int32)
    return rel


# ------------------------------------------------------------------------------ decode_runs
def decode_slots(raw, slot, cnt, off, kbits, hash_shift, surv=False):
    """decode_runs over many slots at once: raw holds len(cnt) / NSUB ... slots of `slot` words back
    to back, cnt / off are [slots, NSUB]. Returns flat (slot index, sub, v) of every key, in run
    order. Raises if a run leaves its slot."""
    raw = np.ascontiguousarray(raw, dtype=np.uint32)
    cnt2 = np.asarray(cnt, dtype=np.int64)
    nsub = cnt2.shape[1]
    c = cnt2.ravel()
    o = np.asarray(off).ravel().astype(np.int64)
    packed_run = ((o >> 31) & 1).astype(bool) if surv else np.full(c.size, kbits != 32)
    assert kbits in (18, 24) or not packed_run[c > 0].any(), f"packed run with kbits = {kbits}"
    o &= 0x7FFFFFFF
    run = np.repeat(np.arange(c.size), c)
    idx = o[run] + (np.arange(run.size) - np.repeat(np.cumsum(c) - c, c))  # key offset in the slot
    unit, pk = run // nsub, packed_run[run]
    by = np.concatenate([raw.view(np.uint8), np.zeros(8, dtype=np.uint8)]).astype(np.uint64)
    base = unit * (slot * 4)  # the slot's byte 0
    # every run inside its slot (checked before anything is read)
    inside_pk = (idx + 1) * kbits <= slot * 32
    assert np.where(pk, inside_pk, idx < slot).all(), "run leaves its slot"
    if kbits == 18:  # key o at bit 18 off + 18 o of the slot
        bit = idx * 18
        b, sh = np.where(pk, base + (bit >> 3), 0), (bit & 7).astype(np.uint64)
        dw = by[b] | (by[b + 1] << np.uint64(8)) | (by[b + 2] << np.uint64(16)) | (by[b + 3] << np.uint64(24))
        vp = (dw >> sh) & np.uint64((1 << 18) - 1)
    elif kbits == 24:  # key o at byte 3 (off + o)
        b = np.where(pk, base + idx * 3, 0)
        vp = by[b] | (by[b + 1] << np.uint64(8)) | (by[b + 2] << np.uint64(16))
    else:
        vp = np.zeros(run.size, dtype=np.uint64)
    vc = raw[np.where(pk, 0, unit * slot + idx)].astype(np.uint64) >> np.uint64(hash_shift)  # 32-bit codes
    return unit, run % nsub, np.where(pk, vp, vc).astype(np.uint32)


def decode_runs(raw, cnt, off, kbits, hash_shift, surv=False):
    """The job keys v of each run of one sweep slot / item region ("Join keys").

    raw: the slot's / region's uint32 words. Run i holds cnt[i] keys from key offset off[i] (its low
    31 bits). Packed runs (every R run when kbits is 18 or 24; a survivor run when bit 31 of its off
    entry is set) hold v as a bit stream from the slot's byte 0: 18-bit keys, key o at bit
    18 off + 18 o; or 24-bit keys, key o at byte 3 (off + o). Other runs hold 32-bit codes at word
    off + o, v = code >> hash_shift. Raises if a run leaves the slot."""
    raw = np.ascontiguousarray(raw, dtype=np.uint32)
    cnt = np.asarray(cnt, dtype=np.int64).reshape(1, -1)
    _, _, v = decode_slots(raw, raw.size, cnt, np.asarray(off).reshape(1, -1), kbits, hash_shift, surv)
    return np.split(v, np.cumsum(cnt.ravel())[:-1])


def pack_runs(runs, kbits, hash_shift, nwords, low=0):
    """The ten-line packer decode_runs is tested against: runs (lists of v) back to back from key
    offset 0 into nwords words; 32-bit codes get `low` as their low hash_shift bits."""
    vs = np.concatenate([np.asarray(r, dtype=np.uint64) for r in runs]) if runs else np.zeros(0, np.uint64)
    if kbits == 32:
        w = np.zeros(nwords, dtype=np.uint32)
        w[:vs.size] = ((vs << np.uint64(hash_shift)) | np.uint64(low)).astype(np.uint32)
        return w
    bits = np.zeros(nwords * 32, dtype=np.uint8)
    for i, v in enumerate(vs.tolist()):
        for b in range(kbits):
            bits[i * kbits + b] = (v >> b) & 1
    return np.packbits(bits, bitorder="little").view(np.uint32)


# --------------------------------------------------------------------------------- classify
def _tail(n, wpl, info):
    """(loop, rest): whether a run of n keys, its first 64 wpl taken by the caller, enters
    tail_run's unpredicated loop (whole rounds of 64 kJoinTailU) and its predicated rest."""
    t = 64 * wpl
    if n <= t:
        return False, False
    rnd = 64 * info["j_tail_u"]
    return (n - t) >= rnd, (n - t) % rnd != 0


def part_items(qi0, qi1, part, nparts):
    """Items [i0, i1) of part `part` of a job whose partition has items [qi0, qi1) (join_job)."""
    return qi0 + (qi1 - qi0) * part // nparts, qi0 + (qi1 - qi0) * (part + 1) // nparts


def hash_pieces(rcnt, info):
    """Keys of each hash-table piece of one R descriptor batch (join_job: consecutive runs while
    the piece holds <= kJoinPiece keys; a single longer run is a piece of its own)."""
    pieces, acc = [], 0
    for c in rcnt:
        if acc + c > info["j_piece"] and acc > 0:
            pieces.append(acc)
            acc = 0
        acc += c
    pieces.append(acc)
    return pieces


def classify(tables, info, R_dup_per_job, jobs=None):
    """{(job, part): record} of the branch join_job must have taken, from the tables and constants.

    tables: r_sweep_start [F + 1], r_cnt [sweeps, NSUB], s_item_start [F + 1], surv_cnt
    [items, NSUB], surv_off [items, NSUB], nparts [jobs]. R_dup_per_job[job]: the job's R keys hold a
    duplicate (from the input, not from the device). jobs: the jobs to classify (default: all).

    record: cls "empty" | "fused" | "batched" | "hash"; start (hash only) "hash" | "dup_fused" |
    "dup_batched"; pieces (hash: keys per piece, over all R batches), r_batches, s_batches, r_tail /
    s_tail = (loop, rest) over the part's runs in the path that finished the job, s_walk (fused: survivor
    runs beyond those loaded with R's), formats (the set of survivor run formats of the part's items,
    1 packed / 0 codes), nh (PRH / PRHO: buckets per piece)."""
    NSUB = info["NSUB"]
    sw, it = tables["r_sweep_start"], tables["s_item_start"]
    rc = np.asarray(tables["r_cnt"]).reshape(-1, NSUB)
    sc = np.asarray(tables["surv_cnt"]).reshape(-1, NSUB)
    so = np.asarray(tables["surv_off"]).reshape(-1, NSUB)
    out = {}
    for job in (range(info["jobs"]) if jobs is None else jobs):
        q, s = job // NSUB, job % NSUB
        w0, w1, qi0, qi1 = int(sw[q]), int(sw[q + 1]), int(it[q]), int(it[q + 1])
        np_ = int(tables["nparts"][job])
        for part in range(np_):
            i0, i1 = part_items(qi0, qi1, part, np_)
            if w1 == w0 or i1 == i0:
                out[(job, part)] = {"cls": "empty"}
                continue
            rcnt = rc[w0:w1, s].tolist()
            scnt = sc[i0:i1, s].tolist()
            nRd, nSd = w1 - w0, i1 - i0
            dup = bool(R_dup_per_job[job])
            hashed = (not info["bitmap"]) or info["jkind"] != 0
            rec = {"r_batches": -(-nRd // info["j_desc"]), "s_batches": -(-nSd // info["j_desc"]),
                   "r_keys": sum(rcnt), "s_keys": sum(scnt), "r_runs": rcnt, "s_runs": scnt,
                   "formats": set(((so[i0:i1, s] >> 31) & 1).tolist())}
            if not hashed and nRd <= info["j_fused"] and nSd <= info["j_desc"]:
                rec["cls"], rec["start"] = ("hash", "dup_fused") if dup else ("fused", None)
            elif not hashed:
                rec["cls"], rec["start"] = ("hash", "dup_batched") if dup else ("batched", None)
            else:
                rec["cls"], rec["start"] = "hash", "hash"
            rw = info["j_fw"] if rec["cls"] == "fused" else info["j_rw"]
            rt = [_tail(n, rw, info) for n in rcnt]
            st = [_tail(n, info["j_sw"], info) for n in scnt]
            rec["r_tail"] = (any(a for a, _ in rt), any(b for _, b in rt))
            rec["s_tail"] = (any(a for a, _ in st), any(b for _, b in st))
            rec["s_walk"] = rec["cls"] == "fused" and nSd > info["j_waves"] * info["j_fs"]
            if rec["cls"] == "hash":
                rec["pieces"] = []
                for d0 in range(0, nRd, info["j_desc"]):
                    rec["pieces"] += hash_pieces(rcnt[d0:d0 + info["j_desc"]], info)
                if info["jkind"]:
                    rec["nh"] = []
                    for n in rec["pieces"]:
                        nh = 4
                        while nh * 4 < n:
                            nh <<= 1
                        rec["nh"].append(nh)
            out[(job, part)] = rec
    return out


def classify_mat(tables, info, R_dup_per_job, jobs=None):
    """{job: record} for k_join_mat: cls "empty" | "bitmap" | "hash1" (single shot: one R piece, one
    survivor batch) | "general" with r_batches, pieces (R pieces over all batches) and s_batches
    (survivor batches of kMatPiece per piece, over all descriptor batches); start "dup" when the
    bitmap path gave up on a duplicate."""
    NSUB = info["NSUB"]
    sw, it = tables["r_sweep_start"], tables["s_item_start"]
    rc = np.asarray(tables["r_cnt"]).reshape(-1, NSUB)
    sc = np.asarray(tables["surv_cnt"]).reshape(-1, NSUB)
    D, P = info["m_desc"], info["m_piece"]
    out = {}
    for job in (range(info["jobs"]) if jobs is None else jobs):
        q, s = job // NSUB, job % NSUB
        r0, r1, qi0, qi1 = int(sw[q]), int(sw[q + 1]), int(it[q]), int(it[q + 1])
        if r0 == r1 or qi0 == qi1:
            out[job] = {"cls": "empty"}
            continue
        rcnt, scnt = rc[r0:r1, s].tolist(), sc[qi0:qi1, s].tolist()
        rtot, stot = sum(rcnt), sum(scnt)
        rec = {"r_keys": rtot, "s_keys": stot, "start": None}
        single = r1 - r0 <= D and qi1 - qi0 <= D
        if single and info["bitmap"] and rtot <= info["m_rcap"]:
            if not R_dup_per_job[job]:
                rec.update(cls="bitmap", s_batches=-(-stot // info["m_rcap"]))
                out[job] = rec
                continue
            rec["start"] = "dup"
        if single and rtot <= P and stot <= P:
            rec.update(cls="hash1", pieces=1, s_batches=1)
        else:
            pieces = sum(-(-sum(rcnt[d:d + D]) // P) for d in range(0, r1 - r0, D))
            sb = sum(-(-sum(scnt[d:d + D]) // P) for d in range(0, qi1 - qi0, D))
            rec.update(cls="general", r_batches=-(-(r1 - r0) // D), pieces=pieces, s_batches=sb)
        out[job] = rec
    return out


# ------------------------------------------------- crafted relations of the pass-2 job tests
INT_MAX, INT_MIN = 2**31 - 1, -2**31
_GEOM = {}


def mat_geometry(hw, to_dev, args, name, nR):
    """tables_info of a materializing join of |R| = nR under args (throw-away keys); `name` names
    args in the cache, to_dev(array) puts a relation on the device."""
    if (name, nR) not in _GEOM:
        R = np.stack([np.arange(nR, dtype=np.int32), np.zeros(nR, dtype=np.int32)], 1)
        hw.join_materialize_device(to_dev(R), to_dev(R[:8]), args, capacity=64)
        _GEOM[(name, nR)] = hw.tables_info()
    return dict(_GEOM[(name, nR)])


def same_geometry(hw, to_dev, R, args, info):
    """A materializing join of this R and args reports the geometry the keys were crafted for."""
    hw.join_materialize_device(to_dev(R), to_dev(R[:8]), args, capacity=64)
    now = hw.tables_info()
    keys = ("mode", "format", "F", "NSUB", "sub_shift", "hash_shift", "nseg", "bitmap", "G", "CH", "BSW", "slot")
    assert {k: now[k] for k in keys} == {k: info[k] for k in keys}


def payloads(n, rng):
    """n distinct random int32 payloads, none of them INT_MIN (the outer joins' default null)."""
    p = np.unique(rng.integers(-2**31 + 1, 2**31, size=2 * n + 16))
    assert p.size >= n
    return rng.permutation(p)[:n]


def rel(keys, rng):
    keys = np.asarray(keys).astype(np.int64)
    return np.stack([keys, payloads(keys.size, rng)], 1).astype(np.int32).reshape(-1, 2)


def duplicates_on_both_sides(crc, args):
    """5,000 R keys three times each, with INT_MAX, INT_MIN, 0, -1 and the key whose code is the
    kernels' empty-slot value; S holds key i (i mod 5) times (the special keys 0 to 4 times) and
    7,000 keys R lacks. info: special (the five keys), hits (S rows per R key)."""
    rng = np.random.default_rng(21)
    special = np.array([INT_MAX, INT_MIN, 0, -1, int(crc.key_of(0xFFFFFFFF))], dtype=np.int64)
    rest = np.setdiff1d(rng.choice(np.arange(-10**6, 10**6), 6000, replace=False), special)[:5000 - special.size]
    keys = np.concatenate([special, rest])
    assert np.unique(keys).size == 5000
    hits = np.concatenate([[0, 1, 2, 3, 4], np.arange(keys.size - 5) % 5])
    Rk = np.repeat(keys, 3)
    Sk = np.concatenate([np.repeat(keys, hits), rng.integers(2 * 10**6, 3 * 10**6, size=7000)])
    rng.shuffle(Rk)
    rng.shuffle(Sk)
    return rel(Rk, rng), rel(Sk, rng), args, {"special": special, "hits": hits}


def hot_r_key_across_pieces(crc, args, geometry):
    """One job holds an R key 2 kMatPiece + 5 times, keys 11, 12, 13 and six keys no S row has (three
    at the head of R, three at its tail: the job's first and last pieces), more than kMatRCap tuples.
    Its survivors: 40 of the hot key, 10 of 11, 10 of 12, none of 13, 50 of keys R lacks.
    geometry(nR) gives the tables_info the codes are crafted for; info is that, with the job (q0,
    sub0) and `hot`, the hot key's R rows."""
    rng = np.random.default_rng(33)
    nR = 20000
    info = geometry(nR)
    q0, sub0 = 17, 1
    hot = 2 * info["m_piece"] + 5
    rv = np.concatenate([np.full(hot, 7), [11, 12, 13]])
    lone = 2000 + np.arange(6)
    assert rv.size + lone.size >= info["m_rcap"] + 1
    nf = nR - rv.size - lone.size
    fill = filler_codes(info, nf + 3000, {q0}, 1)  # distinct: R takes the first nf
    mid = np.concatenate([job_codes(info, q0, sub0, rv), fill[:nf]])
    rng.shuffle(mid)
    lc = job_codes(info, q0, sub0, lone)
    Rc = np.concatenate([lc[:3], mid, lc[3:]])
    sv = np.concatenate([np.full(40, 7), np.repeat([11, 12], 10), 1000 + np.arange(50)])
    Sc = np.concatenate([job_codes(info, q0, sub0, sv), fill[nf - 3000:]])  # 3,000 of R's, 3,000 not
    rng.shuffle(Sc)
    info.update(q0=q0, sub0=sub0, hot=hot)
    return rel(crc.key_of(Rc), rng), rel(crc.key_of(Sc), rng), args, info


def more_descriptors_than_a_batch(crc, args, geometry):
    """A partition of kMatDesc * BSW * 32 + 1 R tuples (more than kMatDesc build sweeps: several R
    descriptor batches per job), 60,000 distinct keys repeated all over it; S has rows of 50,000 of
    them only. info: the geometry, with q0 (the partition), n_q (its R tuples), member (its 60,000 codes) and
    the shuffled code columns Rc, Sc."""
    rng = np.random.default_rng(55)
    q0, fill = 5, 20000
    probe = geometry(8)
    n_q = probe["m_desc"] * probe["BSW"] * 32 + 1
    nR = n_q + fill
    info = geometry(nR)
    assert (info["m_desc"], info["BSW"]) == (probe["m_desc"], probe["BSW"])
    lf = info["F"].bit_length() - 1
    hi = rng.choice(1 << min(32 - lf, 24), 66000, replace=False).astype(np.uint64)
    qcodes = (np.uint64(q0) | (hi << np.uint64(lf))).astype(np.uint32)
    member, absent = qcodes[:60000], qcodes[60000:]
    Rc = np.concatenate([member[rng.integers(0, member.size, size=n_q)], filler_codes(info, fill, {q0}, 1)])
    Sc = np.concatenate([member[rng.integers(0, 50000, size=3000)], absent[rng.integers(0, absent.size, size=3000)],
                         Rc[n_q:n_q + 3000], filler_codes(info, 3000, {q0}, 777)])
    rng.shuffle(Rc)
    rng.shuffle(Sc)
    info.update(q0=q0, n_q=n_q, member=member, Rc=Rc, Sc=Sc)
    return rel(crc.key_of(Rc), rng), rel(crc.key_of(Sc), rng), args, info
