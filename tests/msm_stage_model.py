"""Exact model of the MSM stages behind the sort (csrc/msm.h, csrc/msm_curve.inc.h) and the ctypes side of
tests/arith/msm_stage_hooks.hip.  Test infrastructure of test_msm_stages.py.

Every point the stages see is a known multiple of the generator, so the model works on integers mod r and turns an
expected scalar into a point only for the comparison (cpu_ref.g1_mul_batch / g2_mul_batch).  Nothing has a tolerance:
points are compared as canonical affine bytes in the storage form, slot and chunk sets as index sets.

Restated here from msm.h and the kernel comments, never read back from the hooks:

  segments   S = max(MSM_MIN_SEG, ceil(M / lanes)): lane l owns the sorted positions [l S, (l + 1) S)
  slots      bucket g with entries [lo, hi) owns the partial slots g + lo div S ... g + (hi - 1) div S, one per lane
             that holds one of its entries; an empty bucket owns none
  hot        a bucket with more than MSM_SMALL_MULTI slots is on the hot list; k_combine_large sums ALL of its slots
             into the first one, which is the only one k_bucket_reduce then reads
  red_chunk  msm_red_chunk: total = nbatch nproof D B buckets per launch; 65536 threads, or 32768 for a hidden launch of
             <= 2^17 buckets per rank; chunk = total div (threads world), within [1, 16]; world > 1: rounded down to a
             power of two and to at most one level-1 sort partition
  chunks     cps = ceil(B / red_chunk) per set, sets = D nproof, chunk q = set q div cps, buckets
             [lo, min(lo + red_chunk, B)) with lo = (q mod cps) red_chunk;  nblk = clamp(ceil((cps div world) / 256), 1, 256)
  contrib    contrib[q] = sum (b + 1) K_b over the chunk's buckets, K_b = the sum of the bucket's slots; a sharded rank
             writes the chunks range[4] div red_chunk ... ceil(range[5] / red_chunk) - 1 only
  wsum       wsum[set] = the sum of the set's (written) contributions
  output     proof z, workspace slot k: sum_d 2^(c d) wsum[z D + d], at z out_stride bytes + k records
  accumulate slot g + l = sum of +- k_idx 2^(c D plane) over the entries of bucket g in lane l with idx >= idx_min whose
             point is finite; a (bucket, lane) pair without entries is never written
"""
import ctypes as C
import os

import numpy as np

import bn254_ref as o
import cpu_ref
import sort_model as SM

ROOT = SM.ROOT
GPU_HOOKS = os.path.join(ROOT, "tests", "arith", "libg16_msmstage_gpu.so")
R = o.R_MOD
MSM_MIN_SEG, MSM_SMALL_MULTI = SM.MSM_MIN_SEG, SM.MSM_SMALL_MULTI
MSM_RED_CHUNK = 16                      # msm.h: max buckets per thread of k_bucket_reduce
SUM_THREADS = 128                       # msm_curve.inc.h: workgroup of k_set_sum
CODE_INF, CODE_POISON = -1, -2
GEO_WORDS, ACC_WORDS = 12, 8
PER_ELEMENT_MAX = 3000                  # larger point arrays are compared by one random linear combination first


def seg_len(M, lanes):
    """msm.h msm_seg_len"""
    return max(MSM_MIN_SEG, -(-M // lanes))


def red_chunk(cfg, nbatch=1, world=1, hidden=False):
    """msm.h msm_red_chunk; nbatch counts every MSM of the launch (workspace slots x proofs)"""
    total = nbatch * cfg.D * cfg.B
    target = 32768 if hidden and total // world <= 1 << 17 else 65536
    ch = min(max(total // (target * world), 1), MSM_RED_CHUNK)
    if world > 1:
        ch = 1 << (ch.bit_length() - 1)
        ch = min(ch, 1 << SM.part_shift(cfg.nb))
    return ch


class Geometry:
    """what reduce_plan (msm_curve.inc.h) derives from the sort, the workspace and (nbatch, hidden)"""

    def __init__(self, cfg, nproof, nbatch, world, hidden, M, lanes):
        self.red_chunk = red_chunk(cfg, nbatch * nproof, world, hidden)
        self.cps = -(-cfg.B // self.red_chunk)
        self.sets = cfg.D * nproof
        self.nchunks = self.cps * self.sets
        self.nblk = min(max(-(-(self.cps // world) // (2 * SUM_THREADS)), 1), 256)
        self.S = seg_len(M, lanes)
        self.lanes, self.M = lanes, M
        self.slots = nproof * cfg.nb + lanes

    def words(self):
        return [self.red_chunk, self.cps, self.nchunks, self.nblk, self.sets, self.S, self.lanes, self.slots]


def slot_layout(offset, S):
    """-> (first, n): bucket g's partials live in slots first[g] ... first[g] + n[g] - 1"""
    off = np.asarray(offset, dtype=np.int64)
    lo, hi = off[:-1], off[1:]
    l0, l1 = lo // S, (np.maximum(hi, 1) - 1) // S
    n = np.where(hi > lo, l1 - l0 + 1, 0)
    first = np.arange(lo.size, dtype=np.int64) + l0
    return first, n


def owned_slots(first, n, slots):
    """bool per slot: some bucket owns it (the layout never hands a slot to two buckets: asserted)"""
    d = np.zeros(slots + 1, dtype=np.int64)
    live = n > 0
    np.add.at(d, first[live], 1)
    np.add.at(d, first[live] + n[live], -1)
    own = np.cumsum(d)[:slots]
    assert own.max(initial=0) <= 1 and int(first[live].max(initial=0)) < slots
    return own.astype(bool)


# ---- curves -------------------------------------------------------------------------------------------------------
class Curve:
    def __init__(self, name, size, gen, mul_batch, msm):
        self.name, self.size, self.gen, self._mul, self._msm = name, size, gen, mul_batch, msm

    def points(self, ks):
        """[k G] as (n, size) uint8, canonical affine storage form; k = 0 mod r: all-zero (infinity)"""
        ks = [int(k) % R for k in ks]
        out = np.zeros((len(ks), self.size), dtype=np.uint8)
        live = [i for i, k in enumerate(ks) if k]
        if live:
            out[live] = self._mul(self.gen, [ks[i] for i in live])
        return out

    def combine(self, pts, coeff):
        """sum coeff_i pts_i as bytes"""
        mont = np.frombuffer(b"".join(o.fr_to_mont_bytes(int(v)) for v in coeff), dtype=np.uint64).reshape(-1, 4).copy()
        return self._msm(np.ascontiguousarray(pts), mont)

    def lambdas(self, values):
        """field elements in the storage form: Fq as ints, Fq2 as pairs"""
        if self.size == 64:
            return np.frombuffer(b"".join(o.fq_to_mont_bytes(v) for v in values), dtype=np.uint8).copy()
        return np.frombuffer(b"".join(o.fq_to_mont_bytes(c) for v in values for c in v), dtype=np.uint8).copy()


G1 = Curve("g1", 64, o.g1_to_bytes(o.G1_GEN), cpu_ref.g1_mul_batch, cpu_ref.msm_g1)
G2 = Curve("g2", 128, o.g2_to_bytes(o.G2_GEN), cpu_ref.g2_mul_batch, cpu_ref.msm_g2)


def first_mismatch(curve, dev, want_k, live=None, seed=1):
    """index of the first element of dev (n, size) that is not want_k[i] G, or None.  live: bool per element to compare.
    More than PER_ELEMENT_MAX elements: one random linear combination with seeded 64-bit coefficients decides, and only
    a mismatch pays for the per-element pass that names the element"""
    idx = np.arange(len(want_k)) if live is None else np.nonzero(live)[0]
    if idx.size == 0:
        return None
    ks = [int(want_k[i]) % R for i in idx]
    if idx.size > PER_ELEMENT_MAX:
        coeff = np.random.default_rng(seed).integers(1, 1 << 63, size=idx.size, dtype=np.uint64) * 2 + 1
        total = sum(int(a) * k for a, k in zip(coeff, ks)) % R
        if curve.combine(dev[idx], coeff) == curve.points([total])[0].tobytes():
            return None
    want = curve.points(ks)
    bad = np.nonzero((want != dev[idx]).any(axis=1))[0]
    return int(idx[bad[0]]) if bad.size else None


# ---- reduction ----------------------------------------------------------------------------------------------------
class Pool:
    """the points synthetic partials are made of: signed multipliers of the generator, small enough that every chunk
    contribution of the model fits an int64.  The LAST point is the poison: it sits in every slot no bucket owns and
    in the slots of a hot bucket behind its first one -- wherever a reduction must not read"""

    def __init__(self, curve, ks, lambdas):
        self.curve = curve
        self.k = np.asarray(ks, dtype=np.int64)
        assert np.abs(self.k).max() < 1 << 21 and self.k[-1] != 0
        self.points = curve.points(self.k)
        self.nlam = len(lambdas)
        self.lam = curve.lambdas(lambdas)

    def code(self, point, lam):
        return point + len(self.k) * lam

    def value(self, codes):
        """multiplier per code (0 for infinity)"""
        c = np.asarray(codes, dtype=np.int64)
        c = np.where(c == CODE_POISON, len(self.k) - 1, c)
        return np.where(c >= 0, self.k[np.maximum(c, 0) % len(self.k)], 0)


def bucket_sums(pool, codes, first, n):
    """K_b per bucket for one workspace slot's codes: the sum over all of the bucket's slots (hot or not)"""
    cs = np.concatenate([[0], np.cumsum(pool.value(codes))])
    return cs[first + n] - cs[first]


def chunk_contribs(K, cfg, geo, nproof):
    """int64 (sets, cps): sum (b + 1) K_b over each chunk"""
    rc, cps, B = geo.red_chunk, geo.cps, cfg.B
    wk = K.reshape(geo.sets, B) * np.arange(1, B + 1, dtype=np.int64)
    pad = np.zeros((geo.sets, cps * rc), dtype=np.int64)
    pad[:, :B] = wk                                       # the ragged last chunk: buckets past B do not exist
    assert np.abs(K).max(initial=0) * B * rc < 1 << 62
    return pad.reshape(geo.sets, cps, rc).sum(axis=2)


def written_chunks(geo, rng_words):
    """bool per chunk: the ones k_bucket_reduce writes (all, or a sharded rank's run)"""
    w = np.ones(geo.nchunks, dtype=bool)
    if rng_words is not None:
        q_lo, q_hi = int(rng_words[4]) // geo.red_chunk, -(-int(rng_words[5]) // geo.red_chunk)
        w[:] = False
        w[q_lo:max(q_hi, q_lo)] = True
    return w


def set_sums(contrib, written, geo):
    """Python ints per set"""
    c = np.where(written.reshape(geo.sets, geo.cps), contrib, 0)
    return [sum(int(v) for v in row) for row in c]


def outputs(wsum, cfg, nproof):
    return [sum(wsum[z * cfg.D + d] << (cfg.c * d) for d in range(cfg.D)) % R for z in range(nproof)]


def describe_chunk(q, cfg, geo, first, n):
    """set, lo and bucket occupancy of chunk q, for a failure message"""
    st, lo = q // geo.cps, (q % geo.cps) * geo.red_chunk
    hi = min(lo + geo.red_chunk, cfg.B)
    g = st * cfg.B + np.arange(lo, hi)
    return (f"chunk {q}: set {st}, lo {lo}, buckets [{lo}, {hi}), partials per bucket {n[g].tolist()}, "
            f"first slots {first[g].tolist()}")


# ---- accumulation -------------------------------------------------------------------------------------------------
def accumulate_expected(offset, entries, S, cfg, ks, idx_min):
    """{slot: multiplier mod r} for every (bucket, lane) pair that holds an entry.  ks[i]: the multiplier of point i of
    the query (None: the point at infinity); entry idx names point idx - idx_min"""
    off = np.asarray(offset, dtype=np.int64)
    M = int(off[-1])
    bucket = np.repeat(np.arange(off.size - 1, dtype=np.int64), np.diff(off))
    slot = bucket + np.arange(M, dtype=np.int64) // S
    mask = (1 << cfg.idx_bits) - 1
    out = {}
    for s, e in zip(slot.tolist(), np.asarray(entries, dtype=np.uint32).tolist()):
        idx, plane, neg = e & mask, (e & 0x7fffffff) >> cfg.idx_bits, e >> 31
        v = out.get(s, 0)
        if idx >= idx_min and ks[idx - idx_min] is not None:
            t = ks[idx - idx_min] << (cfg.c * cfg.D * plane)
            v += -t if neg else t
        out[s] = v
    return {s: v % R for s, v in out.items()}


def reduce_model(slot_k, offset, S, cfg, nproof, hidden=False, world=1, nbatch=1):
    """the model's reduction over a {slot: multiplier} map (Python ints): the single output of proof 0.  The chunk
    structure is kept -- contributions first, then set sums, then Horner -- so that this is the same code path of the
    model the reduction tests rely on, with exact integers in place of int64"""
    first, n = slot_layout(offset, S)
    K = [sum(slot_k.get(int(f) + j, 0) for j in range(int(c))) for f, c in zip(first, n)]
    rc = red_chunk(cfg, nbatch * nproof, world, hidden)
    wsum = []
    for st in range(cfg.D * nproof):
        contrib = [sum((b + 1) * K[st * cfg.B + b] for b in range(lo, min(lo + rc, cfg.B))) for lo in range(0, cfg.B, rc)]
        wsum.append(sum(contrib))
    return outputs(wsum, cfg, nproof)


# ---- the hook library ---------------------------------------------------------------------------------------------
class Result:
    pass


class Hooks:
    def __init__(self, cdll, sort_hooks):
        self.L, self.sort = cdll, sort_hooks
        vp, u32, u64, i = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
        for name in ("g16_test_stage_reduce_g1", "g16_test_stage_reduce_g2"):
            f = getattr(cdll, name)
            f.restype = i
            f.argtypes = [vp, u32, i, i, i, u32, u64, i, i, u32, u32, u32, i, u64, vp, u32, vp, u32, vp, u64, u32, vp,
                          vp, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, C.c_char_p, C.c_size_t]
        for name in ("g16_test_stage_acc_g1", "g16_test_stage_acc_g2"):
            f = getattr(cdll, name)
            f.restype = i
            f.argtypes = [vp, u32, i, i, i, u32, u32, vp, vp, u32, u32, i, vp, vp, vp, u64, vp, vp, u64, C.c_char_p,
                          C.c_size_t]
        cdll.g16_test_stage_plan.restype = i
        cdll.g16_test_stage_plan.argtypes = [u64, i, i, u32, u32, i, i, vp]

    def config(self, length, c=0, planes=0):
        return self.sort.config(length, c, planes)

    def plan(self, length, c, planes, nbatch=1, nproof=1, world=1, hidden=False):
        """-> (red_chunk, default lanes, default lanes2, MSM_FIX_CAP) of this build"""
        out = np.zeros(4, dtype=np.uint32)
        assert self.L.g16_test_stage_plan(length, c, planes, nbatch, nproof, world, int(hidden), out.ctypes.data) == 0
        return [int(v) for v in out]

    @staticmethod
    def _scalars(proofs, mont, stride):
        nproof, n1 = len(proofs), proofs[0].shape[0]
        stride = stride if nproof > 1 else 0
        assert nproof == 1 or stride >= n1
        buf = np.full(((nproof - 1) * stride + n1, 8), 0xa5a5a5a5, dtype=np.uint32)
        for z, p in enumerate(proofs):
            buf[z * stride:z * stride + n1] = SM.to_mont_words(p) if mont else p
        return buf, n1, nproof, stride

    def reduce(self, curve, proofs, mont, c, planes, pool, codes, nbatch=1, hidden=False, out_stride=0, stride=0,
               rank=0, world=1, lanes=0, lanes2=0, contrib_pad=5):
        """codes: (nbatch, slots) int32.  Returns the geometry words, offset, the hot list, range, and contrib / wsum /
        the output sums as affine bytes with their poison flags"""
        buf, n1, nproof, stride = self._scalars(proofs, mont, stride)
        cfg = self.config(n1, c, planes)
        nbt = nproof * cfg.nb
        codes = np.ascontiguousarray(codes, dtype=np.int32)
        assert codes.shape[0] == nbatch
        rc = self.plan(n1, c, planes, nbatch, nproof, world, hidden)[0]
        nchunks = -(-cfg.B // rc) * cfg.D * nproof
        ncontrib, wsets, sz = nchunks + contrib_pad, cfg.D * nproof + 1, curve.size
        r = Result()
        geo = np.zeros(GEO_WORDS, dtype=np.uint32)
        r.offset = np.full(nbt + 1, 0x5a5a5a5a, dtype=np.uint32)
        hot_cap = nproof * n1 * cfg.W // (MSM_MIN_SEG * MSM_SMALL_MULTI) + 2
        hot = np.zeros(hot_cap, dtype=np.uint32)
        r.range = np.full(6, 0x5a5a5a5a, dtype=np.uint32)
        r.contrib = np.full((nbatch * ncontrib, sz), 0x77, dtype=np.uint8)
        r.contrib_flag = np.full(nbatch * ncontrib, 9, dtype=np.uint8)
        r.wsum = np.full((nbatch * wsets, sz), 0x77, dtype=np.uint8)
        r.wsum_flag = np.full(nbatch * wsets, 9, dtype=np.uint8)
        r.sums = np.full((nproof * nbatch, sz), 0x77, dtype=np.uint8)
        r.sums_flag = np.full(nproof * nbatch, 9, dtype=np.uint8)
        gap = C.c_uint64(1 << 63)
        msg = C.create_string_buffer(256)
        fn = self.L.g16_test_stage_reduce_g1 if curve is G1 else self.L.g16_test_stage_reduce_g2
        st = fn(buf.ctypes.data, n1, int(mont), c, planes, nproof, stride, rank, world, lanes, lanes2, nbatch,
                int(hidden), out_stride, pool.points.ctypes.data, len(pool.k), pool.lam.ctypes.data, pool.nlam,
                codes.ctypes.data, codes.size, contrib_pad, geo.ctypes.data, r.offset.ctypes.data, hot.ctypes.data,
                hot_cap, r.range.ctypes.data, r.contrib.ctypes.data, r.contrib_flag.ctypes.data, r.wsum.ctypes.data,
                r.wsum_flag.ctypes.data, r.sums.ctypes.data, r.sums_flag.ctypes.data, C.byref(gap), msg, len(msg))
        assert st == 0, f"stage reduce hook returned {st}: {msg.value.decode()}"
        r.geo = [int(v) for v in geo]
        assert r.geo[8] == ncontrib and r.geo[9] == wsets and r.geo[2] == nchunks
        r.ncontrib, r.wsets, r.gap_dirty = ncontrib, wsets, gap.value
        r.hot = hot[:r.geo[11]]
        r.cfg = cfg
        return r

    def accumulate(self, curve, words, mont, c, planes, pts_a, pts_b=None, idx_min=0, mode=0, lanes=0, lanes2=0):
        """one sort of `words`, one accumulation.  pts: (npts, size) uint8 storage-form points (all-zero: infinity)"""
        n1 = words.shape[0]
        buf = SM.to_mont_words(words) if mont else np.ascontiguousarray(words)
        cfg = self.config(n1, c, planes)
        dl = self.plan(n1, c, planes)
        lane_count = (lanes2 or dl[2]) if curve is G2 else (lanes or dl[1])
        slots = cfg.nb + lane_count
        batch = 2 if mode == 3 else 1
        r = Result()
        info = np.zeros(ACC_WORDS, dtype=np.uint32)
        r.offset = np.full(cfg.nb + 1, 0x5a5a5a5a, dtype=np.uint32)
        ecap = max(n1 * cfg.W, 1)
        entries = np.full(ecap, 0x5a5a5a5a, dtype=np.uint32)
        r.partial = np.full((batch * slots, curve.size), 0x77, dtype=np.uint8)
        r.flag = np.full(batch * slots, 9, dtype=np.uint8)
        pts_a = np.ascontiguousarray(pts_a, dtype=np.uint8)
        npts = pts_a.shape[0]
        if pts_b is not None:
            pts_b = np.ascontiguousarray(pts_b, dtype=np.uint8)
            assert pts_b.shape == pts_a.shape
        msg = C.create_string_buffer(256)
        fn = self.L.g16_test_stage_acc_g1 if curve is G1 else self.L.g16_test_stage_acc_g2
        st = fn(buf.ctypes.data, n1, int(mont), c, planes, lanes, lanes2, pts_a.ctypes.data,
                pts_b.ctypes.data if pts_b is not None else None, npts, idx_min, mode, info.ctypes.data,
                r.offset.ctypes.data, entries.ctypes.data, ecap, r.partial.ctypes.data, r.flag.ctypes.data,
                batch * slots, msg, len(msg))
        assert st == 0, f"stage accumulate hook returned {st}: {msg.value.decode()}"
        r.S, r.lanes, r.slots, r.M = (int(v) for v in info[:4])
        r.overflow, r.fix_cap, r.batch = [int(info[4]), int(info[5])], int(info[6]), int(info[7])
        assert r.slots == slots and r.batch == batch and r.lanes == lane_count
        r.entries = entries[:r.M]
        r.cfg = cfg
        r.partial = r.partial.reshape(batch, slots, curve.size)
        r.flag = r.flag.reshape(batch, slots)
        return r


def load_hooks(request):
    """the module fixture's body: "emu" = the hooks inside the emulator library, "gpu" = the hipcc build, which
    build() leaves next to the source -- missing there is a failure, never a skip or a compile"""
    if request.param == "emu":
        lib = request.getfixturevalue("emu").L
        return Hooks(lib, SM.Hooks(lib))
    import pytest
    for path in (GPU_HOOKS, SM.GPU_HOOKS):
        if not os.path.exists(path):
            pytest.fail(f"{path} is not built (make -C circom_compat_amd/csrc)")
    return Hooks(C.CDLL(GPU_HOOKS), SM.Hooks(C.CDLL(SM.GPU_HOOKS)))
