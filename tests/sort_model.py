"""Exact integer model of MsmSort (csrc/msm_sort.hip) and the ctypes side of tests/arith/sort_hooks.hip.

Test infrastructure of test_msm_sort.py.  Everything is integer arithmetic in numpy, vectorised over the scalars;
nothing has a tolerance.  The model restates, from msm.h and msm_sort.hip:

  digits   raw = ((x >> c w) & (2^c - 1)) + carry;  raw > 2^(c-1): mag = 2^c - raw, negative, carry 1;  otherwise
           mag = raw, positive, carry 0;  mag = 0 emits nothing;  the carry out of window W - 1 is 0
  pair     bucket g = z nb1 + (w mod D) B + mag - 1,  entry = i | (w div D) << idx_bits | neg << 31
  count    pairs per bucket;  offset = its exclusive prefix sum, offset[nb] = the total M
  entries  entries[offset[g] : offset[g+1]) is bucket g's entries in any order
  hot      S = max(MSM_MIN_SEG, ceil(M / lanes));  g is listed iff it is non-empty and spans more than
           MSM_SMALL_MULTI segments: (offset[g+1] - 1) div S - offset[g] div S + 1 > MSM_SMALL_MULTI
  shards   partition p = buckets [p << sh, (p+1) << sh);  cut g = the partition boundary whose prefix is closest to
           floor(g M / world), ties down (k_pick_range's bisection, restated in pick_cut)
"""
import ctypes as C
import os

import numpy as np

import bn254_ref as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_HOOKS = os.path.join(ROOT, "tests", "arith", "libg16_sort_gpu.so")

R_MOD = o.R_MOD
MONT = (1 << 256) % R_MOD               # Fr's Montgomery radix (field.h: 8 x 32-bit words)
MSM_MIN_SEG = 8                         # msm.h: shortest per-lane segment
MSM_SMALL_MULTI = 32                    # msm.h: buckets with <= this many partials are summed inside the reduce
MSM_PART_BITS_MAX = 12                  # msm.h
P2_BINS = 4096                          # msm_sort.hip: buckets of the level-2 LDS histogram
P2_CHUNK, P2S_CHUNK, P1_TILE = 16384, 8192, 2048
CFG_WORDS = 11
PART_OFF_WORDS = (1 << MSM_PART_BITS_MAX) + 1


class Config:
    """msm_make_config's answer as the hook reports it; what follows from c, D and Pn is recomputed and compared"""

    def __init__(self, w):
        (self.c, self.W, self.Pn, self.D, self.B, self.idx_bits, self.lanes, self.lanes2, self.nb, self.sh,
         self.part_bits) = (int(x) for x in w)
        c = self.c
        assert self.W == -(-255 // c)
        assert self.B == 1 << (c - 1)
        assert self.nb == self.D * self.B
        assert self.part_bits == part_bits(self.nb)
        assert self.sh == part_shift(self.nb)
        assert self.idx_bits == (27 if self.Pn <= 16 else 26)


def part_bits(nb):
    """msm.h msm_part_bits: 2^10 partitions, more (up to 2^12) while one would span more than 4096 buckets"""
    bits = 10
    while bits < MSM_PART_BITS_MAX and -(-nb // (1 << bits)) > P2_BINS:
        bits += 1
    return bits


def part_shift(nb):
    """msm.h msm_part_shift: partition = bucket >> shift"""
    bits = max(nb - 1, 0).bit_length()                   # smallest bits with 2^bits >= nb
    return max(bits - part_bits(nb), 0)


# ---- scalars ------------------------------------------------------------------------------------------------------
def to_words(values):
    """canonical integers < 2^256 -> (n, 8) uint32 words, little endian"""
    raw = b"".join(int(v).to_bytes(32, "little") for v in values)
    return np.frombuffer(raw, dtype=np.uint32).reshape(len(values), 8).copy()


def from_words(words):
    b = np.ascontiguousarray(words, dtype=np.uint32).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def to_mont_words(words):
    """the Montgomery form x 2^256 mod r of canonical words (what the prover's witness holds)"""
    return to_words([v * MONT % R_MOD for v in from_words(words)])


def random_words(rng, n):
    """n canonical scalars below 2^253 (< r), every lower bit uniform"""
    w = rng.integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)
    w[:, 7] &= (1 << 21) - 1
    return w


# ---- the model ----------------------------------------------------------------------------------------------------
def pairs(words, cfg, bucket_base=0):
    """every (bucket, entry) pair of one scalar vector, as two uint32 arrays (window-major order)"""
    n = words.shape[0]
    c, W, D = cfg.c, cfg.W, cfg.D
    assert n <= 1 << cfg.idx_bits and (W - 1) // D < 1 << (31 - cfg.idx_bits)
    assert not (words[:, 7] >> 30).any()                 # below 2^254 (> r): no bit above window W - 1 is lost
    ext = np.zeros((n, 10), dtype=np.uint64)
    ext[:, :8] = words
    idx = np.arange(n, dtype=np.uint64)
    half, mask = np.uint64(1 << (c - 1)), np.uint64((1 << c) - 1)
    carry = np.zeros(n, dtype=np.uint64)
    gs, es = [], []
    for w in range(W):
        k, s = divmod(c * w, 32)
        raw = (((ext[:, k] | (ext[:, k + 1] << np.uint64(32))) >> np.uint64(s)) & mask) + carry
        neg = raw > half
        mag = np.where(neg, np.uint64(1 << c) - raw, raw)
        carry = neg.astype(np.uint64)
        live = mag != 0
        g = np.uint64(bucket_base + (w % D) * cfg.B) + mag - np.uint64(1)
        e = idx | np.uint64((w // D) << cfg.idx_bits) | (carry << np.uint64(31))
        gs.append(g[live])
        es.append(e[live])
    assert not carry.any(), "a scalar's top window carries out: not a value the sort is specified for"
    return np.concatenate(gs).astype(np.uint32), np.concatenate(es).astype(np.uint32)


def chunk_pairs(proofs, cfg, keep=None):
    """proofs: one (n1, 8) word array per proof; proof z's buckets start at z nb1.  keep: bool per point index"""
    gs, es = [], []
    for z, words in enumerate(proofs):
        g, e = pairs(words, cfg, z * cfg.nb)
        if keep is not None:
            live = np.asarray(keep, dtype=bool)[e & np.uint32((1 << cfg.idx_bits) - 1)]
            g, e = g[live], e[live]
        gs.append(g)
        es.append(e)
    return np.concatenate(gs), np.concatenate(es)


class Expected:
    """count / offset / the entry list in (bucket, entry) order, for nbt buckets"""

    def __init__(self, g, e, nbt):
        self.nbt = nbt
        self.count = np.bincount(g, minlength=nbt).astype(np.uint32)
        assert self.count.size == nbt
        self.offset = np.zeros(nbt + 1, dtype=np.uint64)
        np.cumsum(self.count, out=self.offset[1:])
        self.M = int(self.offset[nbt])
        assert self.M < 1 << 32
        key = np.sort((g.astype(np.uint64) << np.uint64(32)) | e.astype(np.uint64))
        self.sorted_entries = (key & np.uint64(0xffffffff)).astype(np.uint32)

    def restricted(self, b_lo, b_hi):
        """a bucket-sharded rank's view: the pairs of buckets [b_lo, b_hi) only"""
        r = object.__new__(Expected)
        r.nbt = self.nbt
        r.count = self.count.copy()
        r.count[:b_lo] = 0
        r.count[b_hi:] = 0
        r.offset = np.zeros(self.nbt + 1, dtype=np.uint64)
        np.cumsum(r.count, out=r.offset[1:])
        r.M = int(r.offset[self.nbt])
        r.sorted_entries = self.sorted_entries[int(self.offset[b_lo]):int(self.offset[b_hi])]
        return r

    def spans(self, lanes):
        """segments every bucket's entries span when the list is cut into `lanes` equal runs (0: empty bucket)"""
        S = np.uint64(max(MSM_MIN_SEG, -(-self.M // lanes)))
        lo, hi = self.offset[:-1], self.offset[1:]
        np_ = (np.maximum(hi, np.uint64(1)) - np.uint64(1)) // S - lo // S + np.uint64(1)
        return np.where(hi > lo, np_, np.uint64(0))

    def hot(self, lanes):
        return set(np.nonzero(self.spans(lanes) > MSM_SMALL_MULTI)[0].tolist())


def part_offsets(count, sh):
    """prefix sums of the pairs per level-1 partition: bins1 + 1 values"""
    nb = count.size
    bins1 = ((nb - 1) >> sh) + 1
    per =np.add.reduceat(count.astype(np.uint64), np.arange(0, nb, 1 << sh))
    assert per.size == bins1
    off = np.zeros(bins1 + 1, dtype=np.uint64)
    np.cumsum(per, out=off[1:])
    return off


def pick_cut(part_off, g, world):
    """k_pick_range: the start of rank g's run of partitions"""
    bins1 = len(part_off) - 1
    if g <= 0:
        return 0
    if g >= world:
        return bins1
    M = int(part_off[bins1])
    tgt = M * g // world
    lo, hi = 0, bins1                     # part_off[lo] <= tgt < part_off[hi] (or lo = hi - 1 at the top)
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if int(part_off[mid]) <= tgt:
            lo = mid
        else:
            hi = mid
    return lo if tgt - int(part_off[lo]) <= int(part_off[hi]) - tgt else hi     # ties go down


def closest_cut(part_off, g, world):
    """the same cut WITHOUT the bisection: among the boundaries closest to floor(g M / world) -- the bisection only
    ever compares the two that bracket the target, and a tie between them goes down -- the answer must be one"""
    bins1 = len(part_off) - 1
    tgt = int(part_off[bins1]) * g // world
    d = [abs(int(x) - tgt) for x in part_off]
    return {p for p in range(bins1 + 1) if d[p] == min(d)}


def shard_range(part_off, rank, world, sh, nb):
    lo = pick_cut(part_off, rank, world)
    hi = max(pick_cut(part_off, rank + 1, world), lo)
    return [lo, hi, int(part_off[lo]), int(part_off[hi]) - int(part_off[lo]), min(lo << sh, nb), min(hi << sh, nb)]


def chunk_spans(expected, part_off, sh, chunk):
    """buckets every `chunk`-entry slice of the partition-ordered list spans, as k_bucket_count / k_bucket_scatter
    compute it from the first and last pair's partition (the order inside a partition does not matter)"""
    M = int(part_off[-1])
    lo = np.arange(0, M, chunk, dtype=np.uint64)
    hi = np.minimum(lo + np.uint64(chunk), np.uint64(M))
    p_lo = np.searchsorted(part_off, lo, side="right") - 1
    p_hi = np.searchsorted(part_off, hi - np.uint64(1), side="right") - 1
    return ((p_hi + 1) << sh) - (p_lo << sh)


# ---- the hook library ---------------------------------------------------------------------------------------------
class Result:
    pass


class Hooks:
    def __init__(self, cdll):
        self.L = cdll
        vp, u32, u64, i = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
        cdll.g16_test_sort_config.restype = i
        cdll.g16_test_sort_config.argtypes = [u64, i, i, vp]
        cdll.g16_test_sort_init.restype = i
        cdll.g16_test_sort_init.argtypes = [u64, i, i, u32, C.c_char_p, C.c_size_t]
        cdll.g16_test_sort_run.restype = i
        cdll.g16_test_sort_run.argtypes = [vp, u32, i, i, i, u32, u64, i, i, u32, u32, vp, u32, u32, vp, vp, vp, vp,
                                           u64, vp, vp, vp, vp, u32, vp, C.c_char_p, C.c_size_t]

    def config(self, length, c=0, planes=0):
        out = np.zeros(CFG_WORDS, dtype=np.uint32)
        assert self.L.g16_test_sort_config(length, c, planes, out.ctypes.data) == 0
        return Config(out)

    def init(self, capacity, c, planes, nproof_cap):
        """-> (status, message)"""
        msg = C.create_string_buffer(256)
        st = self.L.g16_test_sort_init(capacity, c, planes, nproof_cap, msg, len(msg))
        return st, msg.value.decode()

    def run(self, proofs, mont, c, planes, stride=0, rank=0, world=1, lanes=0, lanes2=0, keep=None, cap=0,
            nproof_cap=0, refusal=False):
        """proofs: a list of (n1, 8) canonical word arrays (converted here when mont).  keep: bool per point or None.
        Returns the arrays the hook copies back; with refusal=True, (status, message) instead"""
        nproof, n1 = len(proofs), proofs[0].shape[0]
        assert all(p.shape == (n1, 8) for p in proofs)
        stride = stride if nproof > 1 else 0
        assert nproof == 1 or stride >= n1
        buf = np.full(((nproof - 1) * stride + n1, 8), 0xa5a5a5a5, dtype=np.uint32)      # the gaps: never read
        for z, p in enumerate(proofs):
            buf[z * stride:z * stride + n1] = to_mont_words(p) if mont else p
        cfg = self.config(cap or n1, c, planes)
        nbt = nproof * cfg.nb
        ecap = max(nproof * n1 * cfg.W, 1)
        mcap = ecap // (MSM_MIN_SEG * MSM_SMALL_MULTI) + 2
        r = Result()
        cfgw = np.zeros(CFG_WORDS, dtype=np.uint32)
        r.count = np.full(nbt + 1, 0x5a5a5a5a, dtype=np.uint32)
        r.offset = np.full(nbt + 1, 0x5a5a5a5a, dtype=np.uint32)
        entries = np.full(ecap, 0x5a5a5a5a, dtype=np.uint32)
        part_off = np.full(PART_OFF_WORDS, 0x5a5a5a5a, dtype=np.uint32)
        r.range = np.full(6, 0x5a5a5a5a, dtype=np.uint32)
        ml, ml2 = np.zeros(mcap, dtype=np.uint32), np.zeros(mcap, dtype=np.uint32)
        meta = np.zeros(2, dtype=np.uint32)
        kb = None
        if keep is not None:
            keep = np.asarray(keep, dtype=bool)
            assert keep.size == n1
            bits = np.zeros(-(-max(n1, 1) // 32) * 32, dtype=np.uint8)
            bits[:n1] = keep
            kb = np.packbits(bits, bitorder="little").view(np.uint32).copy()
        msg = C.create_string_buffer(256)
        st = self.L.g16_test_sort_run(
            buf.ctypes.data, n1, int(mont), c, planes, nproof, stride, rank, world, lanes, lanes2,
            kb.ctypes.data if kb is not None else None, cap, nproof_cap, cfgw.ctypes.data, r.count.ctypes.data,
            r.offset.ctypes.data, entries.ctypes.data, ecap, part_off.ctypes.data, r.range.ctypes.data,
            ml.ctypes.data, ml2.ctypes.data, mcap, meta.ctypes.data, msg, len(msg))
        if refusal:
            return st, msg.value.decode()
        assert st == 0, f"g16_test_sort_run returned {st}: {msg.value.decode()}"
        r.cfg = Config(cfgw)
        assert r.cfg.nb == cfg.nb and r.cfg.c == cfg.c and r.cfg.D == cfg.D
        r.bins1 = ((nbt - 1) >> part_shift(nbt)) + 1
        r.part_off = part_off[:r.bins1 + 1]
        r.M = int(r.offset[nbt])
        r.entries = entries[:r.M]
        r.multi_l, r.multi_l2 = ml[:meta[0]], ml2[:meta[1]]
        return r


def check_sorted(r, ex):
    """count, offset and every bucket's entry set against the model"""
    assert r.count.size == ex.nbt + 1
    bad = np.nonzero(r.count[:ex.nbt] != ex.count)[0]
    assert bad.size == 0, (f"{bad.size} bucket counts differ; first: bucket {bad[0]}, model {ex.count[bad[0]]}, "
                           f"sort {r.count[bad[0]]}; totals model {ex.M}, sort {int(r.count[:ex.nbt].sum())}")
    assert r.M == ex.M
    assert np.array_equal(r.offset.astype(np.uint64), ex.offset)
    bucket = np.repeat(np.arange(ex.nbt, dtype=np.uint64), ex.count)
    got = np.sort((bucket << np.uint64(32)) | r.entries.astype(np.uint64))
    got = (got & np.uint64(0xffffffff)).astype(np.uint32)
    bad = np.nonzero(got != ex.sorted_entries)[0]
    assert bad.size == 0, (f"{bad.size} entries differ; first in bucket {int(bucket[bad[0]])}: model "
                           f"{ex.sorted_entries[bad[0]]:#x}, sort {got[bad[0]]:#x}")


def check_hot(r, ex):
    """the hot-bucket lists as sets (and without repeats), for both segmentations"""
    for lst, lanes in ((r.multi_l, r.cfg.lanes), (r.multi_l2, r.cfg.lanes2)):
        assert len(set(lst.tolist())) == lst.size
        assert set(lst.tolist()) == ex.hot(lanes)


def load_hooks(request):
    """the module fixture's body: "emu" = the hooks inside the emulator library, "gpu" = the hipcc build, which
    build() leaves next to the source -- missing there is a failure, never a skip or a compile"""
    if request.param == "emu":
        return Hooks(request.getfixturevalue("emu").L)
    import pytest
    if not os.path.exists(GPU_HOOKS):
        pytest.fail(f"{GPU_HOOKS} is not built (make -C circom_compat_amd/csrc)")
    return Hooks(C.CDLL(GPU_HOOKS))
