"""The MSM stages behind the sort -- k_bucket_accumulate with k_acc_fixup, k_combine_large, k_bucket_reduce, the two
k_set_sum levels and k_horner (csrc/msm_curve.inc.h) -- one at a time through the hooks of
tests/arith/msm_stage_hooks.hip, on the emulator build and on the gfx950 build, against the exact model of
tests/msm_stage_model.py.

Reduction tests feed SYNTHETIC partial sums: every slot of the workspace is coded as a known multiple of the
generator in projective form (or infinity, or the poison point no sum may contain), over the layout of a real sort.
contrib, wsum and the outputs are compared with the model element by element (contrib arrays of more than 3000
elements: one random linear combination, then element by element to name the chunk).  Accumulation tests feed real
points k_i G and compare every written partial slot, and the SET of written slots, with the model.

Nothing has a tolerance.  A failure names the stage, the workspace slot and the chunk (set, lo, occupancy) or the
partial slot (bucket, lane).

Emulator leg only: cases that launch more than EMU_MAX_BUCKETS = 2^18 buckets x workspace slots are skipped there by
that rule -- the ids in EMU_SKIPPED, asserted below -- because the emulator steps through every thread of the sort's
scans and of the reduction.  The GPU leg skips nothing.

red_chunk reached (asserted per case): 1 rc1-*, known-weights rc1-c17; 2 rc2-*, the slot-layout cases, shard-c17-*;
3 rc3-*, the chunk of proofs, known-weights rc3-c16; 4 rc4-d8 (dense and known weights), shard-c19-w2; 6 rc6-c18;
8 rc8-c20; 12 rc12-c18-d2; 16 rc16-c20 and rc16-capped.  The emulator leg reaches 1, 2, 3 and 4, the GPU leg all.

Time of the reference side alone -- sort model, codes, expected scalars, cpu_ref products; the test's run time minus
the time inside the hook calls -- in seconds on the CPU of the machine the module was written on (these are CPU
numbers; no GPU time is claimed): dense reductions 0.2 - 0.9 (largest: rc1-c13-g2 0.92, rc3-c16-g2 0.82, rc3-c15-z4
0.74), sharded 0.4 - 0.5 for all ranks together, known weights and slot layout 0.1, chunk of proofs 0.1 - 0.2, every
accumulation case below 0.2, the chain 0.13.  The six cases the emulator leg skips were timed the same way on the
CPU of the GPU machine: 0.08 - 0.31 (shard-c19-w2, two ranks).  No case is near the 5 s the issue allows, so no contrib
comparison had to be thinned further than the linear-combination rule above.  The emulator leg as a whole takes
145 - 170 s on that CPU, nearly all of it inside the emulator (the hook calls): 4 - 16 s per dense or sharded case."""
import numpy as np
import pytest

import msm_stage_model as M
import sort_model as SM

R = M.R
G1, G2 = M.G1, M.G2
EMU_MAX_BUCKETS = 1 << 18
EMU_SKIPPED = {"rc6-c18", "rc12-c18-d2", "rc8-c20", "rc16-c20", "rc16-capped", "shard-c19-w2"}


@pytest.fixture(scope="module", params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def hooks(request):
    h = M.load_hooks(request)
    h.leg = request.param
    return h


def emu_size_rule(hooks, case_id, buckets):
    """the one skip rule of this module (docstring): the list and the rule must agree"""
    assert (buckets > EMU_MAX_BUCKETS) == (case_id in EMU_SKIPPED), (case_id, buckets)
    if hooks.leg == "emu" and buckets > EMU_MAX_BUCKETS:
        pytest.skip(f"{buckets} buckets x workspace slots: emulator size rule (module docstring)")


# ---- pools: computed once, never changed ----------------------------------------------------------------------------
POOL_HALF = 24
LAMBDAS_G1 = [1, 5, 0x1234567890abcdef1234567890abcdef, M.o.Q_MOD - 2]
LAMBDAS_G2 = [(1, 0), (3, 7), (0, 0x1234567890abcdef), (M.o.Q_MOD - 5, 11)]


def make_pool(curve):
    rng = np.random.default_rng(8000 + curve.size)
    ks = rng.integers(1 << 18, 1 << 20, size=POOL_HALF)
    assert len(set(ks.tolist())) == POOL_HALF
    poison = (1 << 20) + 12345
    pool = M.Pool(curve, np.concatenate([ks, -ks, [poison]]), LAMBDAS_G1 if curve is G1 else LAMBDAS_G2)
    pool.points.setflags(write=False)
    return pool


@pytest.fixture(scope="module")
def pools():
    return {G1: make_pool(G1), G2: make_pool(G2)}


# ---- coders: which point sits in which partial slot -----------------------------------------------------------------
def bucket_slot_index(first, n):
    """for every owned slot, in bucket order: (slot, bucket, position inside the bucket)"""
    g = np.repeat(np.arange(n.size), n)
    start = np.cumsum(n) - n
    j = np.arange(int(n.sum())) - np.repeat(start, n)
    return np.repeat(first, n) + j, g, j


def dense_coder(pool, seed):
    """random points and lambdas in every owned slot; among the buckets with several partials a quarter hold the SAME
    point twice (a doubling inside add), a quarter P and -P (a cancellation), and one slot in sixteen is infinite;
    every slot no bucket owns holds the poison point"""
    def coder(first, n, geo, cfg, nbatch):
        rng = np.random.default_rng(seed)
        codes = np.full((nbatch, geo.slots), M.CODE_POISON, dtype=np.int32)
        slot, g, j = bucket_slot_index(first, n)
        for k in range(nbatch):
            pt = rng.integers(0, 2 * POOL_HALF, size=slot.size)
            lam = rng.integers(0, pool.nlam, size=slot.size)
            kind = rng.integers(0, 4, size=n.size)[g]          # per bucket
            second = (j == 1) & (n[g] <= M.MSM_SMALL_MULTI)
            prev = np.roll(pt, 1)
            pt = np.where(second & (kind == 0), prev, pt)                              # P, P
            pt = np.where(second & (kind == 1), (prev + POOL_HALF) % (2 * POOL_HALF), pt)   # P, -P
            c = pool.code(pt, lam).astype(np.int32)
            c[rng.integers(0, 16, size=slot.size) == 0] = M.CODE_INF
            codes[k, slot] = c
        return codes
    return coder


def canonical_coder(pool):
    """K_b depends on the bucket alone, whatever the layout: first slot a point chosen by the bucket id, a second and
    third slot Q and -Q, everything else of the bucket infinite.  (Sharded ranks cut the same buckets into different
    slots; their sums must still add up.)"""
    def coder(first, n, geo, cfg, nbatch):
        codes = np.full((nbatch, geo.slots), M.CODE_POISON, dtype=np.int32)
        slot, g, j = bucket_slot_index(first, n)
        for k in range(nbatch):
            h = (g * 2654435761 + k * 97) >> 7
            pt = np.where(j == 0, h % (2 * POOL_HALF), (h >> 8) % POOL_HALF + np.where(j == 2, POOL_HALF, 0))
            c = pool.code(pt, (h >> 3) % pool.nlam).astype(np.int32)
            c[(j > 2) | ((j == 1) & (n[g] == 2))] = M.CODE_INF
            codes[k, slot] = c
        return codes
    return coder


def canonical_K(pool, nbt, count, k):
    g = np.arange(nbt)
    h = (g * 2654435761 + k * 97) >> 7
    return np.where(count > 0, pool.k[h % (2 * POOL_HALF)], 0)


# ---- one reduction against the model --------------------------------------------------------------------------------
def run_reduce(hooks, curve, pool, proofs, c, planes, nbatch, hidden, coder, world=1, rank=0, lanes=0, lanes2=0,
               out_stride=0, stride=0, want_rc=None, dense=True):
    n1, nproof = proofs[0].shape[0], len(proofs)
    cfg = hooks.config(n1, c, planes)
    nbt = nproof * cfg.nb
    ex = SM.Expected(*SM.chunk_pairs(proofs, cfg), nbt)                # the layout the codes are written for
    rngw = None
    if world > 1:
        rngw = SM.shard_range(SM.part_offsets(ex.count, cfg.sh), rank, world, cfg.sh, cfg.nb)
        ex = ex.restricted(rngw[4], rngw[5])
    lane_count = (lanes2 or cfg.lanes2) if curve is G2 else (lanes or cfg.lanes)
    geo = M.Geometry(cfg, nproof, nbatch, world, hidden, ex.M, lane_count)
    if want_rc is not None:
        assert geo.red_chunk == want_rc, (geo.red_chunk, want_rc)
    first, n = M.slot_layout(ex.offset, geo.S)
    own = M.owned_slots(first, n, geo.slots)
    codes = coder(first, n, geo, cfg, nbatch)
    assert (codes[:, ~own] == M.CODE_POISON).all()
    r = hooks.reduce(curve, proofs, True, c, planes, pool, codes, nbatch=nbatch, hidden=hidden, out_stride=out_stride,
                     stride=stride, rank=rank, world=world, lanes=lanes, lanes2=lanes2)
    assert r.geo[:8] == geo.words(), (r.geo, geo.words())              # red_chunk, cps, nchunks, nblk, sets, S, ...
    assert r.geo[10] == ex.M and np.array_equal(r.offset.astype(np.uint64), ex.offset)
    assert set(r.hot.tolist()) == set(np.nonzero(n > M.MSM_SMALL_MULTI)[0].tolist()) and len(set(r.hot.tolist())) == r.hot.size
    if world > 1:
        assert r.range.tolist() == rngw
    if dense:
        lo, hi = (rngw[4], rngw[5]) if world > 1 else (0, nbt)
        share = float((np.diff(r.offset.astype(np.int64))[lo:hi] > 0).mean())
        assert share >= 0.75, share
    who = f"{curve.name} c={c} nbatch={nbatch} nproof={nproof} world={world} rank={rank}"

    # contrib: the chunks written, and what each holds
    written = M.written_chunks(geo, rngw)
    K = [M.bucket_sums(pool, codes[k], first, n) for k in range(nbatch)]
    contrib = [M.chunk_contribs(K[k], cfg, geo, nproof) for k in range(nbatch)]
    assert not (r.contrib_flag == 2).any() and not (r.wsum_flag == 2).any() and not (r.sums_flag == 2).any()
    want_poison = np.ones(nbatch * r.ncontrib, dtype=bool)
    want_poison[:nbatch * geo.nchunks] = np.tile(~written, nbatch)
    bad = np.nonzero((r.contrib_flag == 1) != want_poison)[0]
    if bad.size:
        k, q = divmod(int(bad[0]), geo.nchunks)
        where = M.describe_chunk(q, cfg, geo, first, n) if k < nbatch else "behind the last chunk"
        pytest.fail(f"k_bucket_reduce [{who}]: workspace slot {k}: contrib element {int(bad[0])} "
                    f"{'was not written' if r.contrib_flag[bad[0]] == 1 else 'was written'}; {where}")
    want_k = np.concatenate([c_.reshape(-1) for c_ in contrib])
    bad = M.first_mismatch(curve, r.contrib[:nbatch * geo.nchunks], want_k, live=np.tile(written, nbatch))
    if bad is not None:
        k, q = divmod(bad, geo.nchunks)
        pytest.fail(f"k_bucket_reduce [{who}]: workspace slot {k}: wrong contribution of "
                    f"{M.describe_chunk(q, cfg, geo, first, n)}")

    # wsum: one per set, the spare set of every workspace slot untouched
    wsum = [M.set_sums(contrib[k], written, geo) for k in range(nbatch)]
    flags = r.wsum_flag.reshape(nbatch, r.wsets)
    assert not flags[:, :geo.sets].any() and (flags[:, geo.sets] == 1).all(), f"k_set_sum [{who}]: {flags.tolist()}"
    dev = r.wsum.reshape(nbatch, r.wsets, curve.size)
    for k in range(nbatch):
        bad = M.first_mismatch(curve, dev[k, :geo.sets], wsum[k])
        assert bad is None, f"k_set_sum [{who}]: workspace slot {k}: wrong sum of set {bad}"

    # outputs: proof-major records, nothing written between them
    out = [M.outputs(wsum[k], cfg, nproof) for k in range(nbatch)]
    assert not r.sums_flag.any(), f"k_horner [{who}]: unwritten output {r.sums_flag.tolist()}"
    want_out = [out[k][z] for z in range(nproof) for k in range(nbatch)]
    bad = M.first_mismatch(curve, r.sums, want_out)
    assert bad is None, f"k_horner [{who}]: wrong output of proof {bad // nbatch}, workspace slot {bad % nbatch}"
    assert r.gap_dirty == 0, f"k_horner [{who}]: {r.gap_dirty} bytes between the records were written"
    r.geo_model, r.first, r.n, r.out_model, r.K, r.ex = geo, first, n, out, K, ex
    return r


def dense_proofs(hooks, rng, c, planes, nproof, fill=1.7):
    """random scalars, enough of them that at least 3/4 of the buckets are occupied (asserted from offset)"""
    cfg = hooks.config(1000, c, planes)
    n = int(fill * cfg.nb / cfg.W) + 1
    assert hooks.config(n, c, planes).D == cfg.D
    return [SM.random_words(rng, n) for _ in range(nproof)]


# id, curve, c, planes, nbatch, nproof, hidden, red_chunk, D
DENSE_CASES = [
    ("rc1-c13", G1, 13, 0, 1, 1, False, 1, 1),
    ("rc1-c13-g2", G2, 13, 4, 2, 1, True, 1, 5),
    ("rc2-c16", G1, 16, 0, 2, 1, True, 2, 1),
    ("rc2-c16-g2", G2, 16, 0, 2, 1, True, 2, 1),
    ("rc3-c16", G1, 16, 0, 3, 1, True, 3, 1),           # 32768 = 3 * 10922 + 2: the ragged last chunk holds 2 buckets
    ("rc3-c16-g2", G2, 16, 0, 3, 1, True, 3, 1),
    ("rc3-c15-z4", G1, 15, 0, 3, 4, False, 3, 1),       # 16384 = 3 * 5461 + 1, four proofs: set boundaries
    ("rc2-c18", G1, 18, 0, 1, 1, False, 2, 1),
    ("rc6-c18", G1, 18, 0, 3, 1, False, 6, 1),          # 131072 = 6 * 21845 + 2
    ("rc4-d8", G1, 16, 2, 1, 1, False, 4, 8),           # k_horner: 8 sets, 16 doublings between them
    ("rc12-c18-d2", G1, 18, 8, 3, 1, False, 12, 2),     # 131072 = 12 * 10922 + 8
    ("rc8-c20", G1, 20, 0, 1, 1, False, 8, 1),
    ("rc16-c20", G1, 20, 0, 2, 1, False, 16, 1),
    ("rc16-capped", G1, 20, 0, 3, 1, False, 16, 1),     # 24 buckets per thread asked for, MSM_RED_CHUNK caps
]


@pytest.mark.parametrize("case", DENSE_CASES, ids=[c[0] for c in DENSE_CASES])
def test_reduce_dense(hooks, pools, case):
    cid, curve, c, planes, nbatch, nproof, hidden, rc, D = case
    cfg = hooks.config(1000, c, planes)
    assert cfg.D == D
    emu_size_rule(hooks, cid, nbatch * nproof * cfg.nb)
    rng = np.random.default_rng(8100 + c * 7 + nbatch)
    proofs = dense_proofs(hooks, rng, c, planes, nproof)
    stride = proofs[0].shape[0] + 3
    r = run_reduce(hooks, curve, pools[curve], proofs, c, planes, nbatch, hidden, dense_coder(pools[curve], 8200 + c),
                   stride=stride, out_stride=(nbatch + 1) * 4 * 9 * 4 * (2 if curve is G2 else 1) + 8, want_rc=rc)
    geo = r.geo_model
    if cfg.B % rc:
        assert geo.cps * rc > cfg.B                                  # a ragged last chunk in every set
    multi = r.n[(r.n > 1)]
    assert multi.size > 20                                           # buckets with several partials: P,P and P,-P pairs
    # chunks that hold several occupied buckets: what no small whole-MSM test reaches
    if rc > 1:
        occ = np.zeros(geo.sets * geo.cps * rc, dtype=bool).reshape(geo.sets, -1)
        occ[:, :cfg.B] = (r.n > 0).reshape(geo.sets, cfg.B)
        assert (occ.reshape(geo.sets, geo.cps, rc).sum(axis=2) >= 2).mean() > 0.5


# ---- known weights ------------------------------------------------------------------------------------------------
def one_digit_words(values):
    return SM.to_words(values)


# c, nbatch, hidden, red_chunk, chunk offsets lo (multiples of red_chunk)
KNOWN_WEIGHTS = [
    # red_chunk 1: lo is the bucket.  Radix-4 digits of lo, least significant first: 0x1b = 3,2,1,0; 0xe4 = 0,1,2,3;
    # 0xffff = eight 3s, a carry out of the top digit into the spare one; 0xc000: top digit 3; 0x3fff: seven 3s
    ("rc1-c17", 17, 1, False, 1, [0, 1, 2, 3, 0x1b, 0xe4, 0x5555, 0xaaaa, 0x3fff, 0xc000, 0xfffe, 0xffff]),
    # red_chunk 3: 3 = digit 3; 15 = 3,3; 21 = 1,1,1; 0x3fff = seven 3s; 32766: the ragged last chunk (2 buckets)
    ("rc3-c16", 16, 3, True, 3, [0, 3, 6, 15, 21, 0x3fff, 0x6666 // 3 * 3, 32766 - 3, 32766]),
    # red_chunk 4 and 8 sets: every lo ends in digit 0; 12 = 0,3; 0x3ffc; 32764: the last chunk
    ("rc4-d8", 16, 1, False, 4, [0, 4, 8, 12, 0x1b0, 0x3ffc, 0x7000, 32764]),
]


@pytest.mark.parametrize("case", KNOWN_WEIGHTS, ids=[c[0] for c in KNOWN_WEIGHTS])
def test_reduce_known_weights(hooks, pools, case):
    """One finite bucket per chunk -- at the first, a middle and the last position of the chunk, one position per
    workspace slot (or per bucket set) -- so that contrib[q] = (lo + position + 1) P exactly: the running sums and the
    radix-4 lo * run ladder against known weights.  One more chunk holds P and -P (its run stays infinite), every
    other chunk is empty."""
    cid, c, nbatch, hidden, rc, los = case
    planes = 2 if cid == "rc4-d8" else 0
    pool = pools[G1]
    cfg = hooks.config(1000, c, planes)
    assert all(lo % rc == 0 and lo < cfg.B for lo in los)
    cancel_lo = (0x2222 // rc) * rc
    assert cancel_lo not in los
    # occupancy: every bucket of every chosen chunk once, in every set; the cancelling bucket 9 times (> one segment of
    # MSM_MIN_SEG entries: at least two partials)
    vals = [sum((b + 1) << (c * d) for d in range(cfg.D)) for lo in los for b in range(lo, min(lo + rc, cfg.B))]
    vals += [sum((cancel_lo + 1) << (c * d) for d in range(cfg.D))] * 9
    words = one_digit_words(vals)
    npos = max(nbatch, cfg.D)
    positions = [0, rc // 2, rc - 1, rc // 3, 0, rc - 1, rc // 2, 0][:npos]

    def coder(first, n, geo, cfg_, nb_):
        codes = np.full((nb_, geo.slots), M.CODE_POISON, dtype=np.int32)
        slot, g, j = bucket_slot_index(first, n)
        codes[:, slot] = M.CODE_INF
        for k in range(nb_):
            for st in range(cfg_.D):
                pos = positions[max(k, st)]
                for i, lo in enumerate(los):
                    b = min(lo + pos, cfg_.B - 1)
                    assert n[st * cfg_.B + b] == 1
                    codes[k, first[st * cfg_.B + b]] = pool.code((i + 5 * k + st) % (2 * POOL_HALF), 1 + (i + st) % 3)
                gc = st * cfg_.B + cancel_lo
                assert n[gc] >= 2
                codes[k, first[gc]] = pool.code(3, 1)
                codes[k, first[gc] + 1] = pool.code(3 + POOL_HALF, 2)
        return codes

    r = run_reduce(hooks, G1, pool, [words], c, planes, nbatch, hidden, coder, want_rc=rc, dense=False)
    geo = r.geo_model
    assert cfg.D == (8 if planes else 1)
    # the model's contributions ARE the known weights
    for k in range(nbatch):
        for st in range(cfg.D):
            pos = positions[max(k, st)]
            got = M.chunk_contribs(r.K[k], cfg, geo, 1)[st]
            for i, lo in enumerate(los):
                b = min(lo + pos, cfg.B - 1)
                assert got[lo // rc] == (b + 1) * int(pool.k[(i + 5 * k + st) % (2 * POOL_HALF)])
            assert got[cancel_lo // rc] == 0
    top = (geo.cps - 1) * rc
    assert max(los) >= top - rc                                       # the largest offsets of the grid are among them


# ---- slot layout --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", [G1, G2], ids=["g1", "g2"])
@pytest.mark.parametrize("lanes", [128, 64 * 128], ids=["lanes128", "lanes8192"])
def test_reduce_slot_layout(hooks, pools, curve, lanes):
    """buckets with 1, 2, 3, exactly MSM_SMALL_MULTI and MSM_SMALL_MULTI + 1 partials at 128 lanes (segments of 10);
    at 8192 lanes the same entries leave most lanes dead and make both long buckets hot.  red_chunk = 2: the hot bucket
    shares its chunk with a neighbour."""
    S, k = 10, 312
    sizes = [10, k, 7, k, 9, 12, 25]                                  # buckets 0 .. 6
    vals = [b + 1 for b, sz in enumerate(sizes) for _ in range(sz)]
    singles = list(range(32700, 32769)) + list(range(5000, 5100)) + list(range(8, 500))
    singles = singles[:1250 - len(vals)]
    vals += singles
    assert len(vals) == 1250 and max(vals) == 32768
    rng = np.random.default_rng(8301)
    words = SM.to_words(vals)[rng.permutation(len(vals))]
    r = run_reduce(hooks, curve, pools[curve], [words], 16, 0, 2, True, dense_coder(pools[curve], 8302), lanes=lanes,
                   lanes2=lanes, want_rc=2, dense=False)
    n = r.n
    if lanes == 128:
        assert r.geo_model.S == S
        assert n[:7].tolist() == [1, M.MSM_SMALL_MULTI, 1, M.MSM_SMALL_MULTI + 1, 1, 2, 3]
        assert r.hot.tolist() == [3]
    else:
        assert r.geo_model.S == M.MSM_MIN_SEG and -(-r.ex.M // r.geo_model.S) < lanes // 40   # most lanes are dead
        assert sorted(r.hot.tolist()) == [1, 3]


# ---- chunk sorts and batches ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", [G1, G2], ids=["g1", "g2"])
def test_reduce_chunk_of_proofs(hooks, pools, curve):
    """nproof = 3, nbatch = 2, D = 2, records 3 accumulators apart: every (proof, slot) sum and the gaps"""
    c, planes = 14, 10
    rng = np.random.default_rng(8401)
    proofs = dense_proofs(hooks, rng, c, planes, 3)
    acc_bytes = 4 * 9 * 4 * (2 if curve is G2 else 1)
    r = run_reduce(hooks, curve, pools[curve], proofs, c, planes, 2, True, dense_coder(pools[curve], 8402),
                   stride=proofs[0].shape[0] + 11, out_stride=3 * acc_bytes + 4, want_rc=3)
    assert r.cfg.D == 2 and r.geo_model.sets == 6 and len({v for out in r.out_model for v in out}) == 6


# ---- sharding -----------------------------------------------------------------------------------------------------
# id, c, nbatch, hidden, world, red_chunk
SHARD_CASES = [("shard-c17-w2", 17, 3, True, 2, 2), ("shard-c17-w3", 17, 3, True, 3, 2),
               ("shard-c19-w2", 19, 3, False, 2, 4)]


@pytest.mark.parametrize("case", SHARD_CASES, ids=[c[0] for c in SHARD_CASES])
def test_reduce_sharded(hooks, pools, case):
    """every rank of a bucket-sharded reduction: red_chunk rounded down to a power of two (3 -> 2; 6 -> 4) and within one
    sort partition, only the chunks of the rank's run written, and the ranks' outputs add up to the unsharded result"""
    cid, c, nbatch, hidden, world, rc = case
    pool = pools[G1]
    cfg = hooks.config(1000, c, 0)
    emu_size_rule(hooks, cid, nbatch * cfg.nb)
    rng = np.random.default_rng(8500 + c)
    proofs = dense_proofs(hooks, rng, c, 0, 1)
    assert rc <= 1 << SM.part_shift(cfg.nb) and rc & (rc - 1) == 0
    assert M.red_chunk(cfg, nbatch, 1, hidden) not in (rc, 1)          # the unsharded chunk is another
    total = [0] * nbatch
    runs = []
    for rank in range(world):
        r = run_reduce(hooks, G1, pool, proofs, c, 0, nbatch, hidden, canonical_coder(pool), world=world, rank=rank,
                       want_rc=rc)
        runs.append(r.range.tolist())
        written = M.written_chunks(r.geo_model, r.range)
        assert 0 < written.sum() < r.geo_model.nchunks
        for k in range(nbatch):
            total[k] = (total[k] + r.out_model[k][0]) % R
    assert runs[0][4] == 0 and runs[-1][5] == cfg.nb and all(a[5] == b[4] for a, b in zip(runs, runs[1:]))
    full = SM.Expected(*SM.pairs(proofs[0], cfg), cfg.nb)
    for k in range(nbatch):
        K = canonical_K(pool, cfg.nb, full.count, k)
        want = sum(int(v) * (b + 1) for b, v in enumerate(K.tolist())) % R
        assert total[k] == want, f"workspace slot {k}: the ranks' sums do not add up to the unsharded sum"


# ---- accumulation ---------------------------------------------------------------------------------------------------
NPTS = 1400


@pytest.fixture(scope="module")
def points():
    """k_i G for both curves, computed once: (multipliers, G1 bytes, G2 bytes)"""
    rng = np.random.default_rng(8600)
    ks = [int.from_bytes(rng.bytes(31), "little") % R or 1 for _ in range(NPTS)]
    p1, p2 = G1.points(ks), G2.points(ks)
    p1.setflags(write=False)
    p2.setflags(write=False)
    return ks, p1, p2


class Query:
    """a query of points picked from the module's table: sel[i] = table index (negative: minus that point, None:
    infinity)"""

    def __init__(self, points, curve, sel):
        ks, p1, p2 = points
        tab = p1 if curve is G1 else p2
        self.ks = [None if s is None else (ks[abs(s)] if s >= 0 else R - ks[-s]) for s in sel]
        self.pts = np.zeros((len(sel), curve.size), dtype=np.uint8)
        neg = [i for i, s in enumerate(sel) if s is not None and s < 0]
        for i, s in enumerate(sel):
            if s is not None and s >= 0:
                self.pts[i] = tab[s]
        if neg:
            self.pts[neg] = curve.points([self.ks[i] for i in neg])


MODES = {"single": 0, "first-half": 1, "second-half": 2, "pair": 3}


def run_accumulate(hooks, curve, words, qa, qb, c, planes, mode, idx_min=0, lanes=0, lanes2=0, want_overflow=False):
    """one accumulation against the model: the set of written slots and every partial"""
    single = MODES[mode] == 0
    r = hooks.accumulate(curve, words, True, c, planes, qa.pts, None if single else qb.pts, idx_min=idx_min,
                         mode=MODES[mode], lanes=lanes, lanes2=lanes2)
    cfg = r.cfg
    ex = SM.Expected(*SM.pairs(words, cfg), cfg.nb)
    assert r.M == ex.M and np.array_equal(r.offset.astype(np.uint64), ex.offset)
    bucket = np.repeat(np.arange(cfg.nb, dtype=np.uint64), ex.count)
    got = np.sort((bucket << np.uint64(32)) | r.entries.astype(np.uint64))
    assert np.array_equal((got & np.uint64(0xffffffff)).astype(np.uint32), ex.sorted_entries)
    assert r.S == M.seg_len(r.M, r.lanes)
    halves = {"single": [qa], "first-half": [qa], "second-half": [qb], "pair": [qa, qb]}[mode]
    who = f"k_bucket_accumulate [{curve.name} {mode} c={c} lanes={r.lanes} S={r.S} idx_min={idx_min}]"
    lane_of = dict(zip((bucket.astype(np.int64) + np.arange(r.M) // r.S).tolist(),
                       zip(bucket.tolist(), (np.arange(r.M) // r.S).tolist())))
    for h, q in enumerate(halves):
        want = M.accumulate_expected(r.offset, r.entries, r.S, cfg, q.ks, idx_min)
        assert not (r.flag[h] == 2).any()
        wrote = set(np.nonzero(r.flag[h] == 0)[0].tolist())
        extra, missing = sorted(wrote - set(want)), sorted(set(want) - wrote)
        assert not extra, f"{who} half {h}: slot {extra[0]} was written and belongs to no (bucket, lane) pair"
        assert not missing, f"{who} half {h}: slot {missing[0]} = (bucket, lane) {lane_of[missing[0]]} was not written"
        slots = sorted(want)
        bad = M.first_mismatch(curve, r.partial[h][slots], [want[s] for s in slots])
        assert bad is None, f"{who} half {h}: wrong partial in slot {slots[bad]} = (bucket, lane) {lane_of[slots[bad]]}"
        r.want = want
    assert r.overflow[0] == int(want_overflow) and r.overflow[1] == 0, r.overflow
    return r


def mixed_input(points, curve, n, c, seed):
    """random scalars with the special cases of the issue: infinity points (one alone in its bucket, several in the hot
    bucket of the ones), repeated points under equal one-digit scalars (two and three in a row: on G1 fix-list items,
    two of them on one slot; on G2 the exact doubling), P, -P and Q under one scalar, scalar 0, r - 1"""
    rng = np.random.default_rng(seed)
    words = SM.random_words(rng, n)
    sel_a = [int(v) for v in rng.permutation(NPTS - 1)[:n] + 1]
    sel_b = [int(v) for v in rng.permutation(NPTS - 1)[:n] + 1]
    half = 1 << (c - 1)

    def put(i, value, a, b=None):
        words[i] = SM.to_words([value])[0]
        sel_a[i], sel_b[i] = a, (a if b is None else b)

    i = 8
    for v in (half - 1, half - 2):                                    # P, P under one digit: a doubling
        put(i, v, 700), put(i + 1, v, 700)
        i += 2
    for t in range(3):                                                # P, P, P: two fix-list items on one slot
        put(i + t, half - 3, 701, 702)
    i += 3
    for t, s in enumerate((703, -703, 704)):                          # P, -P, Q in some order
        put(i + t, half - 4, s)
    i += 3
    put(i, half - 5, None)                                            # infinity alone in its bucket
    i += 1
    for t in range(24):                                               # the ones: a bucket of many entries, a third infinite
        put(i + t, 1, None if t % 3 == 0 else 710 + t)
    i += 24
    put(i, 0, 705), put(i + 1, R - 1, 706), put(i + 2, half, 707), put(i + 3, half + 1, 708)
    assert i + 4 <= n
    return words, Query(points, curve, sel_a), Query(points, curve, sel_b)


ACC_CASES = [  # id, curve, mode, n, c, planes, lanes (0: the build's default), idx_min
    ("g1-single-default", G1, "single", 150, 13, 0, 0, 0),
    ("g1-single-128", G1, "single", 150, 13, 0, 128, 0),
    ("g1-single-idxmin", G1, "single", 150, 13, 0, 128, 5),
    ("g1-single-d4", G1, "single", 150, 12, 6, 256, 0),          # D = 4: planes step 2^48
    ("g1-second-half-default", G1, "second-half", 150, 13, 0, 0, 0),
    ("g1-second-half-idxmin", G1, "second-half", 150, 13, 0, 128, 3),
    ("g1-first-half-128", G1, "first-half", 150, 13, 0, 128, 0),
    ("g1-pair-default", G1, "pair", 150, 13, 0, 0, 0),
    ("g1-pair-128", G1, "pair", 150, 13, 0, 128, 0),             # the smallest pair grid: two workgroups
    ("g2-single-default", G2, "single", 80, 13, 0, 0, 0),
    ("g2-single-128", G2, "single", 80, 13, 0, 128, 0),
    ("g2-second-half-128", G2, "second-half", 80, 13, 0, 128, 0),  # the product has no G2 pair launch
]


@pytest.mark.parametrize("case", ACC_CASES, ids=[c[0] for c in ACC_CASES])
def test_accumulate(hooks, points, case):
    cid, curve, mode, n, c, planes, lanes, idx_min = case
    words, qa, qb = mixed_input(points, curve, n, c, 8700 + n + c)
    if idx_min:                                                       # the query starts at scalar idx_min
        qa.pts, qa.ks, qb.pts, qb.ks = qa.pts[idx_min:], qa.ks[idx_min:], qb.pts[idx_min:], qb.ks[idx_min:]
    r = run_accumulate(hooks, curve, words, qa, qb, c, planes, mode, idx_min=idx_min, lanes=lanes, lanes2=lanes)
    cfg = r.cfg
    planes_seen = set(((r.entries & np.uint32(0x7fffffff)) >> np.uint32(cfg.idx_bits)).tolist())
    assert len(planes_seen) == cfg.Pn > 1 and (r.entries >> np.uint32(31)).any()    # planes above 0, negated digits
    live = -(-r.M // r.S)
    if lanes == 0:
        assert r.S == M.MSM_MIN_SEG and live < r.lanes                # short segments, dead lanes behind the last
    else:
        assert live > r.lanes // 2                                    # most lanes live, each crossing many buckets
        first, nn = M.slot_layout(r.offset, r.S)
        assert (np.diff(r.offset.astype(np.int64)) == 0).any() and nn.max() >= 2   # runs of empty buckets; split buckets
    assert 0 in r.want.values()                                       # a written slot that holds the point at infinity


# (bucket sizes, lanes): S = 8 with M = 128 x 8: every segment ends on a bucket boundary and the last lane is full;
# S = 9, M = 9 x 114 + 1: the last live lane holds one entry; S = 9, M = 9 x 120 in buckets of 9, 18 and 27
BOUNDARY_CASES = [("m-multiple-of-s", [8] * 128, 8, 128), ("m-sk-plus-1", [9] * 114 + [1], 9, 115),
                  ("buckets-of-segments", [9, 18, 27, 9, 9, 18] * 12, 9, 120)]


@pytest.mark.parametrize("mode", ["single", "pair"])
@pytest.mark.parametrize("case", BOUNDARY_CASES, ids=[c[0] for c in BOUNDARY_CASES])
def test_accumulate_boundaries(hooks, points, case, mode):
    cid, sizes, S, live = case
    vals = [3 * b + 1 for b, sz in enumerate(sizes) for _ in range(sz)]          # two empty buckets between neighbours
    n = len(vals)
    rng = np.random.default_rng(8800 + n)
    words = SM.to_words(vals)[rng.permutation(n)]
    qa = Query(points, G1, [int(v) for v in rng.permutation(NPTS - 1)[:n] + 1])
    qb = Query(points, G1, [int(v) for v in rng.permutation(NPTS - 1)[:n] + 1])
    r = run_accumulate(hooks, G1, words, qa, qb, 13, 2, mode, lanes=128)   # 2 planes: one-digit scalars use plane 0
    assert r.M == n and r.S == S and -(-r.M // r.S) == live
    off = r.offset.astype(np.int64)
    assert (off[off < n] % S == 0).sum() >= min(live, len(sizes))     # segment ends that are bucket boundaries
    assert len(r.want) == sum(-(-sz // S) for sz in sizes)


@pytest.mark.parametrize("mode", ["single", "pair"])
def test_accumulate_fix_list_overflow(hooks, points, mode):
    """MSM_FIX_CAP + 40 buckets of the build, each P, P under one digit: every one defers its second addition, the list
    overflows, k_acc_fixup says so and the exact kernel redoes the launch.  The pair launch fills the list from both
    halves (half the buckets each would do; it gets all of them twice)."""
    cap = hooks.plan(100, 13, 2)[3]
    nb = cap + 40
    assert nb <= 4096 and nb <= NPTS * 2
    vals = [b + 1 for b in range(nb) for _ in range(2)]
    rng = np.random.default_rng(8900)
    perm = rng.permutation(len(vals))
    words = SM.to_words(vals)[perm]
    sel = np.array([1 + b % (NPTS - 1) for b in range(nb) for _ in range(2)])[perm]
    qa = Query(points, G1, [int(v) for v in sel])
    qb = Query(points, G1, [int(1 + (v * 7) % (NPTS - 1)) for v in sel])
    r = run_accumulate(hooks, G1, words, qa, qb, 13, 2, mode, want_overflow=True)
    assert r.fix_cap == cap and r.S == 8 and len(r.want) == nb        # no bucket is split: every slot is 2 k G


# ---- the two halves of the model agree --------------------------------------------------------------------------------
def test_chain(hooks, points):
    """accumulate hook -> its partials (compared above with the model's slot map) -> the MODEL's reduction of that
    slot map == cpu_ref.msm_g1 of the inputs"""
    n, c = 120, 13
    words, qa, qb = mixed_input(points, G1, n, c, 9001)
    r = run_accumulate(hooks, G1, words, qa, qb, c, 0, "single", lanes=128)
    out = M.reduce_model(r.want, r.offset, r.S, r.cfg, 1)
    mont = np.frombuffer(SM.to_mont_words(words).tobytes(), dtype=np.uint64).reshape(-1, 4).copy()
    assert G1.points(out)[0].tobytes() == M.cpu_ref.msm_g1(np.ascontiguousarray(qa.pts), mont)

