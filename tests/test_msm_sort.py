"""MsmSort (csrc/msm_sort.hip) alone, through the hooks of tests/arith/sort_hooks.hip, on the emulator build and on the
gfx950 build, against the exact integer model of tests/sort_model.py: signed c-bit digits, the level-1 partition, the
level-2 placement, the scans, the hot-bucket lists, the bucket-range cut of sharded ranks and the filtered view.

Nothing has a tolerance: counts, offsets, partition offsets and ranges are compared for equality, every bucket's
entries as a sorted list (the order inside a bucket is unspecified by design), the hot-bucket lists as sets.

Emulator leg only: digit cases with more than 2^19 buckets are skipped there by the rule in EMU_MAX_BUCKETS --
(c, planes) = (24, 0) with 2^23 buckets and (17, 1) with 15 * 2^16 -- because the emulator steps through every thread
of the scans and memsets (about 7 s per 2^20 buckets).  The GPU leg skips nothing.

The product's 2048-block cap of the sort grids needs more than 4 M scalars to reach; that stays with
test_gpu_large.  The grid-stride test below puts the emulator's 32-block cap into its stride loops and, on the GPU,
fills 65 level-1 blocks with a ragged last tile and about 130 level-2 chunks."""
import numpy as np
import pytest

import sort_model as M

R = M.R_MOD
EMU_MAX_BUCKETS = 1 << 19


@pytest.fixture(scope="module", params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def hooks(request):
    h = M.load_hooks(request)
    h.leg = request.param
    return h


def run_and_check(hooks, proofs, mont, c, planes, keep=None, **kw):
    """one unsharded sort (or a view of it) against the model: count, offset, entries, both hot lists, part_off"""
    r = hooks.run(proofs, mont, c, planes, keep=keep, **kw)
    nbt = len(proofs) * r.cfg.nb
    ex = M.Expected(*M.chunk_pairs(proofs, r.cfg, keep), nbt)
    M.check_sorted(r, ex)
    M.check_hot(r, ex)
    src = ex if keep is None else M.Expected(*M.chunk_pairs(proofs, r.cfg), nbt)      # part_off: the source sort's
    assert np.array_equal(r.part_off.astype(np.uint64), M.part_offsets(src.count, M.part_shift(nbt)))
    return r, ex


# ---- digits and layouts -------------------------------------------------------------------------------------------
def special_scalars(c):
    W = -(-255 // c)
    half = 1 << (c - 1)
    every = lambda v, windows: sum(v << (c * w) for w in range(windows))
    below = max(w for w in range(W + 1) if c * w <= 253)             # windows that fit below 2^253 < r
    vals = [0, 1, R - 1, R - 2, (R - 1) // 2, half, half + 1, (1 << c) - 1, 1 << c, 1 << 253,
            every(half, W) % R, every(half + 1, W) % R,              # as the issue states them, reduced mod r
            every(half, below), every(half + 1, below)]              # unreduced: a carry chain through `below` windows
    assert all(0 <= v < R for v in vals)
    return vals


DIGIT_CASES = [(2, 0), (3, 0), (5, 0), (6, 2), (7, 0), (13, 0), (15, 0), (15, 3), (16, 0), (17, 0), (17, 1), (20, 0),
               (24, 0), (4, 1)]


@pytest.mark.parametrize("mont", [False, True], ids=["canonical", "mont"])
@pytest.mark.parametrize("c,planes", DIGIT_CASES)
def test_digits_and_layouts(hooks, c, planes, mont):
    cfg = hooks.config(517, c, planes)
    assert cfg.c == c
    if hooks.leg == "emu" and cfg.nb > EMU_MAX_BUCKETS:
        pytest.skip(f"{cfg.nb} buckets: emulator size rule (module docstring)")
    rng = np.random.default_rng(7000 + 10 * c + planes)
    sp = M.to_words(special_scalars(c))
    words = np.concatenate([sp, M.random_words(rng, 517 - len(sp))])
    words = words[rng.permutation(517)]
    r, ex = run_and_check(hooks, [words], mont, c, planes)
    # what the case list is there for
    assert r.cfg.idx_bits == (26 if r.cfg.Pn > 16 else 27)
    if (c, planes) in ((13, 0), (16, 0), (17, 0), (20, 0), (24, 0)):
        assert r.cfg.D == 1
    if (c, planes) in ((17, 1), (4, 1)):
        assert r.cfg.D == r.cfg.W
    if (c, planes) in ((6, 2), (15, 3), (2, 0), (5, 0)):
        assert 1 < r.cfg.D < r.cfg.W
    if c in (3, 5, 15, 17):
        assert c * r.cfg.W == 255
    if c == 20:
        assert r.cfg.nb + 1 > 256 * 1024                              # k_scan_top loops with a carry
    assert ex.M > 250 * r.cfg.W


# ---- exact boundary totals ----------------------------------------------------------------------------------------
BOUNDARY_N = [1, 255, 256, 257, 2039, 2047, 2048, 2049, 8191, 8192, 8193, 16383, 16384, 16385, 3 * 16384 + 247]


@pytest.fixture(scope="module")
def one_digit_scalars():
    """scalars in [1, 2^12) at c = 13: one digit each, so M = n; 4096 buckets (the LDS-histogram path)"""
    rng = np.random.default_rng(7101)
    w = np.zeros((max(BOUNDARY_N), 8), dtype=np.uint32)
    w[:, 0] = rng.integers(1, 1 << 12, size=w.shape[0])
    w.setflags(write=False)
    return w


@pytest.mark.parametrize("view", [False, True], ids=["plain", "view"])
@pytest.mark.parametrize("n", BOUNDARY_N)
def test_boundary_totals(hooks, one_digit_scalars, n, view):
    words = one_digit_scalars[:n]
    keep = (np.arange(n) % 5 != 4) if view else None                  # the view drops every fifth point
    r, ex = run_and_check(hooks, [words], False, 13, 0, keep=keep)
    assert r.cfg.nb == 4096 and r.cfg.D == 1
    assert int(r.part_off[-1]) == n                                   # M = n in the source sort
    assert ex.M == (n if not view else n - n // 5)


# ---- both level-2 paths in one run --------------------------------------------------------------------------------
def test_both_level2_paths(hooks):
    rng = np.random.default_rng(7201)
    words = M.random_words(rng, 1 << 13)
    r, ex = run_and_check(hooks, [words], False, 16, 0)
    assert r.cfg.D == 1 and r.cfg.nb == 32768
    spans = M.chunk_spans(ex, M.part_offsets(ex.count, r.cfg.sh), r.cfg.sh, M.P2_CHUNK)
    assert spans.size >= 8 and ex.M > 130000
    assert (spans <= M.P2_BINS).any(), spans                          # LDS-histogram chunks ...
    assert (spans > M.P2_BINS).any(), spans                           # ... and global-atomic chunks in ONE launch


# ---- grid-stride loops --------------------------------------------------------------------------------------------
def test_grid_stride_loops(hooks):
    """emulator: more level-1 tiles and level-2 chunks than its 32-block cap; GPU: 65 level-1 blocks with a ragged
    last tile, ~130 level-2 count chunks.  (The product's 2048-block cap: test_gpu_large.)"""
    rng = np.random.default_rng(7301)
    if hooks.leg == "emu":
        n, c = 32 * 2048 + 2048 + 5, 15
    else:
        n, c = (1 << 17) + 5, 16
    words = M.random_words(rng, n)
    r, ex = run_and_check(hooks, [words], True, c, 0)
    assert r.cfg.c == c
    if hooks.leg == "emu":
        assert -(-n // M.P1_TILE) > 32 and -(-ex.M // M.P2_CHUNK) > 32
    else:
        assert -(-n // M.P1_TILE) == 65 and n % M.P1_TILE and -(-ex.M // M.P2_CHUNK) >= 125


# ---- chunks of proofs ---------------------------------------------------------------------------------------------
def chunk_of(rng, n, nproof):
    proofs = [M.random_words(rng, n) for _ in range(nproof)]
    for a, b in zip(proofs, proofs[1:]):
        assert (a[0] != b[0]).any()                                   # scalar 0 differs from proof to proof
    return proofs


@pytest.mark.parametrize("c,planes,n,nproof,stride", [(5, 0, 300, 3, 300), (13, 0, 700, 4, 1000), (15, 2, 520, 2, 600)])
def test_chunks(hooks, c, planes, n, nproof, stride):
    proofs = chunk_of(np.random.default_rng(7400 + c), n, nproof)
    r, ex = run_and_check(hooks, proofs, True, c, planes, stride=stride)
    per = [int(ex.offset[(z + 1) * r.cfg.nb] - ex.offset[z * r.cfg.nb]) for z in range(nproof)]
    assert all(per) and len(set(per)) > 1                             # every proof has its own bucket range


def test_view_of_a_chunk(hooks):
    rng = np.random.default_rng(7450)
    proofs = chunk_of(rng, 700, 3)
    keep = rng.integers(0, 2, size=700).astype(bool)
    assert 250 < keep.sum() < 450
    r, ex = run_and_check(hooks, proofs, True, 13, 0, stride=1000, keep=keep)
    assert 0 < ex.M < int(r.part_off[-1])


# ---- hot buckets --------------------------------------------------------------------------------------------------
def ones_and_random(rng):
    words = np.concatenate([M.to_words([1] * 3000), M.random_words(rng, 200)])
    return words[rng.permutation(3200)]


# lanes = workgroups x 128 (MSM_ACC_THREADS), the unit of the G16_ACC_GRID environment the override stands in for:
# at 64 and 32 LANES the ~3170 entries of the ones' bucket would span 16 and 8 segments of the ~13 000 entries and
# neither list could hold anything.  The second pair gives the two lists different segment lengths (26 and 51).
@pytest.mark.parametrize("lanes,lanes2", [(64 * 128, 32 * 128), (512, 256)])
@pytest.mark.parametrize("view", [False, True], ids=["plain", "view"])
def test_hot_buckets(hooks, view, lanes, lanes2):
    rng = np.random.default_rng(7501)
    words = ones_and_random(rng)
    keep = (np.arange(3200) % 3 != 1) if view else None               # the view drops a third of the points
    r, ex = run_and_check(hooks, [words], True, 5, 0, keep=keep, lanes=lanes, lanes2=lanes2)
    assert (r.cfg.lanes, r.cfg.lanes2) == (lanes, lanes2)
    assert r.multi_l.size and r.multi_l2.size
    assert 0 in set(r.multi_l.tolist()) and 0 in set(r.multi_l2.tolist())     # the ones' bucket
    if lanes == 512:
        assert set(r.multi_l.tolist()) == {0} and ex.spans(lanes)[0] != ex.spans(lanes2)[0]


def test_hot_bucket_threshold(hooks):
    """two buckets of 312 entries: one starts on a segment boundary and spans exactly MSM_SMALL_MULTI segments, the
    other starts one entry before a boundary and spans one more.  Only the second is listed."""
    S, k = 10, 312
    a0, a2, tail = 10, 7, 9                                           # bucket 0, bucket 2, and the buckets behind
    vals = [1] * a0 + [2] * k + [3] * a2 + [4] * k + [5] * tail
    total = len(vals)
    lanes = 66
    assert -(-total // lanes) == S and S >= M.MSM_MIN_SEG
    rng = np.random.default_rng(7502)
    words = M.to_words(vals)[rng.permutation(total)]
    r, ex = run_and_check(hooks, [words], False, 5, 0, lanes=lanes, lanes2=33)
    assert ex.M == total
    sp = ex.spans(lanes)
    assert int(sp[1]) == M.MSM_SMALL_MULTI and int(sp[3]) == M.MSM_SMALL_MULTI + 1
    assert set(r.multi_l.tolist()) == {3}
    assert r.multi_l2.size == 0 and int(ex.spans(33).max()) <= M.MSM_SMALL_MULTI


# ---- bucket-range shards ------------------------------------------------------------------------------------------
def check_shards(hooks, words, mont, c, planes, world):
    cfg = hooks.config(words.shape[0], c, planes)
    full = M.Expected(*M.pairs(words, cfg), cfg.nb)
    part_off = M.part_offsets(full.count, cfg.sh)
    bins1 = len(part_off) - 1
    ranges, totals = [], 0
    for rank in range(world):
        r = hooks.run([words], mont, c, planes, rank=rank, world=world)
        assert np.array_equal(r.part_off.astype(np.uint64), part_off)
        want = M.shard_range(part_off, rank, world, cfg.sh, cfg.nb)
        assert r.range.tolist() == want, (rank, r.range.tolist(), want)
        for g in (rank, rank + 1):                                    # the bisection against the plain definition
            if 0 < g < world:
                assert M.pick_cut(part_off, g, world) in M.closest_cut(part_off, g, world)
        ex = full.restricted(want[4], want[5])
        assert ex.M == want[3]
        M.check_sorted(r, ex)
        M.check_hot(r, ex)
        ranges.append(want)
        totals += r.M
    assert ranges[0][0] == 0 and ranges[-1][1] == bins1               # the runs tile [0, bins1) in order
    for a, b in zip(ranges, ranges[1:]):
        assert a[1] == b[0]
    assert totals == full.M
    return ranges, full


# (c, planes, random scalars, ones, world).  100 + 200 ones: one partition holds the largest part of a rank's share;
# 40 + 2000 ones: one partition exceeds a fair share, so it is alone in its run and a neighbouring run is empty
@pytest.mark.parametrize("c,planes,n,ones,world", [(13, 0, 900, 0, 4), (14, 3, 600, 0, 8), (12, 0, 100, 200, 3),
                                                   (15, 1, 400, 0, 2), (5, 0, 400, 0, 5), (13, 0, 40, 2000, 4)])
def test_shards(hooks, c, planes, n, ones, world):
    rng = np.random.default_rng(7600 + c + ones)
    words = M.random_words(rng, n)
    if ones:
        words = np.concatenate([words, M.to_words([1] * ones)])[rng.permutation(n + ones)]
    ranges, full = check_shards(hooks, words, True, c, planes, world)
    assert full.M > 0 and sum(1 for r in ranges if r[3]) >= 2
    largest = max(int(x) for x in np.diff(M.part_offsets(full.count, M.part_shift(full.nbt))))
    if ones:
        assert largest >= ones
    if ones == 2000:
        assert largest > full.M // world and any(r[3] == 0 for r in ranges)
        assert any(r[1] - r[0] == 1 and r[3] == largest for r in ranges)


def test_shards_of_nothing(hooks):
    ranges, full = check_shards(hooks, np.zeros((300, 8), dtype=np.uint32), True, 13, 0, 3)
    assert full.M == 0 and all(r[2] == 0 and r[3] == 0 for r in ranges)


# ---- degenerate inputs --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [0, R - 1], ids=["zero", "r-1"])
@pytest.mark.parametrize("mont", [False, True], ids=["canonical", "mont"])
def test_one_scalar(hooks, value, mont):
    r, ex = run_and_check(hooks, [M.to_words([value])], mont, 0, 0)
    assert (ex.M == 0) == (value == 0)


def test_all_zero(hooks):
    r, ex = run_and_check(hooks, [np.zeros((300, 8), dtype=np.uint32)], True, 0, 0)
    assert ex.M == 0 and r.entries.size == 0 and not r.count.any()


@pytest.mark.parametrize("kept", ["none", "all", "one-bucket"])
def test_degenerate_views(hooks, kept):
    rng = np.random.default_rng(7701)
    n = 400
    words = M.random_words(rng, n)
    if kept == "one-bucket":
        keep = rng.integers(0, 4, size=n) == 0
        words[keep] = M.to_words([5])[0]                              # every kept point: the single digit 5
    else:
        keep = np.full(n, kept == "all")
    r, ex = run_and_check(hooks, [words], False, 13, 0, keep=keep)
    if kept == "none":
        assert ex.M == 0 and not r.count.any()
    elif kept == "all":
        assert ex.M == int(r.part_off[-1])
    else:
        assert np.nonzero(ex.count)[0].tolist() == [4] and ex.M == keep.sum() > 50


# ---- configuration and refusals: host only --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(emu):
    return M.Hooks(emu.L)


def test_config_invariants(host):
    for length in (1, 1000, 1 << 11, 1 << 16, 10 ** 5, 1 << 18, 1 << 22, 1 << 27):
        for c in [0] + list(range(2, 25)):
            for planes in (0, 1, 3, 16, 40):
                g = host.config(length, c, planes)                    # Config: W, B, nb, partition shift agree
                if c:
                    assert g.c == c
                assert g.W * g.c >= 255 > (g.W - 1) * g.c
                assert g.Pn * g.D >= g.W and (g.Pn - 1) * g.D < g.W
                assert g.Pn <= 1 << (31 - g.idx_bits)
                assert length <= 1 << g.idx_bits                      # init accepts every one of these lengths
                assert 10 <= g.part_bits <= 12
                assert (1 << g.sh) <= 4096 or g.part_bits == 12
                assert g.lanes >= 1 and g.lanes2 >= 1


def test_init_refusals(host):
    # each is refused before the first allocation: no memory is needed for 2^27 points or 2^32 buckets
    st, msg = host.init((1 << 27) + 1, 16, 0, 1)
    assert st == -1 and "does not fit the sort entry" in msg
    assert host.config(1, 24, 0).nb == 1 << 23
    st, msg = host.init(1, 24, 0, 512)                                # 512 x 2^23 buckets
    assert st == -1 and msg == "MSM bucket count exceeds 2^32"
    assert host.config(1 << 26, 16, 0).W == 16
    st, msg = host.init(1 << 26, 16, 0, 4)                            # 4 x 2^26 x 16 entries
    assert st == -1 and msg == "MSM entry count exceeds 2^32"
    assert host.init(100, 13, 0, 2) == (0, "")


def test_run_refusals(host):
    rng = np.random.default_rng(7801)
    a, b = M.random_words(rng, 10), M.random_words(rng, 10)
    assert host.run([a], True, 13, 0, cap=5, refusal=True) == (-1, "MsmSort::run: more scalars than capacity")
    assert host.run([a, b], True, 13, 0, stride=10, nproof_cap=1, refusal=True) == \
        (-1, "MsmSort::run: more proofs than the chunk capacity")
    assert host.run([a, b], True, 13, 0, stride=10, rank=1, world=2, refusal=True) == \
        (-1, "MsmSort::run: a sharded sort takes one proof")
    assert host.run([a], True, 13, 0, rank=0, world=2, keep=np.ones(10, dtype=bool), refusal=True) == \
        (-1, "MsmSort::run_view: the source sort is sharded")
    assert host.run([a], True, 13, 0, rank=2, world=2, refusal=True) == (-1, "MsmSort::set_shard: bad rank/world")
    assert host.run([a], True, 13, 0, cap=10, refusal=True) == (0, "")
