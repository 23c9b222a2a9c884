"""CPU checks of the depth sort's bucket path (ms-gs_amd/csrc/sort.hip, msgs_internal.h): the host rule that chooses it, the
scratch it needs, the bin function, and the splitter restated in numpy (tests/depth_sort_harness.py, splitter) with the property
the whole scheme rests on: whatever the histogram, no bucket holds more than V / 255 + (the largest bin) keys."""
import numpy as np
import pytest

import depth_sort_harness as D
import sort_harness as H

CONST = D.constants()


def test_host_rule_depends_on_n_and_the_switch_alone():
    prev = D.lib().msgsd_get_mode()
    try:
        assert CONST.BUCKET_MAX_P < CONST.HARD_MAX_N < H.thresholds()["scanned"]
        for n in (1, 63, 4096, 100_000, 1_000_000, CONST.BUCKET_MAX_P):
            assert D.uses_buckets(n, D.MODE_AUTO) and D.uses_buckets(n, D.MODE_BUCKETS) and not D.uses_buckets(n, D.MODE_LSD), n
        for n in (CONST.BUCKET_MAX_P + 1, 2_000_000, CONST.HARD_MAX_N):        # C5 and the like stay on the LSD passes
            assert not D.uses_buckets(n, D.MODE_AUTO) and D.uses_buckets(n, D.MODE_BUCKETS) and not D.uses_buckets(n, D.MODE_LSD), n
        for n in (0, -1, CONST.HARD_MAX_N + 1, 6_000_000, 1 << 31):
            for mode in (D.MODE_AUTO, D.MODE_LSD, D.MODE_BUCKETS):
                assert not D.uses_buckets(n, mode), (n, mode)
        assert D.lib().msgsd_set_mode(7) == prev and D.lib().msgsd_get_mode() == D.MODE_AUTO      # unknown values mean "by n"
    finally:
        D.lib().msgsd_set_mode(prev)
    # a bucket bound below the cap with margin at the largest P of the rule: V / 255 leaves room for a bin of 2300 keys
    assert CONST.BUCKET_MAX_P // CONST.BUCKETS + 2300 <= CONST.LDS_CAP
    assert CONST.LDS_CAP == CONST.LDS_THREADS * CONST.LDS_ITEMS


def _sizes():
    t = H.thresholds()
    edge = [1, 2, 255, 256, 257, 32767, 32768, 32769, 65536, 65537, t["mid"] - 1, t["mid"], t["big"] - 1, t["big"],
            CONST.BUCKET_MAX_P, CONST.BUCKET_MAX_P + 1, CONST.HARD_MAX_N - 1, CONST.HARD_MAX_N, CONST.HARD_MAX_N + 1, 6_100_000]
    rng = np.random.default_rng(0)
    return sorted(set(edge + [int(v) for v in rng.integers(1, 7_000_000, 300)]))


def test_scratch_layout_and_stage1_scratch_are_monotone():
    """msgs_stage1_scratch_bytes never shrinks as P grows inside one regime of the LSD sort, and what it holds besides the LSD
    sort's own scratch — the bucket path's tables among it — never shrinks at all.  (The LSD scratch itself does at the two sizes
    where the keys per thread double and the block-histogram table halves: sort_harness.thresholds, known geometry.)"""
    import diff_gaussian_rasterization as dgr
    lib = dgr._C.lib
    last_extra, last_stage1, last_rest, last_regime = 0, 0, 0, None
    for n in _sizes():
        L = D.scratch(n)
        assert L.sort == 0 and H.geom(n).scratch_bytes <= L.coarse < L.zero_end <= L.map < L.bases < L.slices < L.total, (n, L)
        assert all(v % 256 == 0 for v in (L.coarse, L.map, L.bases, L.slices, L.total)), (n, L)
        assert L.map - L.coarse >= 4 * CONST.COARSE and L.bases - L.map >= CONST.BINS and L.slices - L.bases >= 4 * (CONST.BUCKETS + 2)
        blocks = min(64, -(-n // 32768))
        assert L.total - L.slices >= 2 * CONST.BINS * blocks, (n, L)
        # the words to clear: the LSD sort's own range, extended over the group sums of the depth bins
        off, words = D.zero_region(n)
        lsd_off, lsd_words = H.zero_region(n, 0, 32)
        assert off == lsd_off and words >= lsd_words and off + 4 * words == L.zero_end, (n, off, words, L)
        stage1 = int(lib.msgs_stage1_scratch_bytes(n))
        lsd = H.geom(n).scratch_bytes
        extra, rest, regime = L.total - lsd, stage1 - lsd, H.regime(n)
        assert stage1 >= L.total and extra >= last_extra and rest >= last_rest, (n, L, stage1)
        assert regime != last_regime or stage1 >= last_stage1, (n, stage1, last_stage1)
        last_extra, last_stage1, last_rest, last_regime = extra, stage1, rest, regime


def test_bin_function_is_monotone_and_clamped():
    lo, shift, bins = CONST.BIN_LO, CONST.BIN_SHIFT, CONST.BINS
    assert bins == 256 * CONST.COARSE and (lo + bins - 1) == 0x7F7FFFFF >> shift
    edges = np.array([0, 1, (lo << shift) - 1, lo << shift, (lo << shift) + 1, ((lo + 1) << shift) - 1, (lo + 1) << shift,
                      0x3E4CCCCD, 0x3F800000, 0x7F7FFFFF - (1 << shift), 0x7F7FFFFF, 0x7F800000, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF],
                     dtype=np.uint64).astype(np.uint32)
    rng = np.random.default_rng(1)
    keys = np.sort(np.concatenate([edges, rng.integers(0, 1 << 32, 20_000, dtype=np.uint64).astype(np.uint32),
                                   rng.uniform(0.2, 100.0, 20_000).astype(np.float32).view(np.uint32)]))
    b = D.depth_bin(keys)
    assert b.min() == 0 and b.max() == bins - 1 and np.all(np.diff(b) >= 0)               # monotone in the key
    for k in list(edges) + [int(v) for v in keys[::997]]:
        assert int(D.lib().msgsd_depth_bin(int(k))) == int(D.depth_bin(np.array([k], np.uint32))[0]), hex(int(k))
    assert D.depth_bin(np.array([0, (lo << shift) - 1, lo << shift], np.uint32)).tolist() == [0, 0, 0]
    assert D.depth_bin(np.array([(lo + 1) << shift, 0x7F7FFFFF, 0xFFFFFFFE], np.uint32)).tolist() == [1, bins - 1, bins - 1]
    # 512 bins per octave of depth
    assert int(D.depth_bin(np.array([0x40000000], np.uint32))[0]) - int(D.depth_bin(np.array([0x3F800000], np.uint32))[0]) == 512


def _histograms(rng):
    bins = CONST.BINS
    yield "empty", np.zeros(bins, np.int64)
    yield "one key", np.bincount([bins - 1], minlength=bins)
    yield "one bin", np.bincount([777], weights=[300_000], minlength=bins).astype(np.int64)
    yield "first and last bin", np.bincount([0, bins - 1], weights=[5, 9], minlength=bins).astype(np.int64)
    yield "flat", np.full(bins, 3, np.int64)
    for trial in range(40):
        V = int(rng.integers(1, 1_600_000))
        kind = trial % 4
        if kind == 0:       # depths log-uniform over a few octaves
            idx = rng.integers(1000, 1000 + int(rng.integers(1, 6000)), V)
        elif kind == 1:     # a narrow peak on a wide floor
            idx = np.where(rng.random(V) < 0.7, rng.normal(3000, 3 + 40 * rng.random(), V).astype(np.int64) % bins, rng.integers(0, bins, V))
        elif kind == 2:     # a few huge bins
            idx = rng.choice(rng.integers(0, bins, int(rng.integers(1, 12))), V)
        else:               # exponential fall-off from bin 0, most keys in the clamped end bins
            idx = np.minimum(rng.exponential(1 + 500 * rng.random(), V).astype(np.int64) * int(rng.integers(1, 300)), bins - 1)
        yield f"random {trial}", np.bincount(idx, minlength=bins).astype(np.int64)


def test_splitter_never_exceeds_the_bucket_bound():
    """for every histogram: buckets are runs of bins in bin order, bases are the counts in front, and no bucket holds more than
    V / 255 + (the largest bin) keys — 255 * size <= V + 255 * max_bin in integers"""
    B = CONST.BUCKETS
    for what, hist in _histograms(np.random.default_rng(2)):
        bucket, bases = D.splitter(hist)
        V, big = int(hist.sum()), int(hist.max())
        assert len(bucket) == CONST.BINS and len(bases) == B + 2, what
        assert bucket.min() >= 0 and bucket.max() <= B and np.all(np.diff(bucket) >= 0), what
        assert bases[0] == 0 and bases[-1] == V and bases[B] == V and np.all(np.diff(bases) >= 0), what
        size = np.diff(bases)
        assert size[B] == 0, what          # number 255 is what the empty bins behind the last key get: no workgroup is launched for it
        assert np.array_equal(size, np.bincount(bucket, weights=hist, minlength=B + 1).astype(np.int64)), what
        assert int(size.max()) * B <= V + B * big, (what, int(size.max()), V, big)
        # and per bucket with ITS last bin: the run of bins of a bucket starts at a prefix >= k V / 255 and its last bin starts below (k + 1) V / 255
        for k in np.flatnonzero(size):
            last = int(np.flatnonzero(bucket == k)[-1])
            assert int(size[k]) * B <= V + B * int(hist[last]), (what, int(k))


@pytest.mark.parametrize("V,big", [(558_169, 1500), (1_000_000, 2300), (1_500_000, 2300)])
def test_the_rule_keeps_realistic_scenes_inside_lds(V, big):
    """the figures the host rule is sized with: V survivors and a largest bin of `big` keys fit one workgroup's LDS"""
    assert V // CONST.BUCKETS + 1 + big <= CONST.LDS_CAP
