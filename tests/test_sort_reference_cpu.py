"""The host references of tests/test_sort_gpu.py, checked on the CPU: the O(n) checker accepts exactly the argsort result, the
scan reference agrees with a plain loop, and the test-only harness library loads without a GPU and puts every size the GPU tests
derive into the regime they name."""
import numpy as np
import pytest

import sort_harness as H
from sort_reference import check_sorted, compacted_reference, key_field, scan_reference, sort_reference

RANGES = [(0, 32), (0, 13), (3, 16), (24, 32), (0, 1)]


def _inputs(kind, n, rng):
    if kind == "random":
        return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    if kind == "duplicated":        # a handful of distinct fields, random bits around them
        return (rng.integers(0, 5, n, dtype=np.uint64) * 0x01010101 & 0xFFFFFFFF).astype(np.uint32)
    raise ValueError(kind)


# ---------------------------------------------------------------------------------------------------- checker against argsort ---
@pytest.mark.parametrize("bits", RANGES, ids=lambda b: f"bits{b[0]}-{b[1]}")
@pytest.mark.parametrize("vals_kind", ["identity", "permutation"])
@pytest.mark.parametrize("kind", ["random", "duplicated"])
@pytest.mark.parametrize("n", [1, 2, 65, 3000])
def test_checker_accepts_exactly_the_argsort_result(n, kind, vals_kind, bits):
    rng = np.random.default_rng(n * 7 + bits[0] + bits[1])
    keys = _inputs(kind, n, rng)
    vals = None if vals_kind == "identity" else rng.permutation(n).astype(np.uint32)
    k, v = sort_reference(keys, vals, *bits)
    assert check_sorted(keys, vals, k, v, *bits) is None
    f = key_field(k, *bits)
    assert (f[1:] >= f[:-1]).all()
    assert (k == keys[v if vals is None else np.argsort(vals)[v]]).all()
    if n < 2:
        return
    # every other arrangement of the pairs is rejected: swap any two neighbouring pairs
    for i in rng.choice(n - 1, size=min(n - 1, 20), replace=False):
        k2, v2 = k.copy(), v.copy()
        k2[[i, i + 1]] = k2[[i + 1, i]]
        v2[[i, i + 1]] = v2[[i + 1, i]]
        why = check_sorted(keys, vals, k2, v2, *bits)
        assert why is not None and why.startswith("stability" if f[i] == f[i + 1] else "order"), (i, why)


def _case():
    rng = np.random.default_rng(5)
    keys = _inputs("duplicated", 4000, rng) | rng.integers(0, 2, 4000, dtype=np.uint64).astype(np.uint32) << np.uint32(31)
    k, v = sort_reference(keys, None, 0, 32)
    assert check_sorted(keys, None, k, v, 0, 32) is None
    return keys, k, v, key_field(k, 0, 32)


def test_checker_rejects_an_unstable_sort():
    keys, k, v, f = _case()
    i = int(np.argmax(f[1:] == f[:-1]))            # two neighbours with equal keys: swapping them leaves the keys sorted
    v[[i, i + 1]] = v[[i + 1, i]]
    assert check_sorted(keys, None, k, v, 0, 32).startswith("stability")


def test_checker_rejects_one_pair_out_of_order():
    keys, k, v, f = _case()
    i = int(np.argmax(f[1:] != f[:-1]))
    k[[i, i + 1]] = k[[i + 1, i]]
    v[[i, i + 1]] = v[[i + 1, i]]
    assert check_sorted(keys, None, k, v, 0, 32).startswith("order")


def test_checker_rejects_a_duplicated_value():
    keys, k, v, f = _case()
    i = int(np.argmax(f[1:] == f[:-1]))            # the copy has the same key: only the value count gives it away
    v[i + 1] = v[i]
    assert check_sorted(keys, None, k, v, 0, 32).startswith("values")
    v[i + 1] = 4000                                # not an input value at all
    assert check_sorted(keys, None, k, v, 0, 32).startswith("values")


def test_checker_rejects_a_key_detached_from_its_value():
    keys, k, v, f = _case()
    # two values of DIFFERENT keys change places: still a permutation, the keys still sorted
    i = 0
    j = int(np.argmax(f != f[0]))
    v[[i, j]] = v[[j, i]]
    assert check_sorted(keys, None, k, v, 0, 32).startswith("pairing")
    # and with explicit values
    rng = np.random.default_rng(6)
    vals = rng.permutation(4000).astype(np.uint32)
    k, v = sort_reference(keys, vals, 0, 32)
    assert check_sorted(keys, vals, k, v, 0, 32) is None
    v[[i, j]] = v[[j, i]]
    assert check_sorted(keys, vals, k, v, 0, 32).startswith("pairing")


def test_bits_outside_the_range_travel_and_do_not_order():
    rng = np.random.default_rng(7)
    keys = _inputs("random", 2000, rng)
    k, v = sort_reference(keys, None, 3, 16)
    assert (k == keys[v]).all() and (np.sort(k) == np.sort(keys)).all()
    assert not (k[1:] >= k[:-1]).all()
    assert check_sorted(keys, None, k, v, 3, 16) is None
    assert check_sorted(keys, None, *sort_reference(keys, None, 0, 32), 3, 16) is not None


def test_compacted_reference():
    keys = np.array([5, 0xFFFFFFFF, 3, 5, 0xFFFFFFFF, 1], dtype=np.uint32)
    V, k, v = compacted_reference(keys, None, 0, 32)
    assert V == 4 and k.tolist() == [1, 3, 5, 5] and v.tolist() == [5, 2, 0, 3]


# ------------------------------------------------------------------------------------------------------------ scan reference ---
@pytest.mark.parametrize("n", [0, 1, 17, 300])
@pytest.mark.parametrize("variant", ["plain", "gather", "gather-mask", "gather-mask-side", "gather-side"])
def test_scan_reference_against_a_loop(n, variant):
    bits = H.constants().TILE_COUNT_BITS
    rng = np.random.default_rng(n + len(variant))
    m = n + 13
    inp = rng.integers(0, 1 << 32, m, dtype=np.uint64).astype(np.uint32)        # near 2^31 on average: the total passes 2^32
    gather = rng.permutation(m).astype(np.uint32)[:n] if "gather" in variant else None
    mask = (1 << bits) - 1 if "mask" in variant else 0xFFFFFFFF
    out, total, side = scan_reference(inp, n, gather, mask, bits if "side" in variant else None)
    run = 0
    for i in range(n):
        x = int(inp[gather[i]] if gather is not None else inp[i])
        assert int(out[i]) == run % (1 << 32)
        if side is not None:
            assert int(side[i]) == x >> bits
        run += x & mask
    assert total == run and out.dtype == np.uint32 and out.shape == (n,)
    assert (side is None) == ("side" not in variant)
    if n == 300 and variant == "plain":
        assert total > 1 << 32


# ---------------------------------------------------------------------------------------------------------- harness geometry ---
def test_the_harness_library_loads_without_a_gpu_and_answers_the_host_queries():
    c = H.constants()
    assert c.SCAN_CHUNK == c.SCAN_THREADS * c.SCAN_ITEMS and c.SCAN_ITEMS % 4 == 0
    assert H.scan_blocks(0) == 0 and H.scan_blocks(1) == 1 and H.scan_blocks(c.SCAN_CHUNK + 1) == 2
    assert H.keys16_ok(1000, 0, 16) and not H.keys16_ok(1000, 0, 17) and not H.keys16_ok(0, 0, 16)
    assert H.supports_device_count(1000, 0, 32) and not H.supports_device_count(0, 0, 32)
    assert H.zero_region(0, 0, 32) is None
    for n in (1, 5000, H.thresholds()["big"]):
        g = H.geom(n)
        for bits, passes in (((0, 8), 1), ((0, 13), 2), ((0, 17), 3), ((0, 32), 4), ((5, 32), 4)):
            off, words = H.zero_region(n, *bits)
            # the group sums of `passes` passes, right behind the block histograms; the scratch holds four passes' worth
            assert words == passes * 256 * g.ngroups
            assert off % 256 == 0 and off >= 8 * n and off + 4 * 256 * g.ngroups * 4 <= g.scratch_bytes
            assert off + 4 * words <= g.scratch_bytes


def test_the_sizes_the_gpu_tests_derive_land_in_the_regimes_they_name():
    c = H.constants()
    t = H.thresholds()
    assert H.geom(t["mid"]).items == 8 and H.geom(t["mid"] - 1).items == 4
    assert H.geom(t["big"]).items == 16 and H.geom(t["big"] - 1).items == 8
    assert H.geom(t["scanned"]).scanned and not H.geom(t["scanned"] - 1).scanned
    expect = {"mid-1": "items4", "mid": "items8", "mid+chunk+1": "items8", "big-1": "items8", "big": "items16",
              "big+chunk+1": "items16", "scanned-1": "items16", "scanned": "items16-scanned",
              "scanned+chunk+1": "items16-scanned"}
    got = {what: H.regime(n) for n, what in H.boundary_sizes()}
    assert got == expect
    assert set(got.values()) == set(H.REGIMES)                  # all four code paths are among the derived sizes
    by_what = {what: n for n, what in H.boundary_sizes()}
    for name in ("mid", "big", "scanned"):                      # + one chunk + 1: one more block
        n = by_what[name + "+chunk+1"]
        assert H.geom(n).nb == H.geom(t[name]).nb + 1 and n == t[name] + H.chunk(n) + 1
    assert dict(H.regime_sizes()).keys() == set(H.REGIMES)
    # one group of blocks, and the first size whose groups are larger
    sizes = {what: n for n, what in H.group_sizes()}
    g = H.geom(sizes["group"])
    assert g.nb == g.gsize == 8 and g.ngroups == 1 and H.geom(sizes["group+1"]).ngroups == 2
    assert H.geom(sizes["gsize-grows-1"]).gsize == 8 and H.geom(sizes["gsize-grows"]).gsize > 8
    assert H.geom(sizes["gsize-grows"]).nb == 65
    assert all(H.regime(n) == "items4" for n in sizes.values())
    # the scanned route starts at SORT_SCANNED_MIN_BLOCKS blocks
    assert H.geom(t["scanned"]).nb == c.SORT_SCANNED_MIN_BLOCKS and H.geom(t["scanned"]).gsize == c.SORT_SCANNED_GSIZE


def test_group_geometry_for_every_block_count():
    """Every block count the three unscanned regimes can have (each n at which nb changes, up to the scanned threshold): the group
    size is the smallest multiple of 8 whose square covers nb — SortGeom's SORT_MAX_GROUPS floor never raises it, because that
    needs nb > SORT_MAX_GROUPS^2 = 16 384 and the scanned route takes over at SORT_SCANNED_MIN_BLOCKS = 4096 — the groups
    cover the blocks, and there are at most SORT_MAX_GROUPS of them.  Behind the threshold every size is scanned."""
    c = H.constants()
    t = H.thresholds()
    assert c.SORT_SCANNED_MIN_BLOCKS <= c.SORT_MAX_GROUPS ** 2
    seen = set()
    for lo, hi in ((1, t["mid"] - 1), (t["mid"], t["big"] - 1), (t["big"], t["scanned"] - 1)):
        ch = H.chunk(lo)
        edges = {lo, hi} | {k for b in range(lo // ch, hi // ch + 2) for k in (b * ch, b * ch + 1) if lo <= k <= hi}
        for n in sorted(edges):
            g = H.geom(n)
            assert not g.scanned and g.items * c.SORT_THREADS == ch
            assert g.nb == -(-n // ch)
            want = 8
            while want * want < g.nb:
                want += 8
            assert g.gsize == want, (n, g)
            assert g.ngroups == -(-g.nb // g.gsize) and g.ngroups <= c.SORT_MAX_GROUPS
            assert g.scratch_bytes >= 8 * n + 4 * 256 * (g.nb + 4 * g.ngroups)
            seen.add((g.items, g.nb))
    assert len(seen) > 1000
    for n in [t["scanned"] + k * 9_999_991 for k in range(0, 400, 7)] + [(1 << 32) - 1, 1 << 32]:
        g = H.geom(n)
        assert g.scanned and g.items == 16 and g.gsize == c.SORT_SCANNED_GSIZE and g.ngroups == -(-g.nb // g.gsize)
