"""GPU voxel-average pooling (ms-gs_amd/csrc/voxel_pool.hip) bit for bit against tests/voxel_pool_truth.py.

Everything the build produces is determined: the voxel of a point is floor of a float32 product clamped in float, the
rows ascend in (z, y, x), points keep ascending ids inside a row and the mean is a sequential float32 sum divided by
float32(count).  So every comparison here is equality — voxel_index, counts, order[:M], seg_start and the float32
bits of average() — at the ends of the 21-bit key fields, on both sides of the key's 32-bit split (bit 11 of the y
field: y = -2049 | -2048 and 2047 | 2048), at the clamp, on exact voxel boundaries, for voxels of one to 70 001 points and
for M around every block edge the build passes through."""
import os
import re

import numpy as np
import pytest
import torch

from voxel_pool_truth import voxel_indices, voxel_pool_truth

pytestmark = pytest.mark.gpu

f32 = np.float32
LO, HI = -(1 << 20), (1 << 20) - 1
# block edges on the way of voxel_pool_build for M < 400 000 (tests/test_sort_gpu.py covers the sort's larger geometries)
VP_LAUNCH = 256             # blockDim of every vp_* kernel
SORT_BLOCK = 256 * 4        # radix_sort_pairs: SORT_THREADS x SORT_ITEMS keys per block
SCAN_CHUNK = 256 * 16       # exclusive_scan_u32: SCAN_THREADS x SCAN_ITEMS values per block


def _check(pos, feats, vs):
    """build on the GPU, compare every output with the truth; returns (grouping, truth)"""
    from voxel_pool import VoxelGrouping
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    feats = np.ascontiguousarray(feats, dtype=np.float32)
    t = voxel_pool_truth(pos, feats, vs)
    g = VoxelGrouping(torch.from_numpy(pos).cuda(), vs)
    M = pos.shape[0]
    assert g.num_voxels == len(t["counts"])
    np.testing.assert_array_equal(g.voxel_index.cpu().numpy(), t["voxel_index"])
    np.testing.assert_array_equal(g.counts.cpu().numpy(), t["counts"])
    np.testing.assert_array_equal(g.order[:M].cpu().numpy(), t["order"])
    np.testing.assert_array_equal(g.seg_start.cpu().numpy(), t["seg_start"])
    got = g.average(torch.from_numpy(feats).cuda()).cpu().numpy()
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, t["features"])
    return g, t


def _features(rng, M, F):
    """columns of very different magnitude (1e-6 .. 1e6 when F allows): nothing a global scale could hide"""
    return rng.standard_normal((M, F)).astype(np.float32) * (f32(10.0) ** rng.integers(-6, 7, size=(1, F)).astype(np.float32))


def test_block_sizes_named_here_are_the_sources():
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ms-gs_amd", "csrc")
    hdr = open(os.path.join(src, "msgs_internal.h")).read()
    val = lambda name: int(re.search(r"constexpr int " + name + r" = (\d+);", hdr).group(1))
    assert val("SORT_THREADS") * val("SORT_ITEMS") == SORT_BLOCK
    assert val("SCAN_THREADS") * val("SCAN_ITEMS") == SCAN_CHUNK
    assert int(re.search(r"SORT_MID_N = ([\d']+);", hdr).group(1).replace("'", "")) > 70_001     # one sort geometry below
    vp = open(os.path.join(src, "voxel_pool.hip")).read()
    assert set(re.findall(r"hipLaunchKernelGGL\(vp_\w+, dim3\([^)]*\)\)?, dim3\((\d+)\)", vp)) == {str(VP_LAUNCH)}


EXTREME = np.array([LO, -2049, -2048, -1, 0, 2047, 2048, HI], dtype=np.int64)


def _extreme_lattice(rng):
    """8^3 voxels at the extreme indices, 1..3 points each at idx + 0.5 (exact in float32), rows shuffled; vs = 1"""
    cells = np.stack(np.meshgrid(EXTREME, EXTREME, EXTREME, indexing="ij"), axis=-1).reshape(-1, 3)
    cells = np.repeat(cells, rng.integers(1, 4, size=len(cells)), axis=0)
    pos = (cells.astype(np.float64) + 0.5).astype(np.float32)
    assert (pos.astype(np.float64) == cells + 0.5).all()
    perm = rng.permutation(len(pos))
    return pos[perm], cells[perm]


def test_extreme_index_lattice():
    rng = np.random.default_rng(21)
    pos, cells = _extreme_lattice(rng)
    np.testing.assert_array_equal(voxel_indices(pos, 1.0), cells)
    g, t = _check(pos, _features(rng, len(pos), 3), 1.0)
    assert g.num_voxels == 512
    want = np.stack(np.meshgrid(EXTREME, EXTREME, EXTREME, indexing="ij"), axis=-1).reshape(-1, 3)[:, ::-1]   # z slowest
    np.testing.assert_array_equal(g.voxel_index.cpu().numpy(), want)


def test_out_of_range_and_infinite_coordinates_share_the_outermost_cells():
    rng = np.random.default_rng(22)
    pos, _ = _extreme_lattice(rng)
    base = voxel_pool_truth(pos, np.zeros((len(pos), 1), np.float32), 1.0)
    extra, cell = [], []
    for axis in range(3):
        for mag in (3e6, 5e8, np.inf):
            for sign, edge in ((1.0, HI), (-1.0, LO)):
                p = np.array([0.5, 2047.5, -0.5], np.float32)
                c = [0, 2047, -1]
                p[axis], c[axis] = sign * mag, edge
                extra.append(p)
                cell.append(c)
    extra.append(np.array([np.inf, -np.inf, np.inf], np.float32))
    cell.append([HI, LO, HI])
    allpos = np.concatenate([pos, np.array(extra, np.float32)])
    perm = rng.permutation(len(allpos))
    g, t = _check(allpos[perm], _features(rng, len(allpos), 3), 1.0)
    assert g.num_voxels == 512                                       # no new cell: each of them joined a lattice cell
    np.testing.assert_array_equal(t["voxel_index"], base["voxel_index"])
    assert t["counts"].sum() == base["counts"].sum() + len(extra)
    got = g.voxel_index.cpu().numpy()[t["inverse"][np.argsort(perm)[len(pos):]]]
    np.testing.assert_array_equal(got, np.array(cell))


@pytest.mark.parametrize("lvl", [1, 2, 3, 4])
def test_exact_multiples_follow_the_product_rule(lvl):
    """p = fl32(k * vs), k = -400..400, on each axis and on the diagonal, at the call site's voxel size 0.02 * lvl / 4:
    the voxel is floor(fl32(p * fl32(1 / vs))), which is NOT floor(p / vs) for about one k in ten"""
    vs = 0.02 * lvl / 4
    k = np.arange(-400, 401)
    p = (k * vs).astype(np.float32)
    rest = f32(0.5 * vs)
    rows = [np.stack([p, p, p], axis=1)]
    for axis in range(3):
        r = np.full((len(k), 3), rest, np.float32)
        r[:, axis] = p
        rows.append(r)
    pos = np.concatenate(rows)
    prod = np.floor(p * (f32(1.0) / f32(vs))).astype(np.int64)
    assert (prod != np.floor(p / f32(vs)).astype(np.int64)).sum() > 50          # the two rules do part on this input
    g, t = _check(pos, _features(np.random.default_rng(lvl), len(pos), 3), vs)
    got = g.voxel_index.cpu().numpy()[t["inverse"]]                             # voxel of every point, as built
    np.testing.assert_array_equal(got[: len(k)], np.stack([prod, prod, prod], axis=1))
    for axis in range(3):
        np.testing.assert_array_equal(got[(axis + 1) * len(k): (axis + 2) * len(k), axis], prod)


@pytest.mark.parametrize("vs", [1.0, 0.005])
def test_signed_zero_and_small_negatives(vs):
    pos = np.array([[-0.0, 0.0, -0.0], [-1e-30, 0.0, 0.0], [0.0, -1e-30, 1e-30], [-0.0, -0.0, -1e-30]], np.float32)
    g, t = _check(pos, np.arange(8, dtype=np.float32).reshape(4, 2), vs)
    got = g.voxel_index.cpu().numpy()[t["inverse"]]
    assert got.tolist() == [[0, 0, 0], [-1, 0, 0], [0, -1, 0], [0, 0, -1]]


def test_one_voxel_holds_every_point():
    """70 001 points, one voxel: a count above 65 535, seg_start = [0, M], one thread sums 70 001 floats in order"""
    rng = np.random.default_rng(31)
    M = 70_001
    pos = rng.random((M, 3), dtype=np.float32) * f32(0.009) + f32(0.0005)
    g, t = _check(pos, _features(rng, M, 3), 0.01)
    assert g.num_voxels == 1 and g.seg_start.cpu().tolist() == [0, M] and g.counts.cpu().tolist() == [M]


def test_one_crowded_voxel_among_sparse_ones():
    rng = np.random.default_rng(32)
    M = 70_001
    pos = rng.random((M, 3), dtype=np.float32) * f32(4) - f32(2)
    crowd = rng.permutation(M)[:69_000]
    pos[crowd] = rng.random((69_000, 3), dtype=np.float32) * f32(0.009) + f32(-1.0095)
    g, t = _check(pos, _features(rng, M, 3), 0.01)
    assert t["counts"].max() == 69_000 and g.num_voxels > 900


@pytest.mark.parametrize("M", [edge + d for edge in (VP_LAUNCH, SORT_BLOCK, SCAN_CHUNK) for d in (-1, 0, 1)])
def test_sizes_around_every_block_edge(M):
    rng = np.random.default_rng(M)
    pos = rng.random((M, 3), dtype=np.float32) * f32(4) - f32(2)
    pos[: M // 10] = np.round(pos[: M // 10], 1)
    _check(pos, _features(rng, M, 3), 0.5)                           # 512 cells: crowded voxels at every M
    _check(pos, _features(rng, M, 3), 0.02)                          # nearly one voxel per point: num_voxels near M


@pytest.mark.parametrize("F", [1, 3, 45, 48])
def test_feature_widths(F):
    rng = np.random.default_rng(40 + F)
    M = 3001
    pos = rng.random((M, 3), dtype=np.float32) * f32(4) - f32(2)
    _check(pos, _features(rng, M, F), 0.5)


def test_columns_twelve_decades_apart():
    """1e-6 beside 1e6: an error of the small column is invisible at the scale of the large one; equality sees it"""
    rng = np.random.default_rng(50)
    M = 5000
    pos = rng.random((M, 3), dtype=np.float32) * f32(4) - f32(2)
    feats = rng.standard_normal((M, 4)).astype(np.float32) * np.array([1e-6, 1e6, 1e-6, 1.0], np.float32)
    g, t = _check(pos, feats, 0.5)
    assert np.abs(t["features"][:, 0]).max() < 1e-5 and np.abs(t["features"][:, 1]).max() > 1e4


def _fresh(src, device, dtype):
    """a new tensor with src's values whose version counter is that of every tensor made this way"""
    t = torch.empty(src.shape, dtype=dtype, device=device)
    t.copy_(src)
    return t


@pytest.mark.parametrize("device,dtype", [("cpu", torch.float32), ("cuda", torch.float64)])
def test_shim_cache_is_not_fooled_by_a_reused_address(device, dtype):
    """Pool A with one VoxelPooling, delete A, allocate B of the same shape until it lands on A's address (up to 20
    tries; a B that landed elsewhere is kept so that the next try cannot get its block): B must be pooled with B's grouping.
    If the host allocator never hands the address out again, B is placed there by construction (see below), so the
    collision is exercised in every run.  On the GPU the positions are float64, which the grouping copies: a float32 contiguous GPU tensor shares its storage
    with the cached grouping, so its address cannot be handed out again while the entry lives (asserted at the end)."""
    from voxel_pool import VoxelPooling
    rng = np.random.default_rng(60)
    M = 70_001
    b_np = rng.random((M, 3), dtype=np.float32) * f32(4) - f32(2)
    feats = _features(rng, M, 3)
    want = voxel_pool_truth(b_np, feats, 0.25)
    b_src = torch.from_numpy(b_np).to(device=device, dtype=dtype)
    a_src = b_src * 0.5                                                # another grouping than B's: an eighth of the rows
    f_dev = torch.from_numpy(feats).cuda()
    vp = VoxelPooling(position_fn="center", feature_fn="average")
    want_centers = (want["voxel_index"].astype(np.float32) + f32(0.5)) * f32(0.25)

    def pool_a_then_b(make_a, make_b):
        """pool A, drop it, make B: (B, did B take A's address and version?); B's result is checked against B's truth"""
        a = make_a()
        ra = vp(a, f_dev, 0.25)
        assert ra.pooled_features.shape[0] != len(want["counts"])
        ptr, ver = a.data_ptr(), a._version
        del a, ra
        b = make_b()
        same = b.data_ptr() == ptr and b._version == ver
        rb = vp(b, f_dev, 0.25)
        assert rb.pooled_features.shape[0] == len(want["counts"])
        np.testing.assert_array_equal(rb.pooled_features.cpu().numpy(), want["features"])
        np.testing.assert_array_equal(rb.pooled_positions.cpu().numpy(), want_centers)
        return b, same

    kept, matched = [], False
    for attempt in range(20):
        b, matched = pool_a_then_b(lambda: _fresh(a_src, device, dtype), lambda: _fresh(b_src, device, dtype))
        kept.append(b)
        if matched:
            break
    if not matched:
        # An allocator need not cooperate: the host's aligned request asks malloc for more than the tensor, so the hole A
        # leaves is too short for B whenever a small live block sits right behind it (seen in the middle of a long
        # session; a fresh process reuses the address at the first try).  Then B is PUT at A's address: both are new
        # tensors over one storage, made the same way (so at the same version), A is dropped and the storage refilled
        # before B is made.
        store = _fresh(a_src.reshape(-1), device, dtype)
        wrap = lambda: torch.empty(0, dtype=dtype, device=device).set_(store.untyped_storage(), 0, (M, 3))

        def b_in_place():
            store.copy_(b_src.reshape(-1))
            return wrap()
        b, matched = pool_a_then_b(wrap, b_in_place)
        kept.append(b)
    assert matched, "no B took the address of its A: the case was not exercised"
    # eleven calls, one grouping: the cached entry answers for the same tensor object
    b = kept[-1]
    g0 = vp._cache[-1]
    for _ in range(11):
        vp(b, f_dev, 0.25)
    assert vp._cache[-1] is g0
    if device == "cuda":
        a32 = _fresh(b_src.float(), "cuda", torch.float32)
        vp(a32, f_dev, 0.25)
        ptr = a32.data_ptr()
        assert vp._cache[-1]._pos.data_ptr() == ptr                    # the grouping holds A's storage ...
        del a32
        assert _fresh(b_src.float(), "cuda", torch.float32).data_ptr() != ptr     # ... so nothing new can live there
