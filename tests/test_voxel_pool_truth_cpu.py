"""tests/voxel_pool_truth.py (exact float32) against oracle/voxel_pool_oracle.py (float64 means), the clamp of both at
+-2^20, the float32 sum order, and the cache rule of the VoxelPooling shim — all without a GPU."""
import warnings

import numpy as np
import pytest
import torch

from oracle.voxel_pool_oracle import voxel_average_pool
from voxel_pool_truth import voxel_indices, voxel_pool_truth

f32 = np.float32
LO, HI = -(1 << 20), (1 << 20) - 1


def _order_of(inverse):
    return np.argsort(inverse, kind="stable")


@pytest.mark.parametrize("M,F,vs,seed", [(1, 3, 0.5, 0), (257, 1, 0.1, 1), (5000, 7, 0.02, 2), (20_000, 45, 0.01, 3),
                                          (70_001, 3, 0.005, 4), (4097, 48, 1.0, 5)])
def test_truth_matches_the_oracle_on_finite_input(M, F, vs, seed):
    rng = np.random.default_rng(seed)
    pos = (rng.random((M, 3), dtype=np.float32) * f32(4) - f32(2))
    pos[: M // 10] = np.round(pos[: M // 10], 1)                       # coincident points: voxels with many members
    if seed == 5:
        pos[: M // 2] = f32(0.25)                                      # one voxel with half of all points
    feats = rng.standard_normal((M, F)).astype(np.float32) * f32(10.0) ** rng.integers(-6, 7, size=(1, F)).astype(np.float32)
    t, o = voxel_pool_truth(pos, feats, vs), voxel_average_pool(pos, feats, vs)
    np.testing.assert_array_equal(t["voxel_index"], o["voxel_index"])
    np.testing.assert_array_equal(t["counts"], o["counts"])
    np.testing.assert_array_equal(t["inverse"], o["inverse"])
    np.testing.assert_array_equal(t["order"], _order_of(o["inverse"]))
    np.testing.assert_array_equal(np.diff(t["seg_start"]), o["counts"])
    assert t["seg_start"][0] == 0 and t["seg_start"][-1] == M
    # a float32 sequential sum of n terms is within (n - 1) u sum|x| of the exact sum (u = 2^-24), the division adds one
    # rounding of the mean: count * 2^-24 * sum|feature| covers both, per voxel and column
    sum_abs = np.zeros(o["features"].shape)
    np.add.at(sum_abs, o["inverse"], np.abs(feats.astype(np.float64)))
    bound = o["counts"][:, None] * 2.0 ** -24 * sum_abs
    err = np.abs(t["features"].astype(np.float64) - o["features"])
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    assert t["features"].dtype == np.float32


def test_truth_sum_is_the_sequential_float32_loop():
    """np.add.at on float32 = `s = 0.f; for m in ascending point id: s += x[m]`, then s / float(count)"""
    rng = np.random.default_rng(11)
    M, F = 3000, 4
    pos = rng.random((M, 3), dtype=np.float32)
    feats = (rng.standard_normal((M, F)) * 10.0 ** rng.integers(-6, 7, size=(M, F))).astype(np.float32)
    t = voxel_pool_truth(pos, feats, 0.34)                             # 27 voxels, ~110 points each
    assert t["counts"].max() > 50
    want = np.empty_like(t["features"])
    for v in range(len(t["counts"])):
        for f in range(F):
            s = f32(0.0)
            for m in t["order"][t["seg_start"][v]: t["seg_start"][v + 1]]:
                s = s + feats[m, f]
            want[v, f] = s / f32(t["counts"][v])
    np.testing.assert_array_equal(t["features"], want)
    # and the order matters: summing in float64 first gives different bits somewhere
    o = voxel_average_pool(pos, feats, 0.34)
    assert (o["features"].astype(np.float32) != t["features"]).any()


def test_out_of_range_and_infinite_coordinates_clamp_to_their_side():
    big = np.array([3e6, 5e8, np.inf], np.float32)
    for oracle_like in (lambda p: voxel_indices(p, 1.0), lambda p: voxel_average_pool(p, np.zeros((len(p), 1), np.float32), 1.0)):
        for axis in range(3):
            for sign, edge in ((1.0, HI), (-1.0, LO)):
                pos = np.full((len(big) + 1, 3), 0.5, np.float32)
                pos[:-1, axis] = sign * big
                pos[-1, axis] = edge + 0.5                             # the outermost cell of that side
                with warnings.catch_warnings():
                    warnings.simplefilter("error")                     # the cast must not see a value it cannot hold
                    r = oracle_like(pos)
                if isinstance(r, dict):
                    assert r["voxel_index"].shape == (1, 3) and r["counts"].tolist() == [len(big) + 1]
                    r = r["voxel_index"]
                want = [0, 0, 0]
                want[axis] = edge
                assert (r == np.array(want)).all(), (axis, sign, r)
    # the same with a small voxel: the product overflows the range, not the coordinate
    assert voxel_indices(np.array([[30000.0, -30000.0, 0.0]], np.float32), 0.005).tolist() == [[HI, LO, 0]]
    assert voxel_average_pool(np.array([[30000.0, -30000.0, 0.0]], np.float32), np.zeros((1, 1)), 0.005)["voxel_index"].tolist() == [[HI, LO, 0]]
    # signed zero and the smallest negatives
    assert voxel_indices(np.array([[-0.0, -1e-30, 0.0]], np.float32), 1.0).tolist() == [[0, -1, 0]]


def test_product_rule_differs_from_the_quotient_on_exact_multiples():
    """the rule as built is floor(fl32(p * fl32(1 / vs))); on p = fl32(k * vs) the quotient rule disagrees for these many k"""
    k = np.arange(-400, 401)
    differing = []
    for lvl in (1, 2, 3, 4):
        vs = 0.02 * lvl / 4
        p = (k * vs).astype(np.float32)
        pos = np.stack([p, p, p], axis=1)
        prod = voxel_indices(pos, vs)[:, 0]
        assert (prod == np.floor(p * (f32(1.0) / f32(vs))).astype(np.int64)).all()
        quot = np.floor(p / f32(vs)).astype(np.int64)
        differing.append(int((prod != quot).sum()))
        np.testing.assert_array_equal(voxel_average_pool(pos, np.zeros((len(k), 1)), vs)["voxel_index"][:, 0], np.unique(prod))
    assert differing == [85, 85, 242, 85], differing                  # of 801 each: a fact of IEEE float32, no kernel involved


class _CountingGrouping:
    built = 0

    def __init__(self, positions, voxel_size):
        type(self).built += 1
        self.positions = positions.clone()
        self.centers = None

    def average(self, features):
        return self.positions                                         # lets the caller see WHICH positions were grouped


def test_shim_cache_hits_only_the_same_live_tensor(monkeypatch):
    """eleven calls with one positions tensor build one grouping; a new tensor at the freed tensor's address, an in-place
    change, another voxel size or an equal copy build a new one"""
    import voxel_pool
    monkeypatch.setattr(voxel_pool, "VoxelGrouping", _CountingGrouping)
    _CountingGrouping.built = 0
    vp = voxel_pool.VoxelPooling()
    a = torch.zeros(1000, 3)
    for _ in range(11):
        vp(a, None, 0.1)
    assert _CountingGrouping.built == 1
    vp(a.clone(), None, 0.1)
    vp(a, None, 0.1)
    vp(a, None, 0.2)
    assert _CountingGrouping.built == 4
    a.add_(1.0)
    assert (vp(a, None, 0.2).pooled_features == 1.0).all() and _CountingGrouping.built == 5
    # address reuse: the stale grouping must not answer for the new tensor
    matched = False
    for attempt in range(20):
        a = torch.empty(70_001, 3)
        a.fill_(float(attempt))
        vp(a, None, 0.1)
        ptr, ver = a.data_ptr(), a._version
        del a
        b = torch.empty(70_001, 3)
        b.fill_(-1.0)
        matched = b.data_ptr() == ptr and b._version == ver
        got = vp(b, None, 0.1).pooled_features
        assert (got == -1.0).all()
        if matched:
            break
    if not matched:
        # the allocator need not cooperate (an aligned request needs more room than the hole the freed tensor leaves when
        # a small live block sits behind it): then B is PUT at A's address, both wrapping one buffer, both at version 0
        buf = np.zeros((70_001, 3), np.float32)
        a = torch.from_numpy(buf)
        vp(a, None, 0.1)
        ptr, ver = a.data_ptr(), a._version
        del a
        buf[...] = -1.0
        b = torch.from_numpy(buf)
        matched = b.data_ptr() == ptr and b._version == ver
        assert (vp(b, None, 0.1).pooled_features == -1.0).all()
    assert matched, "no B took the address of its A: the case was not exercised"
