"""Float32 all-pairs truth for distCUDA2 (ms-gs_amd/csrc/knn.hip), and the input families both knn test files use.

knn.hip is compiled with `#pragma clang fp contract(off)`, so every float32 operation of scan_box and knn_query_kernel
rounds on its own and numpy's float32 arithmetic reproduces it bit for bit:

    d       = ((dx*dx + dy*dy) + dz*dz)      with dx = q.x - x (candidate minus query), every step rounded to float32
    b0..b2  = the three smallest d over all OTHER indices (a point is excluded by its index only), ascending
    result  = ((b0 + b1) + b2) / 3.0f        (IEEE division, correctly rounded)

The three smallest VALUES do not depend on the order in which the kernel meets the candidates, and its box pruning only
discards candidates whose float32 lower bound (same operation order, monotone under rounding) is not below b2: the
result is a pure function of the point set.  Nothing here shares code with oracle/knn_oracle.py (float64 kd-tree, then
a float32 evaluation of the neighbours it chose); tests/test_knn_truth_cpu.py requires the two to agree bit for bit.
"""
import numpy as np

f32 = np.float32
FLT_MAX = np.finfo(np.float32).max


def mean_dist2_knn3(points, chunk=256):
    """[P, 3] -> [P] float32, P >= 4.  Memory: chunk * P floats per temporary."""
    pts = np.ascontiguousarray(points, dtype=np.float32)
    P = pts.shape[0]
    assert pts.ndim == 2 and pts.shape[1] == 3 and P >= 4, pts.shape
    x, y, z = pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy()
    out = np.empty(P, dtype=np.float32)
    for c in range(0, P, chunk):
        e = min(P, c + chunk)
        dx = x[None, :] - x[c:e, None]
        dy = y[None, :] - y[c:e, None]
        dz = z[None, :] - z[c:e, None]
        d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == np.float32
        d[np.arange(e - c), np.arange(c, e)] = FLT_MAX              # self: excluded by index only
        b = np.sort(np.partition(d, 2, axis=1)[:, :3], axis=1)
        out[c:e] = ((b[:, 0] + b[:, 1]) + b[:, 2]) / f32(3.0)
    return out


# ---------------------------------------------------------------------------------------------------------------
# Input families.  A box is 64 Morton-sorted points and a superbox 64 boxes, so the hierarchy has seams at P = 64 k
# and P = 4096 k: every size below sits on a seam or one step off it.  4161 = 65 * 64 + 1: two superboxes, the second
# holding one full box and a one-point box.
# ---------------------------------------------------------------------------------------------------------------
SIZES = (4, 5, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 4161, 8193)


def uniform_cube(P):
    rng = np.random.default_rng(7000 + P)
    return (rng.random((P, 3), dtype=np.float32) * f32(10.0) - f32(5.0))


def _two_sheets():
    """x = 0.5 -/+ 1e-3 inside a unit bounding box: the nearest neighbours of the points lie across the top Morton split"""
    rng = np.random.default_rng(7101)
    P = 8193
    pts = rng.random((P, 3), dtype=np.float32)
    pts[:, 0] = np.where(np.arange(P) % 2 == 0, f32(0.5 - 1e-3), f32(0.5 + 1e-3))
    pts[0], pts[1] = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)              # the corners that make the bounding box the unit cube
    return pts


def _far_outlier():
    """one point at (1e6, -1e6, 1e6): the 10-bit Morton grid collapses, every other point gets the same code, the boxes
    overlap completely and nothing is pruned"""
    rng = np.random.default_rng(7102)
    pts = rng.random((8193, 3), dtype=np.float32)
    pts[5000] = (1e6, -1e6, 1e6)
    return pts


def _lattice():
    """shuffled 20^3 integer lattice: every answer is exactly 1.0 with 3 to 6 tied nearest neighbours"""
    g = np.arange(20, dtype=np.float32)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    np.random.default_rng(7103).shuffle(pts)
    return np.ascontiguousarray(pts)


def _offset_cube():
    """unit cube moved to 4096: coordinates carry 2^-11 of resolution, differences are exact, duplicates are frequent"""
    return np.random.default_rng(7104).random((4097, 3), dtype=np.float32) + f32(4096.0)


def _coincident():
    pts = np.random.default_rng(7105).random((4161, 3), dtype=np.float32)
    pts[1000:1100] = pts[1000]
    return pts


def _line():
    t = np.random.default_rng(7106).random(4096, dtype=np.float32)
    return np.stack([t, f32(2.0) * t, f32(-3.0) * t], axis=1)


STRUCTURES = {"two_sheets": _two_sheets, "far_outlier": _far_outlier, "lattice": _lattice, "offset_cube": _offset_cube,
              "coincident": _coincident, "line": _line}
FAMILIES = tuple(f"uniform_{P}" for P in SIZES) + tuple(STRUCTURES)

_cache = {}


def family(name):
    """(points, truth) of a named input; both are computed once per process and must be left unchanged"""
    if name not in _cache:
        pts = uniform_cube(int(name.split("_")[1])) if name.startswith("uniform_") else STRUCTURES[name]()
        pts = np.ascontiguousarray(pts, dtype=np.float32)
        truth = mean_dist2_knn3(pts)
        pts.setflags(write=False)
        truth.setflags(write=False)
        _cache[name] = (pts, truth)
    return _cache[name]


def assert_normal_range(pts, truth):
    """coordinates, and every nonzero answer, stay out of the float32 denormal range (the kernel is not asked what it does
    with denormals); everything is finite"""
    tiny = np.finfo(np.float32).tiny
    assert np.isfinite(pts).all() and np.isfinite(truth).all()
    assert ((pts == 0) | (np.abs(pts) >= tiny)).all()
    assert ((truth == 0) | (truth >= tiny * 1e8)).all()
