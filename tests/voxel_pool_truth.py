"""Exact float32 truth for GPU voxel-average pooling (ms-gs_amd/csrc/voxel_pool.hip): every output bit for bit.

    index      = floor(fl32(p * fl32(1 / voxel_size))) per axis, clamped IN FLOAT to [-2^20, 2^20 - 1] with fmaxf / fminf
                 (so +-inf and out-of-range coordinates land in the outermost cells), then cast
    rows       = the occupied voxels in ascending (z, y, x)
    order      = point ids grouped by row, ascending inside a row; seg_start = the row boundaries, closed by M
    mean       = float32 sequential sum in ascending point id, starting from +0, divided by float32(count)

The sum is what vp_mean_kernel does with one thread per (voxel, feature): np.add.at on float32 arrays is unbuffered and
walks the indices in order, i.e. the same additions in the same order (checked against an explicit loop in
tests/test_voxel_pool_truth_cpu.py).  The kernel's product and division are single IEEE operations and nothing in the file
can be contracted into an fma, so numpy's float32 arithmetic reproduces them.
"""
import numpy as np

f32 = np.float32
BIAS = 1 << 20


def voxel_indices(positions, voxel_size):
    """[M, 3] int64 voxel index of every point"""
    pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
    inv = f32(1.0) / f32(voxel_size)
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.floor(pos * inv)
    assert v.dtype == np.float32
    v = np.fmin(np.fmax(v, f32(-BIAS)), f32(BIAS - 1))              # fmaxf / fminf: a NaN gives the other operand
    return v.astype(np.int64)


def voxel_pool_truth(positions, features, voxel_size):
    idx = voxel_indices(positions, voxel_size)
    M = idx.shape[0]
    key = ((idx[:, 2] + BIAS) << 42) | ((idx[:, 1] + BIAS) << 21) | (idx[:, 0] + BIAS)
    order = np.argsort(key, kind="stable")                          # ascending point id inside a voxel
    ks = key[order]
    head = np.ones(M, dtype=bool)
    head[1:] = ks[1:] != ks[:-1]
    starts = np.flatnonzero(head)
    seg_start = np.concatenate([starts, [M]]).astype(np.int64)
    counts = np.diff(seg_start)
    Mv = starts.shape[0]
    inverse = np.empty(M, dtype=np.int64)
    inverse[order] = np.cumsum(head) - 1
    feats = np.ascontiguousarray(features, dtype=np.float32).reshape(M, -1)
    sums = np.zeros((Mv, feats.shape[1]), dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        np.add.at(sums, inverse, feats)
        means = sums / counts.astype(np.float32)[:, None]
    assert sums.dtype == np.float32 and means.dtype == np.float32
    return dict(voxel_index=idx[order[starts]], counts=counts, order=order, seg_start=seg_start, features=means,
                inverse=inverse)
