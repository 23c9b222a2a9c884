"""tests/knn_truth.py (float32 all pairs) against oracle/knn_oracle.py (float64 kd-tree, float32 evaluation): the two
share no code and must agree bit for bit on every input family tests/test_knn_exact_gpu.py runs on the kernel."""
import numpy as np
import pytest

import knn_truth
from oracle import knn_oracle


@pytest.mark.parametrize("name", knn_truth.FAMILIES)
def test_truth_equals_the_kdtree_oracle_bit_for_bit(name):
    pts, truth = knn_truth.family(name)
    knn_truth.assert_normal_range(pts, truth)
    np.testing.assert_array_equal(truth, knn_oracle.mean_dist2_knn3(pts))


def test_truth_on_cases_known_by_hand():
    # a unit square plus one far point: every corner sees 1, 1, 2
    sq = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [50, 50, 50]], np.float32)
    got = knn_truth.mean_dist2_knn3(sq)
    np.testing.assert_array_equal(got[:4], np.full(4, np.float32(4.0) / np.float32(3.0)))
    # float32 operation order: (dx*dx + dy*dy) + dz*dz differs from dx*dx + (dy*dy + dz*dz) for these values
    a = np.float32(1.0) + np.float32(2.0 ** -12)
    p = np.array([[0, 0, 0], [a, a, 2.0 ** -12]] + [[0, 0, 0]] * 2, np.float32)
    dx2 = a * a
    want = ((np.float32(0) + np.float32(0)) + ((dx2 + dx2) + np.float32(2.0 ** -24))) / np.float32(3.0)
    assert knn_truth.mean_dist2_knn3(p)[0] == want
    # duplicates count with distance 0 and a point is excluded by its index only
    _, lat = knn_truth.family("lattice")
    assert (lat == 1.0).all()
    pts, co = knn_truth.family("coincident")
    assert (co[1000:1100] == 0).all() and (co[:1000] > 0).all()
    # chunking does not change anything
    u, t = knn_truth.family("uniform_4097")
    np.testing.assert_array_equal(knn_truth.mean_dist2_knn3(u, chunk=1000), t)
