"""distCUDA2 (ms-gs_amd/csrc/knn.hip) bit for bit against tests/knn_truth.py, at the seams of its box hierarchy.

knn.hip pins `fp contract(off)` and its result is a pure function of the point set (tests/knn_truth.py says why), so
the comparison is assert_array_equal: no tolerance.  A box is 64 Morton-sorted points and a superbox 64 boxes; the sizes
sit on and around P = 64 k and P = 4096 k, the structures defeat the Morton order in the ways a real cloud can."""
import numpy as np
import pytest
import torch

import knn_truth

pytestmark = pytest.mark.gpu


def _dist(t):
    from simple_knn._C import distCUDA2
    return distCUDA2(t).cpu().numpy()


@pytest.mark.parametrize("name", knn_truth.FAMILIES)
def test_kernel_equals_the_float32_truth_bit_for_bit(name):
    pts, truth = knn_truth.family(name)
    knn_truth.assert_normal_range(pts, truth)
    got = _dist(torch.from_numpy(pts.copy()).cuda())
    assert got.dtype == np.float32 and got.shape == truth.shape
    np.testing.assert_array_equal(got, truth)


@pytest.mark.parametrize("name", ["uniform_4161", "two_sheets", "lattice", "coincident"])
def test_result_follows_a_permutation_of_the_points_and_repeats(name):
    pts, truth = knn_truth.family(name)
    perm = np.random.default_rng(99).permutation(len(pts))
    dev = torch.from_numpy(pts.copy()).cuda()
    first = _dist(dev)
    np.testing.assert_array_equal(_dist(dev), first)                                   # two runs, the same bits
    np.testing.assert_array_equal(_dist(torch.from_numpy(pts[perm]).cuda()), first[perm])
    np.testing.assert_array_equal(first[perm], truth[perm])


def test_wrapper_inputs_give_the_bits_of_the_plain_call():
    pts, truth = knn_truth.family("uniform_4097")
    P = len(pts)
    plain = torch.from_numpy(pts.copy()).cuda()
    want = _dist(plain)
    np.testing.assert_array_equal(want, truth)
    np.testing.assert_array_equal(_dist(plain.double()), want)                         # float64 holding float32 values
    wide = torch.full((P, 4), 7.5, device="cuda")
    wide[:, :3] = plain
    view = wide[:, :3]
    assert not view.is_contiguous()
    np.testing.assert_array_equal(_dist(view), want)
    np.testing.assert_array_equal(_dist(plain.clone().requires_grad_(True)), want)
    big = torch.full((P + 3, 3), -3.25, device="cuda")                                 # one row in: a 12-byte offset, so the
    big[1:P + 1] = plain                                                               # kernel's input is not 16-byte aligned
    inner = big[1:P + 1]
    assert inner.is_contiguous() and inner.data_ptr() == big.data_ptr() + 12
    np.testing.assert_array_equal(_dist(inner), want)
    assert (big[0] == -3.25).all() and (big[P + 1:] == -3.25).all() and torch.equal(big[1:P + 1], plain)
    assert (wide[:, 3] == 7.5).all()
