"""SPEC Q10's tie rule (equal float32 depth bits blend in Gaussian-index order) inside the CHECKER, without a GPU: the float32 C++
oracle (stable_sort on tile << 32 | depth) and the float64 autograd oracle (stable argsort on the float32 depth) state the rule
independently and have to agree on scenes in which it decides every pixel — tests/tie_scenes.py: one depth plane, and four
planes two of which differ in the lowest key bit, both with densify-style clones.  And the scenes must stay what they claim to
be: rendering the rows in the opposite index order has to move nearly every pixel by far more than the forward tolerance, or the
GPU tests built on them (tests/test_depth_ties_gpu.py) would pass whatever order the kernels produce."""
import pytest
import torch

import scenes
import tie_scenes
from oracle import oracle_ctypes as oc
from test_oracle_cpu import ST0, _compare

# (P, W, H, seed, levels).  _compare holds EVERY Gaussian's gradient to 1e-4, the flagged ones too, and an alpha that the float32
# and the float64 evaluation put on different sides of 1/255 moves its Gaussian by ~1e-3 (seed 2 of the four planes: row 324,
# flagged by the oracle).  That is Q7, not Q10: the seeds are the lowest at which the float32 oracle flags NO undecided decision
# on these inputs (asserted below as a property of the input).
CASES = {"one_plane": (260, 56, 40, 4, tie_scenes.ONE_PLANE), "four_planes": (400, 72, 48, 3, tie_scenes.FOUR_PLANES)}


def _case(name):
    P, W, H, seed, levels = CASES[name]
    sc = tie_scenes.tied_scene(P, W, H, seed, levels, culled=0.1, px=3.0, clones=0.5)
    tie_scenes.assert_tied(sc.means3D[:, 2], levels)
    return sc, scenes.front_camera(W, H), levels


@pytest.mark.parametrize("name", list(CASES))
def test_c_oracle_matches_autograd_on_tied_depths(name):
    """test_oracle_cpu._compare's bounds as they are (forward 1e-5, gradients 1e-4 on every Gaussian, radii equal); on the
    Gaussians the oracle does not flag the two agree to ~2e-6"""
    sc, cam, levels = _case(name)
    r, outs = _compare(sc, cam, ST0, (0.1, 0.3, 0.6))
    assert int(r.borderline_gaussians.sum()) == 0 and int(r.borderline.sum()) == 0
    # the clones are there, and rendered: pairs with bit-identical means P / 2 rows apart
    half = sc.P // 2
    pair = (sc.means3D[:half] == sc.means3D[half:2 * half]).all(dim=1) & (r.radii[:half] > 0)
    assert int(pair.sum()) >= sc.P // 8, int(pair.sum())
    assert torch.equal(r.radii[:half][pair], r.radii[half:2 * half][pair])


@pytest.mark.parametrize("name", list(CASES))
def test_reversing_the_rows_changes_nearly_every_pixel(name):
    sc, cam, _ = _case(name)
    bg = torch.tensor([0.1, 0.3, 0.6])
    a = oc.rasterize(sc, cam, ST0, bg)
    b = oc.rasterize(tie_scenes.reversed_rows(sc), cam, ST0, bg)
    assert torch.equal(a.radii, b.radii.flip(0))
    moved = (a.color - b.color).abs().max(dim=0).values > 1e-5
    frac = moved.float().mean().item()
    print(f"[ties] {name}: pixels moved by reversing the index order {frac:.4f}, "
          f"largest change {(a.color - b.color).abs().max().item():.3f}")
    assert frac > 0.9, frac
