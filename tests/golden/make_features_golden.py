"""Generates tests/golden/features_truth.npz: the float64 truth of the feature-channel render (DESIGN.md SPEC M12) on scene F,
independent of the op:
    python tests/golden/make_features_golden.py        (CPU only, a few seconds)

tests/replay_truth.render restates the blend loop of oracle/torch_oracle.rasterize and blends any number of channels with its
weights, F[c,p] = sum_i f_ic w_ip over a zero background.  C = 5 seeded features in [0, 1] go through it in float64, and autograd
of sum G * F (replay_truth.gradients) gives dL/dfeatures and the geometry gradients (means3D, opacities, scales, rotations;
means2D from the pixel-unit leaf, scaled to the op's units).  Pixels the oracle flags as borderline (an alpha or a transmittance
within rounding of a threshold) get G = 0 here, and the test zeroes the same pixels on the op's side and leaves them out of the
map comparison: they contribute nothing whatever either side decides there.

tests/test_features_cpu.py imports compute() and pins the committed file to it."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

W, H, P, C, SCENE_SEED, FEATURE_SEED, G_SEED = 40, 24, 200, 5, 1, 91, 92
PLAIN = dict(filter_small=False, filter_large=False, fade_size=1.0)
import replay_truth as rt                        # noqa: E402  (tests/ is on the path now)
from replay_truth import MAX_BORDERLINE          # noqa: E402  (of the image's pixels)

PATH = os.path.join(HERE, "features_truth.npz")


def scene_f():
    """(scene, camera) of scene F (make_absgrad_golden.py)"""
    from parity_utils import small_scene
    return small_scene(P, W, H, seed=SCENE_SEED)


def features():
    """[P,C] float32, seeded, uniform in [0, 1)"""
    return torch.rand(P, C, generator=torch.Generator().manual_seed(FEATURE_SEED))


def seed_map():
    """G = dL/dF [C,H,W] float32, seeded, uniform in (-0.5, 0.5)"""
    return torch.rand(C, H, W, generator=torch.Generator().manual_seed(G_SEED)) - 0.5


def compute():
    """dict: features [P,C] f32, G [C,H,W] f32 (zero on borderline pixels), map [C,H,W] f64, dfeatures [P,C] f64, the geometry
    gradients means3D [P,3], opacities [P,1], scales [P,3], rotations [P,4], means2D [P,3] (op units) f64, borderline [H,W] bool,
    visible [P] bool"""
    sc, cam = scene_f()
    r = rt.render(sc, cam, PLAIN, features=features())
    borderline = r.borderline
    assert borderline.sum().item() <= MAX_BORDERLINE * W * H, "too many borderline pixels for this fixture"
    G = seed_map() * (~borderline).to(torch.float32)[None]
    g = rt.gradients(r, dict(features=G))
    return dict(features=features().numpy(), G=G.numpy(), map=r.features.detach().numpy(), dfeatures=g["features"].numpy(),
                means3D=g["means3D"].numpy(), opacities=g["opacities"].numpy(), scales=g["scales"].numpy(),
                rotations=g["rotations"].numpy(), means2D=g["means2D"].numpy(), borderline=borderline.numpy(),
                visible=(r.radii > 0).numpy())


if __name__ == "__main__":
    out = compute()
    np.savez(PATH, **out)
    print(f"visible {int(out['visible'].sum())}  borderline pixels {int(out['borderline'].sum())} of {W * H}  "
          f"max |map| {np.abs(out['map']).max():.4g}  pixels with a zero map {(np.abs(out['map']).sum(0) == 0).sum()}  "
          f"max |dfeatures| {np.abs(out['dfeatures']).max():.4g}  max |means3D grad| {np.abs(out['means3D']).max():.4g}")
