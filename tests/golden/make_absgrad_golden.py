"""Generates tests/golden/absgrad_truth.npz: the float64 truth of the absolute screen-space gradient (DESIGN.md SPEC M10) on
scene F, independent of the op:
    python tests/golden/make_absgrad_golden.py        (CPU only, a few seconds)

tests/replay_truth.render restates the blend loop of oracle/torch_oracle.rasterize with a zero leaf per (list entry, pixel) added
to the pixel-centre distances, so one autograd.grad gives every single pixel's own share of dL/dmeans2D; absgrad is the sum of
their absolute values, the net gradient their plain sum, both scaled to the op's units (0.5 W, 0.5 H).  Pixels the oracle flags as borderline (an alpha or a
transmittance within rounding of a threshold) get dL = 0 here, and the test zeroes the same pixels on the op's side: they
contribute nothing whatever either side decides there.

tests/test_absgrad_cpu.py imports compute() and pins the committed file to it."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

W, H, P, SCENE_SEED, DL_SEED = 40, 24, 200, 1, 78
BG = (0.2, 0.4, 0.1)
PLAIN = dict(filter_small=False, filter_large=False, fade_size=1.0)
import replay_truth as rt                        # noqa: E402  (tests/ is on the path now)
from replay_truth import MAX_BORDERLINE          # noqa: E402  (of the image's pixels)

PATH = os.path.join(HERE, "absgrad_truth.npz")


def scene_f():
    """(scene, camera, bg [3], dL [3,H,W]) of scene F"""
    import scenes
    from parity_utils import small_scene
    sc, cam = small_scene(P, W, H, seed=SCENE_SEED)
    return sc, cam, torch.tensor(BG), scenes.grad_seed(W, H, DL_SEED)


def compute():
    """dict of float64 / bool arrays: absgrad [P,2], grad [P,2] (op units), borderline [H,W], visible [P]"""
    sc, cam, bg, dL = scene_f()
    r = rt.render(sc, cam, PLAIN, bg=bg, per_pixel=True)
    borderline = r.borderline
    assert borderline.sum().item() <= MAX_BORDERLINE * W * H, "too many borderline pixels for this fixture"
    dLm = dL.to(torch.float64) * (~borderline).to(torch.float64)[None]
    g = rt.gradients(r, dict(color=dLm), absgrad=True)
    return dict(absgrad=g["absgrad"].numpy(), grad=g["absgrad_net"].numpy(), borderline=borderline.numpy(),
                visible=(r.radii > 0).numpy())


if __name__ == "__main__":
    out = compute()
    np.savez(PATH, **out)
    a, g, vis = out["absgrad"], out["grad"], out["visible"]
    print(f"visible {int(vis.sum())}  borderline pixels {int(out['borderline'].sum())}  sum|absgrad| {np.abs(a).sum():.4g}  "
          f"sum|grad| {np.abs(g).sum():.4g}  rows with absgrad > 1.5 |grad|: "
          f"{int(((np.linalg.norm(a, axis=1) > 1.5 * np.linalg.norm(g, axis=1)) & vis).sum())}")
