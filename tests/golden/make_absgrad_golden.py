"""Generates tests/golden/absgrad_truth.npz: the float64 truth of the absolute screen-space gradient (DESIGN.md SPEC M10) on
scene F, independent of the op:
    python tests/golden/make_absgrad_golden.py        (CPU only, a few seconds)

oracle/torch_oracle.rasterize returns a float64 image with an `aux["means2D"]` leaf in pixel units, so the gradient of every
single pixel's loss term is one batched autograd.grad over the pixels; absgrad is the sum of their absolute values, the net
gradient their plain sum, both scaled to the op's units (0.5 W, 0.5 H).  Pixels the oracle flags as borderline (an alpha or a
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
MAX_BORDERLINE = 0.02          # of the image's pixels
PATH = os.path.join(HERE, "absgrad_truth.npz")


def scene_f():
    """(scene, camera, bg [3], dL [3,H,W]) of scene F"""
    import scenes
    from parity_utils import small_scene
    sc, cam = small_scene(P, W, H, seed=SCENE_SEED)
    return sc, cam, torch.tensor(BG), scenes.grad_seed(W, H, DL_SEED)


def compute():
    """dict of float64 / bool arrays: absgrad [P,2], grad [P,2] (op units), borderline [H,W], visible [P]"""
    from oracle import torch_oracle as to
    sc, cam, bg, dL = scene_f()
    dt = torch.float64
    view = to.view_dict(cam, sh_degree=sc.sh_degree, **PLAIN)
    kw = dict(max_pixel_sizes=sc.max_pixel_sizes, min_pixel_sizes=sc.min_pixel_sizes, base_mask=sc.base_mask,
              scales=sc.scales.to(dt), rotations=sc.rotations.to(dt), shs=sc.shs.to(dt))
    color, _, _, radii, _, aux = to.rasterize(sc.means3D.to(dt), sc.opacities.to(dt), view, bg, **kw)
    borderline = aux["borderline"]
    assert borderline.sum().item() <= MAX_BORDERLINE * W * H, "too many borderline pixels for this fixture"
    dLm = dL.to(dt) * (~borderline).to(dt)[None]
    per_pixel_loss = (color * dLm).sum(0).reshape(-1)                       # [N]: the loss term of every pixel
    N = per_pixel_loss.numel()
    g, = torch.autograd.grad(per_pixel_loss, aux["means2D"], grad_outputs=torch.eye(N, dtype=dt), is_grads_batched=True)
    unit = torch.tensor([0.5 * W, 0.5 * H], dtype=dt)                       # pixel units -> the op's (App. A.3)
    return dict(absgrad=(g.abs().sum(0) * unit).numpy(), grad=(g.sum(0) * unit).numpy(),
                borderline=borderline.numpy(), visible=(radii > 0).numpy())


if __name__ == "__main__":
    out = compute()
    np.savez(PATH, **out)
    a, g, vis = out["absgrad"], out["grad"], out["visible"]
    print(f"visible {int(vis.sum())}  borderline pixels {int(out['borderline'].sum())}  sum|absgrad| {np.abs(a).sum():.4g}  "
          f"sum|grad| {np.abs(g).sum():.4g}  rows with absgrad > 1.5 |grad|: "
          f"{int(((np.linalg.norm(a, axis=1) > 1.5 * np.linalg.norm(g, axis=1)) & vis).sum())}")
