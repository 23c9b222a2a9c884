"""Generates tests/golden/distortion_truth.npz: the float64 truth of the depth-distortion map (DESIGN.md SPEC M13) and of its
gradients on two scenes, independent of the op:
    python tests/golden/make_distortion_golden.py        (CPU only, a few seconds)

    Dist_p = 2 sum_{j<i} w_ip w_jp (z_i - z_j),    w_ip = alpha_ip T_ip,    i = 1..n in tile-list order (front to back)

The per-pixel weights come from oracle/torch_oracle.preprocess with the blend loop of torch_oracle.rasterize restated in
tests/replay_truth.py (the same alpha expression, validity, termination and borderline flags, and a zero means2D leaf added to
the pixel centres): rasterize returns sums over the weights, not the weights.  tests/test_distortion_cpu.py pins the restated loop to rasterize (its sum w,
sum w z, counted pairs and borderline mask against 1 - final_T, the depth map, n_blended and the oracle's mask) and this file to
compute().  All gradients are autograd's of sum G * Dist; G is seeded, uniform in (-0.5, 0.5), and zero on the oracle's borderline
pixels, where the test leaves the map out of the comparison too.

Two scenes, both small_scene(200, 40, 24, seed=1) with the front camera: scene F as it is, and "far": every Gaussian with
z > 0.3 moved to z + 2000 with x, y and the scales multiplied by (z + 2000) / z, computed and stored in float32 — the same
picture from 2000 units away, where the float32 moments of the unshifted formulas cancel."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

W, H, P, SCENE_SEED, G_SEED, FAR = 40, 24, 200, 1, 131, 2000.0
PLAIN = dict(filter_small=False, filter_large=False, fade_size=1.0)
import replay_truth as rt                        # noqa: E402  (tests/ is on the path now)
from replay_truth import MAX_BORDERLINE, TILE, distortion_of, pixel_weights      # noqa: E402,F401  (the loop and the definition)

PATH = os.path.join(HERE, "distortion_truth.npz")
SCENES = ("F", "far")


def scene(kind):
    """(scene, camera): scene F, or its copy pushed FAR units down the view axis (float32 arithmetic throughout)"""
    from parity_utils import small_scene
    sc, cam = small_scene(P, W, H, seed=SCENE_SEED)
    if kind == "far":
        m, s = sc.means3D.clone(), sc.scales.clone()
        z = m[:, 2].clone()
        sel = z > 0.3
        f = (z + torch.tensor(FAR, dtype=torch.float32)) / z
        m[sel, 0], m[sel, 1], m[sel, 2] = (m[:, 0] * f)[sel], (m[:, 1] * f)[sel], (z + torch.tensor(FAR, dtype=torch.float32))[sel]
        s[sel] = (s * f[:, None])[sel]
        assert m.dtype == torch.float32 and s.dtype == torch.float32
        sc.means3D, sc.scales = m, s
    return sc, cam


def seed_map():
    """G = dL/dDist [H,W] float32, seeded, uniform in (-0.5, 0.5)"""
    return torch.rand(H, W, generator=torch.Generator().manual_seed(G_SEED)) - 0.5


def restated(kind, leaves=None, view_edit=None):
    """the restated loop over the whole image (tests/replay_truth.render): dict of dist [H,W] (differentiable), wsum, wzsum [H,W],
    count [H,W] int64, borderline [H,W] bool, radii [P], the leaves (means3D, opacities, scales, rotations, means2D), per-tile
    lists.  view_edit(view): edits the oracle's view dict first (float64 camera leaves for the camera gradient)"""
    sc, cam = scene(kind)
    given = dict(zip(("means3D", "opacities", "scales", "rotations"), leaves)) if leaves else None
    r = rt.render(sc, cam, PLAIN, leaves=given, view_edit=view_edit)
    L = r.leaves
    tiles = [(x0, x1, y0, y1, wgt, r.pre["depth"][sel].detach()) for (x0, x1, y0, y1, sel, wgt, _) in r.tiles]
    return dict(dist=r.distortion, wsum=r.alpha.detach(), wzsum=r.depth.detach(), count=r.n_blended, borderline=r.borderline,
                radii=r.radii, leaves=(L["means3D"], L["opacities"], L["scales"], L["rotations"], L["means2D"]), tiles=tiles,
                view=r.view, scene=sc)


def compute_scene(kind):
    r = restated(kind)
    bl = r["borderline"]
    assert bl.sum().item() <= MAX_BORDERLINE * W * H, "too many borderline pixels for this fixture"
    G = seed_map() * (~bl).to(torch.float32)
    (r["dist"] * G.to(torch.float64)).sum().backward()
    means3D, opac, scales, rots, means2D = r["leaves"]
    m2 = torch.zeros(P, 3, dtype=torch.float64)
    m2[:, 0], m2[:, 1] = means2D.grad[:, 0] * 0.5 * W, means2D.grad[:, 1] * 0.5 * H      # -> the op's units (App. A.3)
    return dict(G=G.numpy(), map=r["dist"].detach().numpy(), means3D=means3D.grad.numpy(), opacities=opac.grad.numpy(),
                scales=scales.grad.numpy(), rotations=rots.grad.numpy(), means2D=m2.numpy(), borderline=bl.numpy(),
                visible=(r["radii"] > 0).numpy(), count=r["count"].numpy())


def compute():
    """dict, per scene S in SCENES: S_G [H,W] f32 (zero on borderline pixels), S_map [H,W] f64, the geometry gradients S_means3D
    [P,3], S_opacities [P,1], S_scales [P,3], S_rotations [P,4], S_means2D [P,3] (op units) f64, S_borderline [H,W] bool,
    S_visible [P] bool, S_count [H,W] int64 (counted pairs)"""
    out = {}
    for kind in SCENES:
        for k, v in compute_scene(kind).items():
            out[f"{kind}_{k}"] = v
    return out


if __name__ == "__main__":
    out = compute()
    np.savez(PATH, **out)
    for kind in SCENES:
        g = lambda k: out[f"{kind}_{k}"]
        print(f"{kind}: visible {int(g('visible').sum())}  borderline pixels {int(g('borderline').sum())} of {W * H}  "
              f"min counted pairs {int(g('count').min())}  Dist {g('map').min():.4g} .. {g('map').max():.4g}  "
              f"Gaussians with a z gradient {int((g('means3D')[:, 2] != 0).sum())}  max |means3D grad| {np.abs(g('means3D')).max():.4g}")
