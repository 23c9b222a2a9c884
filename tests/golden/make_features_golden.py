"""Generates tests/golden/features_truth.npz: the float64 truth of the feature-channel render (DESIGN.md SPEC M12) on scene F,
independent of the op:
    python tests/golden/make_features_golden.py        (CPU only, a few seconds)

oracle/torch_oracle.rasterize blends `colors_precomp` triples; over a zero background a colour channel IS a feature channel,
F[c,p] = sum_i f_ic w_ip.  C = 5 seeded features in [0, 1] go through it as the triples (0, 1, 2) and (3, 4, zeros), in float64,
and autograd of sum G * F gives dL/dfeatures and the geometry gradients (means3D, opacities, scales, rotations; means2D from
the oracle's pixel-unit leaf, scaled to the op's units).  Pixels the oracle flags as borderline (an alpha or a transmittance
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
MAX_BORDERLINE = 0.02          # of the image's pixels (the cap of make_absgrad_golden.py)
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
    from oracle import torch_oracle as to
    sc, cam = scene_f()
    dt = torch.float64
    leaf = lambda t: t.detach().to(dt).clone().requires_grad_(True)
    means3D, opac, scales, rots, f = leaf(sc.means3D), leaf(sc.opacities), leaf(sc.scales), leaf(sc.rotations), leaf(features())
    view = to.view_dict(cam, sh_degree=sc.sh_degree, **PLAIN)
    maps, m2_leaves, borderline, radii = [], [], None, None
    for c0 in range(0, C, 3):
        triple = f[:, c0:c0 + 3]
        if triple.shape[1] < 3:
            triple = torch.cat([triple, torch.zeros(P, 3 - triple.shape[1], dtype=dt)], 1)
        color, _, _, radii, _, aux = to.rasterize(means3D, opac, view, torch.zeros(3, dtype=dt), scales=scales, rotations=rots,
                                                  colors_precomp=triple, max_pixel_sizes=sc.max_pixel_sizes,
                                                  min_pixel_sizes=sc.min_pixel_sizes, base_mask=sc.base_mask)
        maps.append(color[:min(3, C - c0)])
        m2_leaves.append(aux["means2D"])
        assert borderline is None or torch.equal(borderline, aux["borderline"])      # a property of the geometry alone
        borderline = aux["borderline"]
    fmap = torch.cat(maps, 0)
    assert borderline.sum().item() <= MAX_BORDERLINE * W * H, "too many borderline pixels for this fixture"
    G = seed_map() * (~borderline).to(torch.float32)[None]
    (fmap * G.to(dt)).sum().backward()
    g2 = sum(m.grad for m in m2_leaves)                                            # pixel units, [P,2]
    m2 = torch.zeros(P, 3, dtype=dt)
    m2[:, 0], m2[:, 1] = g2[:, 0] * 0.5 * W, g2[:, 1] * 0.5 * H                    # -> the op's units (App. A.3)
    return dict(features=features().numpy(), G=G.numpy(), map=fmap.detach().numpy(), dfeatures=f.grad.numpy(),
                means3D=means3D.grad.numpy(), opacities=opac.grad.numpy(), scales=scales.grad.numpy(),
                rotations=rots.grad.numpy(), means2D=m2.numpy(), borderline=borderline.numpy(), visible=(radii > 0).numpy())


if __name__ == "__main__":
    out = compute()
    np.savez(PATH, **out)
    print(f"visible {int(out['visible'].sum())}  borderline pixels {int(out['borderline'].sum())} of {W * H}  "
          f"max |map| {np.abs(out['map']).max():.4g}  pixels with a zero map {(np.abs(out['map']).sum(0) == 0).sum()}  "
          f"max |dfeatures| {np.abs(out['dfeatures']).max():.4g}  max |means3D grad| {np.abs(out['means3D']).max():.4g}")
