"""Generates tests/golden/median_depth_truth.npz: the float64 truth of the median-depth and Gaussian-id maps (DESIGN.md SPEC M15)
and of the map's gradients on two scenes, independent of the op:
    python tests/golden/make_median_depth_golden.py        (CPU only, a few seconds)

Over the blended entries i = 1..n of a pixel in tile-list order, T_1 = 1, T_{i+1} = T_i (1 - alpha_i):
    m(p)         = the LAST blended entry with T_i > 0.5 (the 2DGS / gsplat rule)
    median_id    = the model row of entry m(p), -1 where nothing was blended
    median_depth = its view depth, 0 where nothing was blended;  d median_depth / dz_i = [i = m(p)], nothing through the selection

The per-pixel weights come from oracle/torch_oracle.preprocess and the blend loop of torch_oracle.rasterize as
tests/replay_truth.pixel_weights restates it (tests/test_distortion_cpu.py pins that loop to rasterize); it is imported, not
restated again.  T_i = 1 - sum_{j<i} w_j of its float64 weights.  The gradients are autograd's of sum G * median_depth, with
median_depth gathered from the oracle's differentiable view depth at the selected entry, for a float64 means3D leaf and a
float64 viewmatrix leaf.

Two scenes with the front camera, 40 x 24:
    F     small_scene(200, 40, 24, seed=1): every pixel crosses 1/2
    thin  small_scene(20, 40, 24, seed=3) with opacities * 0.35 (float32): 323 empty pixels, 8 crossing, 629 never crossing

mask: the oracle's borderline pixels together with the pixels where some blended entry has |T_{i+1} - 0.5| < NEAR = 1e-4 — about
four times a worst-case linear float32 rounding of a 200-factor product (one ulp, 2^-23, per factor for the alpha and the fma:
200 * 2^-23 = 2.4e-5) — where float32 may legitimately select the neighbouring entry.  G is seeded, uniform in (-0.5, 0.5),
and zero on the mask; the mask must cover <= 2 % of the image (asserted here and in the tests)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

W, H, G_SEED = 40, 24, 151
PLAIN = dict(filter_small=False, filter_large=False, fade_size=1.0)
import replay_truth as rt                        # noqa: E402  (tests/ is on the path now)
from replay_truth import NEAR, TILE, median_of   # noqa: E402,F401  (|T_{i+1} - 0.5| < NEAR: left out of the comparison)

MAX_MASKED = rt.MAX_BORDERLINE                   # of the image's pixels
PATH = os.path.join(HERE, "median_depth_truth.npz")
SCENES = ("F", "thin")


def scene(kind):
    """(scene, camera)"""
    from parity_utils import small_scene
    if kind == "F":
        return small_scene(200, W, H, seed=1)
    sc, cam = small_scene(20, W, H, seed=3)
    sc.opacities = sc.opacities * torch.tensor(0.35, dtype=torch.float32)
    assert sc.opacities.dtype == torch.float32
    return sc, cam


def seed_map():
    """G = dL/dmedian_depth [H,W] float32, seeded, uniform in (-0.5, 0.5)"""
    return torch.rand(H, W, generator=torch.Generator().manual_seed(G_SEED)) - 0.5


def restated(kind, view_edit=None):
    """the maps over the whole image (tests/replay_truth.render): dict of depth [H,W] float64 (differentiable), id [H,W] int32,
    count [H,W] (blended entries), crossed, near, borderline [H,W] bool, pos [H,W] (list position of the median entry, -1: none),
    radii [P], the means3D leaf.  view_edit(view): edits the oracle's view dict first (a float64 viewmatrix leaf for the camera
    gradient)"""
    sc, cam = scene(kind)
    r = rt.render(sc, cam, PLAIN, view_edit=view_edit)
    return dict(depth=r.median_depth, id=r.median_id, pos=r.median_pos, count=r.n_blended, radii=r.radii,
                means3D=r.leaves["means3D"], view=r.view, scene=sc, crossed=r.crossed, near=r.near, borderline=r.borderline)


def compute_scene(kind):
    leaves = {}

    def edit(view):
        leaves["V"] = view["viewmatrix"].to(torch.float64).clone().requires_grad_(True)
        view["viewmatrix"] = leaves["V"]
    r = restated(kind, view_edit=edit)
    mask = r["borderline"] | r["near"]
    assert mask.sum().item() <= MAX_MASKED * W * H, "too many masked pixels for this fixture"
    G = seed_map() * (~mask).to(torch.float32)
    (r["depth"] * G.to(torch.float64)).sum().backward()
    return dict(G=G.numpy(), depth=r["depth"].detach().numpy(), id=r["id"].numpy(), means3D=r["means3D"].grad.numpy(),
                viewmatrix=leaves["V"].grad.numpy(), mask=mask.numpy(), borderline=r["borderline"].numpy(), near=r["near"].numpy(),
                visible=(r["radii"] > 0).numpy(), count=r["count"].numpy(), crossed=r["crossed"].numpy(), pos=r["pos"].numpy())


def compute():
    """dict, per scene S in SCENES: S_G [H,W] f32 (zero on the mask), S_depth [H,W] f64, S_id [H,W] i32, the gradients S_means3D
    [P,3] and S_viewmatrix [4,4] f64, S_mask = S_borderline | S_near [H,W] bool, S_visible [P] bool, S_count [H,W] i64 (blended
    entries), S_crossed [H,W] bool, S_pos [H,W] i64 (list position of the median entry)"""
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
        empty, crossed = g("count") == 0, g("crossed")
        print(f"{kind}: visible {int(g('visible').sum())}  empty {int(empty.sum())}  crossing {int(crossed.sum())}  never crossing "
              f"{int((~empty & ~crossed).sum())}  masked: borderline {int(g('borderline').sum())} + near "
              f"{int((g('near') & ~g('borderline')).sum())} of {W * H}  median position {g('pos')[~empty].min()} .. {g('pos').max()}  "
              f"depth {g('depth')[~empty].min():.4g} .. {g('depth').max():.4g}  distinct ids {len(np.unique(g('id')))}  "
              f"max |means3D grad| {np.abs(g('means3D')).max():.4g}  max |viewmatrix grad| {np.abs(g('viewmatrix')).max():.4g}")
