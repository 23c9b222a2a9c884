"""Generates tests/golden/median_depth_truth.npz: the float64 truth of the median-depth and Gaussian-id maps (DESIGN.md SPEC M15)
and of the map's gradients on two scenes, independent of the op:
    python tests/golden/make_median_depth_golden.py        (CPU only, a few seconds)

Over the blended entries i = 1..n of a pixel in tile-list order, T_1 = 1, T_{i+1} = T_i (1 - alpha_i):
    m(p)         = the LAST blended entry with T_i > 0.5 (the 2DGS / gsplat rule)
    median_id    = the model row of entry m(p), -1 where nothing was blended
    median_depth = its view depth, 0 where nothing was blended;  d median_depth / dz_i = [i = m(p)], nothing through the selection

The per-pixel weights come from oracle/torch_oracle.preprocess and the blend loop of torch_oracle.rasterize as
make_distortion_golden.pixel_weights restates it (tests/test_distortion_cpu.py pins that loop to rasterize); it is imported, not
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
import importlib.util
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
NEAR = 1e-4                    # |T_{i+1} - 0.5| below which the selection is left out of the comparison
MAX_MASKED = 0.02              # of the image's pixels
PATH = os.path.join(HERE, "median_depth_truth.npz")
SCENES = ("F", "thin")
TILE = 16


def _distortion_generator():
    spec = importlib.util.spec_from_file_location("make_distortion_golden", os.path.join(HERE, "make_distortion_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    assert (m.W, m.H, m.TILE) == (W, H, TILE)          # pixel_weights reads its module's image size
    return m


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


def median_of(wgt, blended):
    """the definition on one tile: wgt [n, npix] float64 (alpha T of the blended pairs, 0 elsewhere), blended [n, npix] bool, in
    list order.  Returns (m [npix] list position of the median entry or -1, crossed [npix] bool: some blend took T to <= 0.5,
    near [npix] bool: some blended entry leaves T within NEAR of 0.5)"""
    w = wgt.detach()
    T_before = 1.0 - (torch.cumsum(w, 0) - w)
    T_after = T_before - w
    cand = blended & (T_before > 0.5)
    idx = torch.arange(w.shape[0])[:, None].expand_as(cand)
    m = torch.where(cand, idx, torch.full_like(idx, -1)).max(0).values
    crossed = (blended & (T_after <= 0.5)).any(0)
    near = (blended & ((T_after - 0.5).abs() < NEAR)).any(0)
    return m, crossed, near


def restated(kind, view_edit=None):
    """the maps over the whole image: dict of depth [H,W] float64 (differentiable), id [H,W] int32, count [H,W] (blended entries),
    crossed, near, borderline [H,W] bool, pos [H,W] (list position of the median entry, -1: none), radii [P], the means3D leaf.
    view_edit(view): edits the oracle's view dict first (a float64 viewmatrix leaf for the camera gradient)"""
    from oracle import torch_oracle as to
    dd = _distortion_generator()
    sc, cam = scene(kind)
    dt = torch.float64
    P = sc.means3D.shape[0]
    means3D = sc.means3D.detach().to(dt).clone().requires_grad_(True)
    view = to.view_dict(cam, sh_degree=sc.sh_degree, **PLAIN)
    if view_edit is not None:
        view_edit(view)
    pre = to.preprocess(means3D, sc.opacities.to(dt), view, scales=sc.scales.to(dt), rotations=sc.rotations.to(dt), shs=sc.shs,
                        max_pixel_sizes=sc.max_pixel_sizes, min_pixel_sizes=sc.min_pixel_sizes, base_mask=sc.base_mask)
    means2D = torch.zeros(P, 2, dtype=dt)
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    ids = torch.full((H, W), -1, dtype=torch.int32)
    pos = torch.full((H, W), -1, dtype=torch.int64)
    count = torch.zeros(H, W, dtype=torch.int64)
    maps = {k: torch.zeros(H, W, dtype=torch.bool) for k in ("crossed", "near", "borderline")}
    rows = []
    for ty in range(gy):
        parts = []
        for tx in range(gx):
            r = dd.pixel_weights(pre, means2D, tx, ty)
            x0, y0 = tx * TILE, ty * TILE
            x1, y1 = min(x0 + TILE, W), min(y0 + TILE, H)
            shape = (y1 - y0, x1 - x0)
            if r is None:
                parts.append(torch.zeros(shape, dtype=dt))
                continue
            sel, wgt, blended, bl, _ = r
            m, crossed, near = median_of(wgt, blended)
            has = m >= 0
            mc = m.clamp_min(0)
            z = pre["depth"][sel]
            parts.append(torch.where(has, z[mc], torch.zeros_like(z[mc])).view(shape))
            ids[y0:y1, x0:x1] = torch.where(has, sel[mc], torch.full_like(mc, -1)).to(torch.int32).view(shape)
            pos[y0:y1, x0:x1] = m.view(shape)
            count[y0:y1, x0:x1] = blended.sum(0).view(shape)
            for k, v in (("crossed", crossed), ("near", near), ("borderline", bl)):
                maps[k][y0:y1, x0:x1] = v.view(shape)
        rows.append(torch.cat(parts, dim=1))
    return dict(depth=torch.cat(rows, dim=0), id=ids, pos=pos, count=count, radii=pre["radii"], means3D=means3D, view=view,
                scene=sc, **maps)


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
