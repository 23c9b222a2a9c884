"""Generates tests/golden/distortion_truth.npz: the float64 truth of the depth-distortion map (DESIGN.md SPEC M13) and of its
gradients on two scenes, independent of the op:
    python tests/golden/make_distortion_golden.py        (CPU only, a few seconds)

    Dist_p = 2 sum_{j<i} w_ip w_jp (z_i - z_j),    w_ip = alpha_ip T_ip,    i = 1..n in tile-list order (front to back)

The per-pixel weights come from oracle/torch_oracle.preprocess with the blend loop of torch_oracle.rasterize restated (the same
alpha expression, validity, termination and borderline flags, and a zero means2D leaf added to the pixel centres): rasterize
returns sums over the weights, not the weights.  tests/test_distortion_cpu.py pins the restated loop to rasterize (its sum w,
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
MAX_BORDERLINE = 0.02          # of the image's pixels (the cap of make_absgrad_golden.py)
PATH = os.path.join(HERE, "distortion_truth.npz")
SCENES = ("F", "far")
TILE = 16


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


def pixel_weights(pre, means2D, tx, ty):
    """torch_oracle.rasterize's blend loop of tile (tx, ty), restated: (sel [n] Gaussian ids in list order, wgt [n, npix] float64
    = alpha T of the blended pairs and 0 elsewhere, blended [n, npix] bool, borderline [npix] bool, (x0, x1, y0, y1)); None for a
    tile with an empty list"""
    dt = torch.float64
    px, py = pre["px"] + means2D[:, 0], pre["py"] + means2D[:, 1]
    vis = pre["visible"]
    rminx, rminy, rmaxx, rmaxy = pre["rect"]
    order_all = torch.argsort(pre["depth32"], stable=True)
    vs = order_all[vis[order_all]]
    sel = vs[(rminx[vs] <= tx) & (tx < rmaxx[vs]) & (rminy[vs] <= ty) & (ty < rmaxy[vs])]
    x0, y0 = tx * TILE, ty * TILE
    x1, y1 = min(x0 + TILE, W), min(y0 + TILE, H)
    if sel.numel() == 0:
        return None
    ys, xs = torch.meshgrid(torch.arange(y0, y1, dtype=dt), torch.arange(x0, x1, dtype=dt), indexing="ij")
    npix = ys.numel()
    xs, ys = xs.reshape(-1), ys.reshape(-1)
    dx = px[sel][:, None] - xs[None, :]
    dy = py[sel][:, None] - ys[None, :]
    con = pre["conic"][sel]
    power = -0.5 * (con[:, 0:1] * dx * dx + con[:, 2:3] * dy * dy) - con[:, 1:2] * dx * dy
    Gs = torch.exp(torch.clamp(power, max=0.0))
    a_raw = pre["opacity"][sel][:, None] * Gs
    alpha = a_raw + (torch.clamp(a_raw, max=0.99) - a_raw).detach()
    valid = (power <= 0) & (alpha.detach() >= 1.0 / 255.0)
    near = (power.detach() <= 0) & ((alpha.detach() - 1.0 / 255.0).abs() < 2e-6)
    alpha_v = torch.where(valid, alpha, torch.zeros_like(alpha))
    one_m = 1.0 - alpha_v
    T_after = torch.cumprod(one_m, dim=0)
    T_before = torch.cat([torch.ones(1, npix, dtype=dt), T_after[:-1]], dim=0)
    fail = valid & (T_after.detach() < 1e-4)
    near_t = valid & ((T_after.detach() - 1e-4).abs() < 1e-9)
    any_fail = fail.any(dim=0)
    first_fail = torch.where(any_fail, fail.to(torch.int64).argmax(dim=0), torch.full((npix,), sel.numel(), dtype=torch.int64))
    idx = torch.arange(sel.numel())[:, None]
    blended = valid & (idx < first_fail[None, :])
    bl = ((near | near_t) & (idx <= first_fail[None, :])).any(dim=0)
    wgt = torch.where(blended, alpha * T_before, torch.zeros_like(alpha))
    return sel, wgt, blended, bl, (x0, x1, y0, y1)


def distortion_of(wgt, z):
    """the definition: 2 sum_{j<i} w_i w_j (z_i - z_j) per pixel; wgt [n, npix], z [n] in list order.  With prefix sums
    A_i = sum_{j<i} w_j and Z_i = sum_{j<i} w_j z_j it is 2 sum_i w_i (z_i A_i - Z_i)."""
    wz = wgt * z[:, None]
    A = torch.cumsum(wgt, 0) - wgt
    Z = torch.cumsum(wz, 0) - wz
    return 2.0 * (wgt * (z[:, None] * A - Z)).sum(0)


def restated(kind, leaves=None, view_edit=None):
    """the restated loop over the whole image: dict of dist [H,W] (differentiable), wsum, wzsum [H,W], count [H,W] int64,
    borderline [H,W] bool, radii [P], the leaves (means3D, opacities, scales, rotations, means2D), per-tile lists.
    view_edit(view): edits the oracle's view dict first (float64 camera leaves for the camera gradient)"""
    from oracle import torch_oracle as to
    sc, cam = scene(kind)
    dt = torch.float64
    leaf = lambda t: t.detach().to(dt).clone().requires_grad_(True)
    means3D, opac, scales, rots = leaves or (leaf(sc.means3D), leaf(sc.opacities), leaf(sc.scales), leaf(sc.rotations))
    view = to.view_dict(cam, sh_degree=sc.sh_degree, **PLAIN)
    if view_edit is not None:
        view_edit(view)
    pre = to.preprocess(means3D, opac, view, scales=scales, rotations=rots, shs=sc.shs, max_pixel_sizes=sc.max_pixel_sizes,
                        min_pixel_sizes=sc.min_pixel_sizes, base_mask=sc.base_mask)
    means2D = torch.zeros(P, 2, dtype=dt, requires_grad=True)
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    dist = torch.zeros(H, W, dtype=dt)
    wsum, wzsum = torch.zeros(H, W, dtype=dt), torch.zeros(H, W, dtype=dt)
    count = torch.zeros(H, W, dtype=torch.int64)
    borderline = torch.zeros(H, W, dtype=torch.bool)
    tiles = []
    rows = []
    for ty in range(gy):
        parts = []
        for tx in range(gx):
            r = pixel_weights(pre, means2D, tx, ty)
            x0, y0 = tx * TILE, ty * TILE
            x1, y1 = min(x0 + TILE, W), min(y0 + TILE, H)
            if r is None:
                parts.append(torch.zeros(y1 - y0, x1 - x0, dtype=dt))
                continue
            sel, wgt, blended, bl, _ = r
            z = pre["depth"][sel]
            parts.append(distortion_of(wgt, z).view(y1 - y0, x1 - x0))
            wsum[y0:y1, x0:x1] = wgt.detach().sum(0).view(y1 - y0, x1 - x0)
            wzsum[y0:y1, x0:x1] = (wgt.detach() * z.detach()[:, None]).sum(0).view(y1 - y0, x1 - x0)
            count[y0:y1, x0:x1] = blended.sum(0).view(y1 - y0, x1 - x0)
            borderline[y0:y1, x0:x1] = bl.view(y1 - y0, x1 - x0)
            tiles.append((x0, x1, y0, y1, wgt.detach(), z.detach()))
        rows.append(torch.cat(parts, dim=1))
    dist = torch.cat(rows, dim=0)
    return dict(dist=dist, wsum=wsum, wzsum=wzsum, count=count, borderline=borderline, radii=pre["radii"],
                leaves=(means3D, opac, scales, rots, means2D), tiles=tiles, view=view, scene=sc)


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
