"""One float64 restatement of the blend loop for every opt-in output of the tile-list replays (DESIGN.md SPEC M10-M13, M15): the
alpha map, absgrad, contribution scores, feature channels, depth distortion, median depth / id — with the scene, the camera and the
settings as ARGUMENTS, so that the same truth serves the committed fixtures (tests/golden/make_{absgrad,contrib,features,
distortion,median_depth}_golden.py import it) and the seeded sweep (tests/replay_cases.py, tests/test_replay_sweep_{cpu,gpu}.py).

The per-Gaussian stage is oracle/torch_oracle.preprocess; the blend loop of torch_oracle.rasterize is restated in pixel_weights
(the same alpha expression, validity, termination and borderline flags, a zero means2D leaf added to the pixel centres), because
rasterize returns sums over the weights w_ip = alpha_ip T_ip and the replays need the weights.  tests/test_replay_sweep_cpu.py pins
the restated loop to rasterize on every case of the sweep (colour, depth, 1 - final_T, n_blended, radii, borderline mask).

    render(scene, camera, ...)      every map, differentiable, plus the discrete maps and the per-tile lists
    gradients(r, seeds)             autograd of sum(seed * map) in the form parity_utils.leaf_space / check_backward accept
    contributions(r, m)             per-Gaussian sum / max / count of m_p w_ip
dtype=torch.float32 evaluates the same code in float32: the reference's own float32 distance from its float64 result is the
allowance of the project's three-way rule (parity_utils.TRUTH_FACTOR) and is never measured on the code under test."""
import types

import torch

from oracle import torch_oracle as to

TILE = to.TILE
NEAR = 1e-4                    # |T_{i+1} - 0.5| below which the median selection is left out of a comparison
MAX_BORDERLINE = 0.02          # of the image's pixels: the cap of every fixture generator
PLAIN = dict(filter_small=False, filter_large=False, fade_size=1.0)
MAPS = ("color", "depth", "alpha", "distortion", "median_depth", "features")
ABSGRAD_TERMS = ("color", "depth", "alpha")         # the loss terms msgs_absgrad is handed (dL, dLd, dLa)


def pixel_weights(pre, means2D, tx, ty, W, H, offsets=None):
    """torch_oracle.rasterize's blend loop of tile (tx, ty), restated: (sel [n] Gaussian ids in list order, wgt [n, npix]
    = alpha T of the blended pairs and 0 elsewhere, blended [n, npix] bool, borderline [npix] bool, (x0, x1, y0, y1), terminated
    [npix] bool: an entry was refused because it would have taken T below 1e-4); None for a tile with an empty list.  offsets(n, npix) -> [n, npix, 2] zeros that are added to the pixel-centre distances: a leaf per
    (entry, pixel), whose gradient is the pixel's own share of dL/dmeans2D (absgrad)"""
    dt = pre["conic"].dtype
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
    if offsets is not None:
        off = offsets(sel.numel(), npix)
        dx, dy = dx + off[..., 0], dy + off[..., 1]
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
    return sel, wgt, blended, bl, (x0, x1, y0, y1), any_fail


def distortion_of(wgt, z):
    """the definition: 2 sum_{j<i} w_i w_j (z_i - z_j) per pixel; wgt [n, npix], z [n] in list order.  With prefix sums
    A_i = sum_{j<i} w_j and Z_i = sum_{j<i} w_j z_j it is 2 sum_i w_i (z_i A_i - Z_i)."""
    wz = wgt * z[:, None]
    A = torch.cumsum(wgt, 0) - wgt
    Z = torch.cumsum(wz, 0) - wz
    return 2.0 * (wgt * (z[:, None] * A - Z)).sum(0)


def median_of(wgt, blended, near_tol=NEAR):
    """the definition on one tile: wgt [n, npix] (alpha T of the blended pairs, 0 elsewhere), blended [n, npix] bool, in list
    order.  Returns (m [npix] list position of the median entry or -1, crossed [npix] bool: some blend took T to <= 0.5,
    near [npix] bool: some blended entry leaves T within near_tol of 0.5)"""
    w = wgt.detach()
    T_before = 1.0 - (torch.cumsum(w, 0) - w)
    T_after = T_before - w
    cand = blended & (T_before > 0.5)
    idx = torch.arange(w.shape[0])[:, None].expand_as(cand)
    m = torch.where(cand, idx, torch.full_like(idx, -1)).max(0).values
    crossed = (blended & (T_after <= 0.5)).any(0)
    near = (blended & ((T_after - 0.5).abs() < near_tol)).any(0)
    return m, crossed, near


def render(sc, cam, settings=PLAIN, scaling_modifier=1.0, bg=None, features=None, view_edit=None, dtype=torch.float64,
           cov3D_precomp=False, leaves=None, per_pixel=False):
    """The restated loop over the whole image.  sc, cam: a scenes.Scene and its camera; settings: filter_small / filter_large /
    fade_size; bg [3] (zeros when None); features [P, C] or None; view_edit(view) edits the oracle's view dict first (camera
    leaves); cov3D_precomp: the covariance is built from the scale / rotation leaves and handed to the oracle's cov3D_precomp
    entry; leaves: {name: tensor} that replace the module's own leaves (means3D, opacities, scales, rotations, shs, features);
    per_pixel: keep a zero leaf per (entry, pixel) for gradients(..., absgrad=True).

    Returns a namespace: color [3,H,W], depth, alpha, distortion, median_depth [H,W], features [C,H,W] or None (differentiable,
    `dtype`); median_id [H,W] int32 (-1: nothing blended), median_pos [H,W] int64 (list position of the median entry), n_blended
    [H,W] int64, final_T [H,W], borderline, near, crossed, terminated [H,W] bool, radii [P] int32, leaves, view, pre, W, H, P and tiles =
    [(x0, x1, y0, y1, sel, wgt (detached), blended)] of the tiles with a list."""
    dt = dtype
    W, H, P = int(cam.image_width), int(cam.image_height), sc.means3D.shape[0]
    leaf = lambda t: t.detach().to(dt).clone().requires_grad_(True)
    L = dict(leaves or {})
    for k, src in (("means3D", sc.means3D), ("opacities", sc.opacities), ("scales", sc.scales), ("rotations", sc.rotations),
                   ("shs", sc.shs)):
        if k not in L:
            L[k] = leaf(src)
    if features is not None and "features" not in L:
        L["features"] = leaf(features)
    view = to.view_dict(cam, sh_degree=sc.sh_degree, scale_modifier=float(scaling_modifier), **settings)
    if view_edit is not None:
        view_edit(view)
    kw = dict(shs=L["shs"], max_pixel_sizes=sc.max_pixel_sizes, min_pixel_sizes=sc.min_pixel_sizes, base_mask=sc.base_mask)
    if cov3D_precomp:
        kw["cov3D_precomp"] = to.cov3d_from_scale_rot(L["scales"].to(dt), L["rotations"].to(dt), float(scaling_modifier))
    else:
        kw["scales"], kw["rotations"] = L["scales"], L["rotations"]
    if dt != torch.float64:
        kw["dtype"] = dt
    pre = to.preprocess(L["means3D"], L["opacities"], view, **kw)
    means2D = torch.zeros(P, 2, dtype=dt, requires_grad=True)
    L["means2D"] = means2D
    bg = torch.zeros(3, dtype=dt) if bg is None else bg.to(dt)
    f = L.get("features")
    C = f.shape[1] if f is not None else 0
    offs = []

    def offsets(n, npix):
        offs.append(torch.zeros(n, npix, 2, dtype=dt, requires_grad=True))
        return offs[-1]

    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    flat = {k: [] for k in ("color", "depth", "alpha", "distortion", "median_depth", "features", "id", "pos", "count", "borderline",
                            "near", "crossed", "terminated", "pixel")}
    tiles = []
    for ty in range(gy):
        for tx in range(gx):
            r = pixel_weights(pre, means2D, tx, ty, W, H, offsets if per_pixel else None)
            x0, y0 = tx * TILE, ty * TILE
            x1, y1 = min(x0 + TILE, W), min(y0 + TILE, H)
            ys, xs = torch.meshgrid(torch.arange(y0, y1), torch.arange(x0, x1), indexing="ij")
            flat["pixel"].append((ys * W + xs).reshape(-1))
            npix = ys.numel()
            if r is None:
                flat["color"].append(bg[:, None].expand(3, npix).clone())
                for k in ("depth", "alpha", "distortion", "median_depth"):
                    flat[k].append(torch.zeros(npix, dtype=dt))
                flat["features"].append(torch.zeros(C, npix, dtype=dt))
                flat["id"].append(torch.full((npix,), -1, dtype=torch.int32))
                flat["pos"].append(torch.full((npix,), -1, dtype=torch.int64))
                flat["count"].append(torch.zeros(npix, dtype=torch.int64))
                for k in ("borderline", "near", "crossed", "terminated"):
                    flat[k].append(torch.zeros(npix, dtype=torch.bool))
                continue
            sel, wgt, blended, bl, _, ended = r
            z = pre["depth"][sel]
            alpha = wgt.sum(0)
            flat["color"].append((wgt[:, None, :] * pre["rgb"][sel][:, :, None]).sum(0) + (1.0 - alpha)[None, :] * bg[:, None])
            flat["depth"].append((wgt * z[:, None]).sum(0))
            flat["alpha"].append(alpha)
            flat["distortion"].append(distortion_of(wgt, z))
            m, crossed, near = median_of(wgt, blended)
            has = m >= 0
            mc = m.clamp_min(0)
            flat["median_depth"].append(torch.where(has, z[mc], torch.zeros_like(z[mc])))
            flat["features"].append((wgt[:, None, :] * f[sel][:, :, None]).sum(0) if C else torch.zeros(0, npix, dtype=dt))
            flat["id"].append(torch.where(has, sel[mc], torch.full_like(mc, -1)).to(torch.int32))
            flat["pos"].append(m)
            flat["count"].append(blended.sum(0))
            for k, v in (("borderline", bl), ("near", near), ("crossed", crossed), ("terminated", ended)):
                flat[k].append(v)
            tiles.append((x0, x1, y0, y1, sel, wgt.detach(), blended))
    inv = torch.empty(W * H, dtype=torch.int64)
    inv[torch.cat(flat["pixel"])] = torch.arange(W * H)
    image = lambda k: torch.cat(flat[k], dim=-1)[..., inv].reshape(*flat[k][0].shape[:-1], H, W)
    alpha = image("alpha")
    return types.SimpleNamespace(
        color=image("color"), depth=image("depth"), alpha=alpha, distortion=image("distortion"), median_depth=image("median_depth"),
        features=image("features") if C else None, median_id=image("id"), median_pos=image("pos"), n_blended=image("count"),
        final_T=1.0 - alpha.detach(), borderline=image("borderline"), near=image("near"), crossed=image("crossed"),
        terminated=image("terminated"),
        radii=pre["radii"], leaves=L, view=view, pre=pre, W=W, H=H, P=P, tiles=tiles, offsets=offs, dtype=dt)


GRAD_LEAVES = ("means3D", "opacities", "scales", "rotations", "shs", "features")


def gradients(r, seeds, absgrad=False, extra_leaves=None):
    """autograd's gradients of sum_k sum(seeds[k] * r.k) over any subset k of MAPS, with respect to means3D, opacities, scales,
    rotations, shs, features and the zero means2D leaf, the latter as [P, 3] in the op's units (pixel gradient x 0.5 W, 0.5 H;
    App. A.3): the dict parity_utils.leaf_space / check_backward take, plus "features" (dL/dfeatures) and every name of
    extra_leaves {name: leaf} (camera leaves of a view_edit).  absgrad=True (needs render(per_pixel=True)) adds "absgrad" and
    "absgrad_net" [P, 2], op units: the sum over pixels of the absolute value (resp. the plain sum) of each pixel's own share of
    dL/dmeans2D for the loss terms the op's absgrad is handed (ABSGRAD_TERMS: colour, depth, alpha)."""
    dt = r.dtype
    term = lambda k: (getattr(r, k) * seeds[k].to(dt)).sum()
    assert set(seeds) <= set(MAPS) and seeds
    loss = sum(term(k) for k in seeds)
    names = [k for k in GRAD_LEAVES if k in r.leaves] + ["means2D"]
    named = [r.leaves[k] for k in names] + list((extra_leaves or {}).values())
    gs = torch.autograd.grad(loss, named, allow_unused=True, retain_graph=True)
    out = {k: (g if g is not None else torch.zeros_like(l)) for k, l, g in zip(names + list(extra_leaves or {}), named, gs)}
    unit = torch.tensor([0.5 * r.W, 0.5 * r.H], dtype=dt)
    m2 = torch.zeros(r.P, 3, dtype=dt)
    m2[:, :2] = out["means2D"] * unit
    out["means2D"] = m2
    if absgrad:
        a, n = torch.zeros(r.P, 2, dtype=dt), torch.zeros(r.P, 2, dtype=dt)
        terms = [k for k in ABSGRAD_TERMS if k in seeds]
        if terms and r.offsets:
            assert len(r.offsets) == len(r.tiles), "render(per_pixel=True) is needed for absgrad"
            gs = torch.autograd.grad(sum(term(k) for k in terms), r.offsets, allow_unused=True, retain_graph=True)
            for t, g in zip(r.tiles, gs):
                if g is not None:
                    a.index_add_(0, t[4], g.abs().sum(1))
                    n.index_add_(0, t[4], g.sum(1))
        out["absgrad"], out["absgrad_net"] = a * unit, n * unit
    return out


def contributions(r, m):
    """per-Gaussian contribution scores for the pixel-weight map m [H,W] (>= 0): (sum_p m_p w_ip, max_p m_p w_ip [P] in r's
    dtype, the number of blended pairs with m_p > 0 [P] int64)"""
    dt = r.dtype
    m = m.to(dt)
    s, mx, cnt = torch.zeros(r.P, dtype=dt), torch.zeros(r.P, dtype=dt), torch.zeros(r.P, dtype=torch.int64)
    for x0, x1, y0, y1, sel, wgt, blended in r.tiles:
        mt = m[y0:y1, x0:x1].reshape(1, -1)
        t = wgt * mt
        s.index_add_(0, sel, t.sum(1))
        mx[sel] = torch.maximum(mx[sel], t.max(1).values)
        cnt.index_add_(0, sel, (blended & (mt > 0)).sum(1))
    return s, mx, cnt


def masks(r):
    """(borderline, borderline | near): what the seeds of every map, resp. of the median depth, are zeroed on"""
    return r.borderline, r.borderline | r.near
