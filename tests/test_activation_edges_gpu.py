"""The getters' activations at their edges (sigmoid / exp / F.normalize / the SH cat of the reference's GaussianModel), through
the three entries that evaluate or differentiate them: render() with the chained getters (torch forward, the kernel's
backward: raw mode 2), render() on the plain autograd path, and render_fused() (activations and their backward in the
kernels: raw mode 1).  Ordinary small scenes, with chosen rows' RAW leaves overwritten so that the edge rows share tiles with
ordinary ones; every leaf gradient against the float64 autograd oracle (oracle/torch_oracle.py) carried through float64
sigmoid / exp / normalize / cat (parity_utils.leaf_space).

Each edge row is also held to its OWN gradient magnitude: a clamped quaternion's gradient is ~1e12 and would hide every other
row of dL/drotation in a max-norm comparison, and the ordinary rows would hide a tiny edge row."""
import copy
import math

import numpy as np
import pytest
import torch

import scenes
from parity_utils import BWD_RTOL, NORMALIZE_EPS_F32, PIPE, check_forward, leaf_space, rel_err, report, small_scene

pytestmark = pytest.mark.gpu

W, H = 96, 64
P = 900
FOCAL = 1000.0 * W / 1920.0                     # front_camera's focal length in pixels
ST = dict(filter_small=False, filter_large=False, fade_size=1.0)
BG = torch.tensor([0.2, 0.1, 0.3])
ENTRIES = ("chained", "plain", "fused")
LEAF_OF = {"means3D": "_xyz", "features_dc": "_features_dc", "features_rest": "_features_rest", "opacity": "_opacity",
           "scaling": "_scaling", "rotation": "_rotation"}
# an edge row against its own gradient: ||d_i||_inf <= ROW_RTOL ||truth_i||_inf + BWD_RTOL x (the ordinary rows' max norm)
ROW_RTOL = 1e-3
HIP_VS_HIP_RTOL = 2e-6                          # tests/test_getter_chain_gpu.py
FLAGGED_EDGE_ROWS_MAX = 2                       # edge rows a legitimately flipped discrete decision may exclude, per case
EPS32 = NORMALIZE_EPS_F32                     # F.normalize's eps as the float32 model's clamp_min compares it
C0_F32 = np.float32(0.28209479177387814)


def _f32_below(x):
    return float(np.nextafter(np.float32(x), np.float32(-np.inf)))


def _dc_for(target):
    """features_dc value d with float32 (C0 * d) + 0.5 == target, searched among the floats next to -0.5 / C0"""
    d = np.float32(-0.5 / 0.28209479177387814)
    for _ in range(64):
        r = np.float32(np.float32(C0_F32 * d) + np.float32(0.5))
        if r == np.float32(target):
            return float(d)
        d = np.nextafter(d, np.float32(np.inf) if r < target else np.float32(-np.inf))     # C0 d grows with d
    raise AssertionError(f"no features_dc gives {target}")


def _at_pixels(sc, rows, z, seed):
    """moves `rows` inside the image at view depth z, (0.3, 0.2) px from a pixel centre (front camera: x = (px + 0.5 - W/2) z / f).
    Not ON the centre: there the exponent is 0 and its sign undecided in float32 (the oracle flags such a Gaussian)."""
    g = torch.Generator().manual_seed(seed)
    n = len(rows)
    px = torch.randint(6, W - 6, (n,), generator=g).float() + 0.3
    py = torch.randint(6, H - 6, (n,), generator=g).float() + 0.2
    z = torch.as_tensor(z, dtype=torch.float32).expand(n)
    sc.means3D[rows] = torch.stack([(px + 0.5 - W / 2) * z / FOCAL, (py + 0.5 - H / 2) * z / FOCAL, z], dim=1)


def _unit(g, n):
    q = torch.randn(n, 4, generator=g, dtype=torch.float64)
    return q / q.norm(dim=1, keepdim=True)


def _case(family):
    """(scene, {leaf: (rows, raw values)}, edge rows [long]) for one family"""
    deg = 0 if family.startswith("sh") else 3
    sc, cam = small_scene(P, W, H, 4100 + len(family), sh_degree=deg)
    sc = copy.copy(sc)
    sc.means3D = sc.means3D.clone()
    if family == "sh_built_deg0":
        sc.shs = sc.shs[:, :1].contiguous()
    g = torch.Generator().manual_seed(17 + len(family))
    edits = {}
    if family == "rotation":
        raws = []
        for n in (1e-13, 5e-13, 1e-9, 1e-3, 1.0, 1e3, 1e9):           # norms over the clamp and far from it
            raws += list(_unit(g, 2) * n)
        for n in (_f32_below(1e-12), EPS32):                          # one float32 ulp under the clamp, and exactly at it
            raws += [torch.tensor([n, 0.0, 0.0, 0.0], dtype=torch.float64), torch.tensor([0.0, 0.0, -n, 0.0], dtype=torch.float64)]
        raws.append(torch.zeros(4, dtype=torch.float64))              # the zero quaternion
        for n in (1.0, 3e-13):                                        # -q next to q
            q = _unit(g, 1)[0] * n
            raws += [q, -q]
        for n in (1.0, 1e3):                                          # one dominant component, the rest at 1e-8 of it
            raws += [torch.tensor([1.0, 1e-8, -1e-8, 1e-8], dtype=torch.float64) * n,
                     torch.tensor([1e-8, -1e-8, 1.0, 1e-8], dtype=torch.float64) * n]
        rows = torch.arange(len(raws))
        _at_pixels(sc, rows, 2.0 + 4.0 * torch.rand(len(rows), generator=g), 1)
        # visible, anisotropic (a rotation changes the footprint), a few pixels wide
        ls = torch.log(torch.tensor([4.0, 2.0, 1.0]) * 2.0 / FOCAL * sc.means3D[rows, 2:3])
        edits["_rotation"] = (rows, torch.stack(raws).float())
        edits["_scaling"] = (rows, ls)
        edits["_opacity"] = (rows, torch.full((len(rows), 1), 1.5))
    elif family == "opacity":
        logits = [20.0, -20.0, 30.0, -30.0, -87.0, -88.5, -104.0]     # saturated sigmoid; expf(-x) near overflow; 0 / subnormal
        # o G at the nearest pixel centre either side of the 0.99 clamp (Q6) and of the 1/255 skip (Q7)
        straddle = [0.99 * (1 - 1e-3), 0.99 * (1 + 1e-3), 0.99 * (1 + 2e-3), (1 / 255) * (1 - 2e-3), (1 / 255) * (1 + 2e-3)]
        n_sat = len(logits)
        rows = torch.arange(2 * (n_sat + len(straddle)))
        _at_pixels(sc, rows, 1.5 + 5.0 * torch.rand(len(rows), generator=g), 2)
        px = torch.tensor([1.6, 1.2, 1.0]).repeat(len(rows), 1)
        px[2 * n_sat:] *= 3.0                                        # wide enough that G at the nearest centre is ~0.997
        edits["_scaling"] = (rows, torch.log(px / FOCAL * sc.means3D[rows, 2:3]))
        G = _peak_pixel_gaussian(sc, cam, edits)[rows]
        for k in range(2 * n_sat, len(rows)):
            o = straddle[(k - 2 * n_sat) // 2] / G[k].item()
            logits.append(math.log(o / (1 - o)))
        logits = [v for v in logits[:n_sat] for _ in range(2)] + logits[n_sat:]
        edits["_opacity"] = (rows, torch.tensor(logits)[:, None])
    elif family == "scaling_tiny":
        ls = [torch.full((3,), -30.0)] * 4                            # the 2-D covariance is the +0.3 dilation alone (Q3)
        ls += [torch.tensor([-30.0, -30.0, 0.0]), torch.tensor([0.0, -30.0, -30.0])]
        rows = torch.arange(len(ls))
        _at_pixels(sc, rows, 2.0 + 4.0 * torch.rand(len(rows), generator=g), 3)
        ls = torch.stack(ls)
        ls[4:] += torch.log(3.0 / FOCAL * sc.means3D[rows[4:], 2:3]) * (ls[4:] == 0)
        edits["_scaling"] = (rows, ls)
        edits["_opacity"] = (rows, torch.full((len(rows), 1), 2.0))
        edits["_rotation"] = (rows, _unit(g, len(rows)).float())
    elif family == "scaling_giant_needle":
        depth = torch.tensor([1.2, 1.4, 1.6, 3.0, 4.0, 5.0])
        rows = torch.arange(len(depth))
        _at_pixels(sc, rows, depth, 5)
        ls = [torch.full((3,), v) for v in (4.0, 5.0, 6.0)]           # giants in front of the scene: every tile, every pixel
        ls += [torch.log(torch.tensor([1e3, 1.0, 1e-3]) * 2.0 / FOCAL * depth[k]) for k in (3, 4, 5)]   # axis ratio 1e6
        edits["_scaling"] = (rows, torch.stack(ls).float())
        edits["_opacity"] = (rows, torch.tensor([-1.0, 2.0, 0.0, 2.0, 2.0, 2.0])[:, None])   # one giant at the 0.99 clamp
        edits["_rotation"] = (rows, _unit(g, len(rows)).float())
    else:                                                             # SH clamp edge (Q8): C0 dc + 0.5 = 0, -1 ulp, +1 ulp
        ulp = float(np.spacing(np.float32(0.5)))
        trip = [_dc_for(0.0), _dc_for(-ulp), _dc_for(ulp / 2)]         # C0 dc one float32 step either side of -0.5
        assert np.float32(np.float32(C0_F32 * np.float32(trip[1])) + np.float32(0.5)) < 0
        assert np.float32(np.float32(C0_F32 * np.float32(trip[2])) + np.float32(0.5)) > 0
        perms = [(0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 0, 0), (1, 1, 1), (2, 2, 2)]
        dc = torch.tensor([[trip[a], trip[b], trip[c]] for a, b, c in perms for _ in range(2)])
        rows = torch.arange(dc.shape[0])
        _at_pixels(sc, rows, 2.0 + 3.0 * torch.rand(len(rows), generator=g), 4)
        edits["_features_dc"] = (rows, dc[:, None, :])
        edits["_opacity"] = (rows, torch.full((len(rows), 1), 3.0))
        edits["_scaling"] = (rows, torch.log(torch.tensor([3.0, 2.0, 2.5]) / FOCAL * sc.means3D[rows, 2:3]))
    return sc, cam, edits, rows


def _model(sc, edits, device):
    from synthetic_model import SyntheticGaussians
    pc = SyntheticGaussians(sc, device)
    with torch.no_grad():
        for leaf, (rows, vals) in edits.items():
            getattr(pc, leaf)[rows.to(device)] = vals.to(device, torch.float32).reshape(getattr(pc, leaf)[rows].shape)
    return pc


def _peak_pixel_gaussian(sc, cam, edits):
    """G = exp(power) at the pixel centre nearest each Gaussian's mean, from the float64 oracle's conic"""
    from oracle import torch_oracle as to
    seen = _seen(sc, _model(sc, edits, "cpu"))
    view = to.view_dict(cam, sh_degree=sc.sh_degree, **ST)
    pre = to.preprocess(seen.means3D, seen.opacities, view, scales=seen.scales, rotations=seen.rotations, shs=seen.shs)
    dx, dy = pre["px"] - pre["px"].round(), pre["py"] - pre["py"].round()
    con = pre["conic"]
    return torch.exp(-0.5 * (con[:, 0] * dx * dx + con[:, 2] * dy * dy) - con[:, 1] * dx * dy)


def _seen(sc, pc):
    """the activated inputs as torch evaluates the getters on pc's device (parity_utils.hip_render)"""
    seen = copy.copy(sc)
    with torch.no_grad():
        seen.means3D = pc.get_xyz.detach().cpu().contiguous()
        seen.scales = pc.get_scaling.detach().cpu().contiguous()
        seen.rotations = pc.get_rotation.detach().cpu().contiguous()
        seen.opacities = pc.get_opacity.detach().cpu().contiguous()
        seen.shs = pc.get_features.detach().cpu().contiguous()
    return seen


def _sh_flips(seen, rows):
    """rows whose float32 Q8 decision (C0 dc + 0.5 < 0, the kernels' and the float32 oracle's) differs from the float64
    truth's: legitimately different gradients, excluded from the truth comparison"""
    if seen.sh_degree != 0:
        return torch.zeros(seen.P, dtype=torch.bool)
    dc = seen.shs[:, 0].numpy().astype(np.float32)
    f32 = (np.float32(C0_F32) * dc + np.float32(0.5)) < 0
    f64 = (0.28209479177387814 * dc.astype(np.float64) + 0.5) < 0
    return torch.from_numpy((f32 != f64).any(axis=1))


def oracles(sc, cam, edits, dL):
    """(seen, float32 oracle result, float64 autograd grads, float64 radii, flags) for the case, from torch's getters on the CPU"""
    from oracle import oracle_ctypes as oc
    from oracle import torch_oracle as to
    pc = _model(sc, edits, "cpu")
    seen = _seen(sc, pc)
    orc = oc.rasterize(seen, cam, ST, BG)
    t_out, tg = to.forward_backward(seen, cam, ST, BG, dL)
    return seen, orc, tg, t_out


def _row_norm(t, P_):
    t = t.detach().double().cpu().reshape(P_, -1)
    return t.abs().max(dim=1).values if t.shape[1] else torch.zeros(P_, dtype=torch.float64)


def check_rows(name, got, ref, edge, clean):
    """got vs the float64 reference: whole tensor (clean rows, the usual max-norm) at BWD_RTOL; the ordinary rows alone at
    BWD_RTOL of THEIR max norm; every clean edge row at ROW_RTOL of its own magnitude (+ BWD_RTOL of the ordinary scale)"""
    P_ = ref.shape[0]
    got = got.detach().double().cpu().reshape(ref.shape)
    ref = ref.detach().double().cpu()
    ordinary = clean.clone()
    ordinary[edge] = False
    e_all = rel_err(got, ref, clean)
    e_ord = rel_err(got[ordinary], ref[ordinary])
    d = _row_norm(got - ref, P_)
    own = _row_norm(ref, P_)
    scale = max(own[ordinary].max().item(), 1e-30)
    e_clean = edge[clean[edge]]
    bad = d[e_clean] > ROW_RTOL * own[e_clean] + BWD_RTOL * scale
    report(name, "whole tensor", e_all)
    report(name, "ordinary rows", e_ord)
    worst = (d[e_clean] / (own[e_clean] + scale)).max().item() if e_clean.numel() else 0.0
    report(name, "edge rows, worst d / (own + ordinary scale)", worst)
    assert e_all <= BWD_RTOL, f"{name}: {e_all:.3e} (whole tensor)"
    assert e_ord <= BWD_RTOL, f"{name}: {e_ord:.3e} (ordinary rows)"
    assert not bad.any(), (f"{name}: edge rows {e_clean[bad].tolist()}: |d| {d[e_clean][bad].tolist()} "
                           f"vs own {own[e_clean][bad].tolist()} (ordinary scale {scale:.3e})")


def _run(entry, sc, cam, edits, dL):
    import diff_gaussian_rasterization as dgr
    from gaussian_renderer import render, render_fused
    pc = _model(sc, edits, "cuda")
    prev = dgr.chain_reference_getters
    dgr.chain_reference_getters = entry == "chained"
    try:
        fn = render_fused if entry == "fused" else render
        out = fn(cam.to("cuda"), pc, PIPE, BG.cuda(), **ST)
        used = type(out["render"].grad_fn).__name__
        out["render"].backward(dL.cuda())
        torch.cuda.synchronize()
    finally:
        dgr.chain_reference_getters = prev
    # the chain recognises the reference's stored layout only (features_rest [P,15,3]); a model built for a lower degree
    # takes the plain path (_match_reference_getters)
    chains = entry == "chained" and pc._features_rest.shape[1] == 15
    want = None if entry == "fused" else "_RasterizeGaussiansChainedBackward" if chains else "_RasterizeGaussiansBackward"
    assert want is None or used == want, (entry, used)
    return out, pc


FAMILIES = ("rotation", "opacity", "scaling_tiny", "scaling_giant_needle", "sh_stored_deg3", "sh_built_deg0")
# Giant and 1e6-needle Gaussians are ill-conditioned in float32 itself: a needle's 2-D covariance loses its thin direction to
# cancellation (1e-7 x a ~1e6 px^2 long variance, against the 0.3 px^2 dilation), and a giant's alpha / transmittance decisions
# sit within rounding somewhere on almost every pixel.  The float32 oracle is 1e-3 .. 5e-2 from the float64 truth there, so
# this family is held to the float32 algorithm (the parity rules of parity_utils.check_backward: 1e-4 on the undecided-free
# Gaussians) and to the three-way rule (no farther from the truth than the float32 oracle: check_against_truth).
ILL_CONDITIONED = {"scaling_giant_needle"}


@pytest.mark.parametrize("family", FAMILIES)
def test_activation_edges_against_float64(family):
    from oracle import oracle_ctypes as oc
    from parity_utils import check_against_truth, check_backward
    sc, cam, edits, edge = _case(family)
    dL = scenes.grad_seed(W, H, 60 + len(family))
    seen, orc, tg, t_out = oracles(sc, cam, edits, dL)
    flagged = (orc.borderline_gaussians | (t_out["radii"] != orc.radii) | _sh_flips(seen, edge)).cpu()
    n_flag = int(flagged[edge].sum())
    report(family, "flagged edge rows", n_flag)
    # a giant or a needle is undecided somewhere by construction; everywhere else at most a couple of edge rows may be
    assert n_flag <= (len(edge) if family in ILL_CONDITIONED else FLAGGED_EDGE_ROWS_MAX), \
        f"{family}: {n_flag} edge rows flagged {edge[flagged[edge]].tolist()}"
    assert (orc.radii[edge] > 0).sum().item() >= len(edge) // 3, "the edge rows must be rendered"
    clean = ~flagged
    og = oc.backward(orc, dL) if family in ILL_CONDITIONED else None
    res = {}
    for entry in ENTRIES:
        if entry == "fused" and sc.shs.shape[1] != 16:
            # raw mode reads the stored layout (features_rest [P,15,3]) only, and says so instead of guessing
            with pytest.raises(ValueError, match="features_rest"):
                _run(entry, sc, cam, edits, dL)
            continue
        out, pc = _run(entry, sc, cam, edits, dL)
        res[entry] = (out, pc)
        name = f"{family} {entry}"
        check_forward(out, orc, name)
        m2 = out["viewspace_points"].grad
        for k, (got, _) in leaf_space(pc, m2, tg).items():
            assert torch.isfinite(got).all(), f"{name}: non-finite {k}"
        if family in ILL_CONDITIONED:
            check_backward(pc, m2, og, name, flagged=orc.borderline_gaussians)
            check_against_truth(name, seen, cam, ST, BG, dL, out, pc, m2, orc, og)
        else:
            assert flagged.float().mean().item() < 0.03
            for k, (got, ref) in leaf_space(pc, m2, tg).items():
                check_rows(f"{name} {k}", got, ref, edge, clean)
    # the chained kernel backward of sigmoid / normalize against autograd's own, row by row
    (a, pa), (b, pb) = res["plain"], res["chained"]
    assert torch.equal(a["render"], b["render"]) and torch.equal(a["radii"], b["radii"])
    ordinary = torch.ones(P, dtype=torch.bool)
    ordinary[edge] = False
    for k, leaf in LEAF_OF.items():
        ga, gb = getattr(pa, leaf).grad, getattr(pb, leaf).grad
        d, own = _row_norm(gb - ga, P), _row_norm(ga, P)
        floor = max(own[ordinary].max().item(), 1e-30)
        e = (d[edge] / own[edge].clamp_min(floor)).max().item()
        report(family, f"chained vs plain {k}, edge rows", e)
        assert e <= HIP_VS_HIP_RTOL, f"{family}: chained vs plain {k} {e:.3e}"


def _onto_depth(pw, viewmatrix, target):
    """pw [m,3] float32 moved by at most 4 ulps per coordinate so that the float32 view depth (depth_key_f32) equals
    target [m] where some such move reaches it (rounding the world position from float64 alone moves the depth by ~10 ulps)"""
    from oracle import torch_oracle as to
    bits = pw.contiguous().view(torch.int32)
    out, hit = pw.clone(), torch.zeros(pw.shape[0], dtype=torch.bool)
    r = range(-4, 5)
    for a in r:
        for b in r:
            for c in r:
                cand = (bits + torch.tensor([a, b, c], dtype=torch.int32)).view(torch.float32)
                new = ~hit & (to.depth_key_f32(cand, viewmatrix) == target)
                out[new] = cand[new]
                hit |= new
    return out


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 100_003])
def test_mark_visible_near_plane(n):
    """GaussianRasterizer.markVisible (mark_visible_kernel) against the oracle's near-plane rule Q1: float32 view depth
    ((m2 x + m6 y) + m10 z) + m14 > 0.2 (torch_oracle.depth_key_f32), under a general camera pose, with points placed
    within a float32 ulp of view depth 0.2 and every partial block size."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from oracle import torch_oracle as to
    g = torch.Generator().manual_seed(900 + n)
    q = _unit(g, 1)
    R = to.quat_to_rot(q)[0].numpy()                                   # world -> view rotation
    # a general rotation; the camera within 0.1 of the world origin, so that the float32 depth's partial sums are ~0.2 and
    # resolve single ulps of 0.2 (a translation of ~2 leaves the depth on a grid of ~8 ulps of 0.2 there)
    Tv = (torch.rand(3, generator=g, dtype=torch.float64) * 0.2 - 0.1).numpy()
    cam = scenes.make_camera(R.T, Tv, 1.1, 0.8, 64, 48)                 # make_camera takes camera-to-world R (COLMAP)
    # view-space points: depths around the near plane, and for a third of them within one float32 step of 0.2
    z = (torch.rand(n, generator=g, dtype=torch.float64) * 0.4 - 0.1) + 0.2 * (torch.rand(n, generator=g) < 0.5)
    z0 = np.float32(0.2)
    close = [float(np.nextafter(z0, np.float32(0))), float(z0), float(np.nextafter(z0, np.float32(1)))]
    k = torch.arange(n) % 3 == 0
    z[k] = torch.tensor(close, dtype=torch.float64)[torch.arange(int(k.sum())) % 3]
    xy = torch.randn(n, 2, generator=g, dtype=torch.float64) * z.abs()[:, None]
    pv = torch.cat([xy, z[:, None]], dim=1)
    V = cam.world_view_transform.double()                             # row-vector convention: p_view = [p, 1] @ V
    pw = ((pv - V[3, :3]) @ torch.linalg.inv(V[:3, :3])).float().contiguous()
    pw[k] = _onto_depth(pw[k], cam.world_view_transform, torch.tensor(close)[torch.arange(int(k.sum())) % 3])
    want = to.depth_key_f32(pw, cam.world_view_transform) > 0.2
    camd = cam.to("cuda")
    rs = GaussianRasterizationSettings(image_height=48, image_width=64, tanfovx=math.tan(0.55), tanfovy=math.tan(0.4),
                                       bg=torch.zeros(3, device="cuda"), scale_modifier=1.0,
                                       viewmatrix=camd.world_view_transform, projmatrix=camd.full_proj_transform,
                                       sh_degree=0, campos=camd.camera_center, prefiltered=False, debug=False)
    got = GaussianRasterizer(rs).markVisible(pw.to("cuda")).cpu()
    assert got.dtype == torch.bool and got.shape == (n,)
    assert torch.equal(got, want), (got != want).nonzero()[:10].flatten().tolist()
    if n >= 255:                                                      # the near plane is actually straddled at float32 resolution
        d = to.depth_key_f32(pw, cam.world_view_transform)
        at = (d - z0).abs() <= float(np.spacing(z0))
        assert at.sum() >= n // 4 and want[at].any() and not want[at].all(), int(at.sum())
