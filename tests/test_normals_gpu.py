"""Normal maps on the GPU (SPEC M17; include/msgs.h msgs_gaussian_normals_*, msgs_depth_normal_*).

References, none of them the kernels under test:
  1  tests/normals_truth.py (float64, written from the definitions; pinned by tests/test_normals_cpu.py), gradients by float64
     autograd;
  2  the routes render_with_normals() is composed of — render_with_features fed gaussian_normals(...), render_with_median_depth,
     render() — bit for bit.
Tolerances.  Forward: max(1e-6, 4 x the error of the float32 restatement of the same formulas on the same inputs), the rule of
tests/test_filter3d_gpu.py; a row whose sign decision lies within 1e-5 of its threshold (flagged by the truth, at most 1 % of a
scene) may carry either sign.  Gradients: BWD_RTOL in max-norm (the restatement's own backward error is a few 1e-6 on these
depth maps, so the fall-back to 4 x restatement is not used).  Routes: FWD_ATOL / BWD_RTOL.  The measured maxima are printed
(pytest -s) and recorded in profiles/normals_notes.md."""
import functools

import pytest
import torch

import diff_gaussian_rasterization as dgr
import normals_truth as nt
import scenes
from parity_utils import BWD_RTOL, FWD_ATOL, PIPE, rel_err, report, small_scene
from route_utils import reset_forward_state
from synthetic_model import SyntheticGaussians

pytestmark = pytest.mark.gpu

TILE_W, TILE_H = dgr.DEPTH_NORMAL_TILE_W, dgr.DEPTH_NORMAL_TILE_H
SHAPES = nt.depth_shapes(TILE_W, TILE_H)
BG = (0.1, 0.2, 0.3)


def _settings(W, H, cam=None, tanfov=nt.TANFOV):
    cam = (cam or scenes.front_camera(W, H)).to("cuda")
    return dgr.GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=tanfov[0], tanfovy=tanfov[1], bg=torch.zeros(3, device="cuda"),
        scale_modifier=1.0, viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, sh_degree=0,
        campos=cam.camera_center, prefiltered=False, debug=False)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. Gaussian normals
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gaussian_truth(P, raw, world):
    m, s, r, g = nt.gaussian_rows(P, raw)
    return m, s, r, g, nt.gaussian_truth(m, s, r, g, nt.camera(), world)


def _run_gaussian(m, s, r, g, world, rs=None):
    rs = rs or _settings(1920, 1080, nt.camera())
    M, S, R = (t.cuda().requires_grad_(True) for t in (m, s, r))
    n = dgr.gaussian_normals(M, S, R, rs, world=world)
    (n * g.cuda()).sum().backward()
    torch.cuda.synchronize()
    return n.detach(), R.grad, M.grad, S.grad


@pytest.mark.parametrize("world", [False, True], ids=["view", "world"])
@pytest.mark.parametrize("raw", [False, True], ids=["activated", "raw"])
@pytest.mark.parametrize("P", nt.GAUSSIAN_P)
def test_gaussian_normals_against_float64(P, raw, world):
    m, s, r, g, t = _gaussian_truth(P, raw, world)
    what = f"gaussian normals P={P} {'raw' if raw else 'activated'} {'world' if world else 'view'}"
    n, g_r, g_m, g_s = _run_gaussian(m, s, r, g, world)
    again = _run_gaussian(m, s, r, g, world)
    assert n.shape == (P, 3) and n.dtype == torch.float32 and g_r.shape == (P, 4)
    assert torch.equal(n, again[0]) and torch.equal(g_r, again[1])                   # two runs: the same bits
    assert g_m is None or not g_m.any()
    assert g_s is None or not g_s.any()
    ok, fl = ~t["flagged"], t["flagged"]
    tol = max(1e-6, 4.0 * t["restated"])
    err = (n.cpu().double() - t["normal"]).abs().max(dim=1).values
    e = err[ok].max().item() if ok.any() else 0.0
    report(what, f"normal max abs err on unflagged rows (restatement {t['restated']:.2e}, bound {tol:.2e})", e)
    assert e <= tol
    if fl.any():                                                                     # either sign
        flipped = (n.cpu().double() + t["normal"]).abs().max(dim=1).values
        assert (torch.minimum(err, flipped)[fl] <= tol).all()
    e_g = rel_err(g_r, t["grad"], rows=ok)
    report(what, "grad rotations max-norm rel err", e_g)
    assert e_g <= BWD_RTOL
    assert torch.isfinite(n).all() and torch.isfinite(g_r).all()
    assert (n.norm(dim=1) - 1).abs().max() <= 1e-5


def test_gaussian_normals_hand_made_rows():
    cam = nt.camera()
    rs = _settings(1920, 1080, cam)
    m0, s0, r0, g0 = nt.gaussian_rows(257, raw=True)
    m, s, r = m0.clone(), torch.exp(s0), r0.clone()
    s[3] = torch.tensor([2.0, 1.0, 1.0])                 # two equal smallest scales: the lower index, 1
    s[4] = torch.tensor([1.0, 2.0, 1.0])                 # ... 0
    s[5] = torch.tensor([0.5, 0.5, 0.5])                 # isotropic: 0
    r[6] = torch.tensor([3e-13, -4e-13, 0.0, 0.0])       # ||r|| < 1e-12: q = r / 1e-12, finite
    r[7] = 0.0
    t = nt.gaussian_truth(m, s, r, g0, cam, True)
    assert t["k"][3:6].tolist() == [1, 0, 0]
    n, g_r, _, _ = _run_gaussian(m, s, r, g0, True, rs)
    assert torch.isfinite(n).all() and torch.isfinite(g_r).all()
    ok = ~t["flagged"]
    assert (n.cpu().double() - t["normal"]).abs()[ok].max().item() <= max(1e-6, 4.0 * t["restated"])
    assert rel_err(g_r[3:6], t["grad"][3:6]) <= BWD_RTOL
    # under the clamp the gradient is g / eps, without the projection: compared on those rows against their own scale
    assert rel_err(g_r[6:8], t["grad"][6:8]) <= BWD_RTOL
    for row in (3, 4, 5):                                # the selected column, whatever the sign
        R = nt.rotation_matrix(nt.normalise(r[row:row + 1].double()))[0]
        assert ((n[row].cpu().double().abs() - R[:, int(t["k"][row])].abs()).abs() <= 1e-6).all()
    # a NaN or Inf in any input of a row: (0, 0, 0) there, no gradient there, the neighbours keep their bits
    clean_n, clean_g, _, _ = _run_gaussian(m, s, r, g0, False, rs)
    bad_m, bad_s, bad_r = m.clone(), s.clone(), r.clone()
    bad_m[10, 1], bad_s[70, 2], bad_r[130, 0], bad_r[200, 3], bad_m[256, 0] = (float("nan"), float("inf"), float("nan"),
                                                                              float("-inf"), float("inf"))
    rows = torch.tensor([10, 70, 130, 200, 256])
    n, g_r, _, _ = _run_gaussian(bad_m, bad_s, bad_r, g0, False, rs)
    assert not n[rows].any() and not g_r[rows].any()
    keep = torch.ones(257, dtype=torch.bool)
    keep[rows] = False
    assert torch.equal(n[keep], clean_n[keep]) and torch.equal(g_r[keep], clean_g[keep])
    assert torch.isfinite(n).all() and torch.isfinite(g_r).all()


def test_log_scales_activated_scales_and_filtered_scales_select_the_same_axis():
    m, logs, r, _ = nt.gaussian_rows(4099, raw=True)
    rs = _settings(1920, 1080, nt.camera())
    M, R = m.cuda(), r.cuda()
    act = torch.exp(logs.cuda())
    filt = torch.full((4099, 1), nt.AXIS_TEST_FILTER, device="cuda")
    s_eff, _ = dgr.smoothing_filter(act, torch.full((4099, 1), 0.5, device="cuda"), filt)
    a, b, c = (dgr.gaussian_normals(M, S, R, rs) for S in (logs.cuda(), act, s_eff))
    assert torch.equal(a, b) and torch.equal(a, c) and a.abs().max() > 0


def test_gaussian_normals_empty_strided_and_float64():
    rs = _settings(1920, 1080, nt.camera())
    z = lambda *sh: torch.zeros(*sh, device="cuda", requires_grad=True)
    R = z(0, 4)
    n = dgr.gaussian_normals(z(0, 3), z(0, 3), R, rs)
    assert n.shape == (0, 3)
    n.sum().backward()
    assert R.grad.shape == (0, 4)
    m, s, r, g = nt.gaussian_rows(257, raw=True)
    want, want_g, _, _ = _run_gaussian(m, s, r, g, False, rs)
    wide = lambda t: torch.zeros(t.shape[0], 2 * t.shape[1], dtype=torch.float64, device="cuda")
    wm, ws, wr = wide(m), wide(s), wide(r)
    wm[:, ::2], ws[:, ::2], wr[:, ::2] = m.cuda().double(), s.cuda().double(), r.cuda().double()
    wr.requires_grad_(True)
    n = dgr.gaussian_normals(wm[:, ::2], ws[:, ::2], wr[:, ::2], rs)
    (n * g.cuda()).sum().backward()
    assert n.dtype == torch.float32 and torch.equal(n.detach(), want)
    assert wr.grad.dtype == torch.float64 and torch.equal(wr.grad[:, ::2].float(), want_g) and not wr.grad[:, 1::2].any()
    with pytest.raises(RuntimeError, match="HIP device"):
        dgr.gaussian_normals(m, s, r, rs)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. depth to normal
# ---------------------------------------------------------------------------------------------------------------------------
def _upstream(H, W):
    return scenes.grad_seed(W, H, 5) * float(W * H)                                  # N(0, 1)


@functools.lru_cache(maxsize=None)
def _depth_truth(shape, world):
    H, W = shape
    z = nt.depth_map(H, W)
    vm = nt.camera().world_view_transform if world else None
    return z, nt.depth_truth(z, _upstream(H, W), vm)


def _run_depth(z, G, world, cam=None):
    H, W = z.shape
    rs = _settings(W, H, cam or nt.camera())
    Z = z.cuda().requires_grad_(True)
    n = dgr.depth_to_normal(Z, rs, world=world)
    (n * G.cuda()).sum().backward()
    torch.cuda.synchronize()
    return n.detach(), Z.grad


@pytest.mark.parametrize("world", [False, True], ids=["view", "world"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_depth_to_normal_against_float64(shape, world):
    H, W = shape
    z, t = _depth_truth(shape, world)
    what = f"depth_to_normal {H}x{W} {'world' if world else 'view'}"
    G = _upstream(H, W)
    n, g = _run_depth(z, G, world)
    again = _run_depth(z, G, world)
    assert n.shape == (3, H, W) and n.dtype == torch.float32 and g.shape == (H, W)
    assert torch.equal(n, again[0]) and torch.equal(g, again[1])                     # two runs: the same bits
    valid = t["valid"]
    nc = n.cpu()
    assert not nc[:, ~valid].any()                                                   # exactly 0 off the valid pixels
    if min(H, W) < 3:
        assert not valid.any() and not nc.any() and not g.any()
        return
    assert (nc[:, valid].abs().sum(dim=0) > 0).all()
    tol = max(1e-6, 4.0 * t["restated"])
    err = (nc.double() - t["normal"]).abs().max(dim=0).values
    report(what, f"normal max abs err on valid pixels (restatement {t['restated']:.2e}, bound {tol:.2e})", err.max().item())
    assert err.max().item() <= tol
    assert t["restated_bwd"] <= BWD_RTOL                                             # (else the bound would be 4 x restatement)
    e_g = rel_err(g, t["grad"])
    report(what, f"grad depth max-norm rel err (restatement {t['restated_bwd']:.2e})", e_g)
    assert e_g <= BWD_RTOL
    # the rows and columns on either side of every tile seam, on their own
    scale = t["grad"].abs().max().item()
    gd = (g.cpu().double() - t["grad"]).abs()
    for x in range(TILE_W, W, TILE_W):
        assert err[:, x - 1:x + 1].max().item() <= tol and gd[:, x - 2:x + 2].max().item() <= BWD_RTOL * scale
    for y in range(TILE_H, H, TILE_H):
        assert err[y - 1:y + 1].max().item() <= tol and gd[y - 2:y + 2].max().item() <= BWD_RTOL * scale


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("inf")], ids=["zero", "negative", "nan", "inf"])
def test_a_hole_invalidates_exactly_its_four_neighbours(bad):
    H, W = SHAPES[-1]
    z = nt.depth_map(H, W)
    G = _upstream(H, W)
    clean_n, clean_g = _run_depth(z, G, False)
    holes = [(TILE_H, TILE_W), (TILE_H - 1, 2 * TILE_W - 1), (2 * TILE_H, 5), (3, TILE_W + 1), (1, 1), (H - 1, 7), (9, W - 2)]
    zz = z.clone()
    for y, x in holes:
        zz[y, x] = bad
    t = nt.depth_truth(zz, G)
    want = nt.depth_truth(z, G)["valid"].clone()
    for y, x in holes:
        for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
            if 0 <= yy < H and 0 <= xx < W:
                want[yy, xx] = False
    assert torch.equal(t["valid"], want)                                             # (the truth itself)
    n, g = _run_depth(zz, G, False)
    nc = n.cpu()
    assert torch.isfinite(n).all() and torch.isfinite(g).all()
    assert torch.equal(nc.abs().sum(dim=0) > 0, want)
    assert torch.equal(nc[:, want], clean_n.cpu()[:, want])                          # everybody else keeps their bits
    for y, x in holes:
        assert g[y, x].item() == 0.0                                                 # the hole gets nothing
    assert rel_err(g, t["grad"]) <= BWD_RTOL
    assert not torch.equal(g, clean_g)


def test_world_normals_are_the_view_normals_rotated():
    H, W = SHAPES[-1]
    z = nt.depth_map(H, W)
    G = _upstream(H, W)
    cam = nt.camera()
    view, _ = _run_depth(z, G, False, cam)
    world, _ = _run_depth(z, G, True, cam)
    R = cam.world_view_transform.double()[:3, :3]
    want = torch.einsum("jk,khw->jhw", R, view.cpu().double())
    e = (world.cpu().double() - want).abs().max().item()
    report("depth_to_normal world", "world vs rotated view normals, max abs", e)
    assert e <= 1e-6 and (world - view).abs().max() > 0.1


def test_depth_to_normal_takes_float64_strided_and_one_channel_maps_and_refuses_the_cpu():
    H, W = SHAPES[-1]
    z = nt.depth_map(H, W)
    rs = _settings(W, H)
    want = dgr.depth_to_normal(z.cuda(), rs)
    wide = torch.zeros(H, 2 * W, dtype=torch.float64, device="cuda")
    wide[:, ::2] = z.cuda().double()
    assert torch.equal(dgr.depth_to_normal(wide[:, ::2], rs), want)
    assert torch.equal(dgr.depth_to_normal(z.cuda()[None], rs), want)
    with pytest.raises(RuntimeError, match="HIP device"):
        dgr.depth_to_normal(z, rs)
    with pytest.raises(ValueError):
        dgr.depth_to_normal(z.cuda()[:-1], rs)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. end to end
# ---------------------------------------------------------------------------------------------------------------------------
E2E = dict(P=300, W=64, H=48, seed=41)               # = tests/test_normals_cpu.py
LEAVES = SyntheticGaussians.LEAVES


@functools.lru_cache(maxsize=None)
def _scene():
    return small_scene(E2E["P"], E2E["W"], E2E["H"], E2E["seed"])


def _fresh():
    sc, cam = _scene()
    reset_forward_state()
    return SyntheticGaussians(sc, "cuda", requires_grad=True), cam.to("cuda"), torch.tensor(BG, device="cuda")


def _grads(pc, out):
    torch.cuda.synchronize()
    g = {n: getattr(pc, n).grad.detach().clone() for n in LEAVES if getattr(pc, n).grad is not None}
    if out["viewspace_points"].grad is not None:
        g["viewspace"] = out["viewspace_points"].grad.detach().clone()
    return g


def _plain_loss(out):
    W, H = E2E["W"], E2E["H"]
    return (out["render"] * scenes.grad_seed(W, H, 78).cuda()).sum() + (out["depth"] * scenes.grad_seed(W, H, 77)[0].cuda() * 0.1).sum()


def test_render_with_normals_is_its_composition_bit_for_bit():
    import normals
    from gaussian_renderer import _settings as host_settings, render, render_with_features, render_with_median_depth
    pc, cam, bg = _fresh()
    out = normals.render_with_normals(cam, pc, PIPE, bg)
    assert set(out) == {"render", "acc_pixel_size", "depth", "viewspace_points", "visibility_filter", "radii", "pixel_sizes",
                        "alpha", "normal", "surf_depth", "surf_normal", "median_id"}
    H, W = E2E["H"], E2E["W"]
    assert out["normal"].shape == (3, H, W) and out["surf_normal"].shape == (3, H, W) and out["surf_depth"].shape == (H, W)
    _plain_loss(out).backward()
    g_out = _grads(pc, out)
    # "normal": render_with_features fed gaussian_normals
    pc2, _, _ = _fresh()
    rs = host_settings(cam, pc2, PIPE, bg, 1.0, False, False, 1.0)
    feats = dgr.gaussian_normals(pc2.get_xyz, pc2.get_scaling, pc2.get_rotation, rs)
    f = render_with_features(cam, pc2, PIPE, bg, feats)
    assert torch.equal(out["normal"], f["features"]) and out["normal"].abs().max() > 0.1
    # "surf_normal": depth_to_normal of render_with_median_depth's map
    reset_forward_state()
    md = render_with_median_depth(cam, pc2, PIPE, bg)
    assert torch.equal(out["surf_depth"], md["median_depth"]) and torch.equal(out["median_id"], md["median_id"])
    assert torch.equal(out["surf_normal"], dgr.depth_to_normal(md["median_depth"], rs))
    assert (out["surf_normal"].abs().sum(dim=0) > 0).float().mean() > 0.2
    # "render", "depth" and their gradients: render()'s when the loss ignores the new maps
    pc3, _, _ = _fresh()
    plain = render(cam, pc3, PIPE, bg)
    _plain_loss(plain).backward()
    g_plain = _grads(pc3, plain)
    for k in ("render", "depth", "acc_pixel_size", "radii", "pixel_sizes"):
        assert torch.equal(out[k], plain[k]), k
    assert set(g_out) == set(g_plain)
    for k in g_plain:
        assert torch.equal(g_out[k], g_plain[k]), k


def _consistency_run(**kw):
    import normals
    pc, cam, bg = _fresh()
    out = normals.render_with_normals(cam, pc, PIPE, bg, **kw)
    loss = normals.normal_consistency(out)
    loss.backward()
    return loss.detach(), _grads(pc, out), out


def test_normal_consistency_reaches_rotations_and_means_reproducibly():
    loss, g, out = _consistency_run()
    again_loss, again, _ = _consistency_run()
    report("normals end to end", "normal_consistency loss", loss.item())
    assert torch.isfinite(loss) and 0.0 < loss.item() < 2.0
    for k in ("_rotation", "_xyz"):
        assert torch.isfinite(g[k]).all() and g[k].abs().max() > 0, k
    assert torch.equal(loss, again_loss)
    for k in g:
        assert torch.isfinite(g[k]).all() and torch.equal(g[k], again[k]), k
    # world space: the same loss up to the rotation's rounding
    loss_w, _, _ = _consistency_run(world=True)
    assert abs(loss_w.item() - loss.item()) <= 1e-5


def test_fused_route_matches_the_plain_route():
    import normals
    W, H = E2E["W"], E2E["H"]
    G = scenes.grad_seed(W, H, 79).cuda()

    def run(fused):
        pc, cam, bg = _fresh()
        out = normals.render_with_normals(cam, pc, PIPE, bg, fused=fused)
        (_plain_loss(out) + (out["normal"] * G).sum() + (out["alpha"] * G[0]).sum()).backward()
        return out, _grads(pc, out)
    (a, ga), (b, gb) = run(False), run(True)
    for k in ("render", "alpha", "normal"):
        e = (a[k] - b[k]).abs().max().item()
        report("normals fused", f"{k} fused vs plain, max abs", e)
        assert e <= FWD_ATOL, k
    same = a["median_id"] == b["median_id"]
    assert same.float().mean().item() >= 0.99
    assert (a["surf_depth"] - b["surf_depth"]).abs()[same].max().item() <= FWD_ATOL
    assert set(ga) == set(gb)
    for k in ga:
        e = rel_err(gb[k], ga[k])
        report("normals fused", f"grad {k} fused vs plain, max-norm rel", e)
        assert e <= BWD_RTOL, k


def test_expected_depth_runs():
    loss, g, out = _consistency_run(depth="expected")
    assert "median_id" not in out and torch.isfinite(loss)
    assert torch.equal(out["surf_depth"], out["depth"] / out["alpha"].clamp_min(1e-8))
    rs_valid = out["surf_normal"].abs().sum(dim=0) > 0
    assert rs_valid.any() and torch.isfinite(out["surf_normal"]).all()
    for k in ("_rotation", "_xyz", "_opacity"):
        assert torch.isfinite(g[k]).all() and g[k].abs().max() > 0, k


def test_a_filtered_model_is_rendered_through_its_filter_with_unfiltered_normals():
    import filter3d
    import normals
    from gaussian_renderer import render_with_features
    pc, cam, bg = _fresh()
    filter3d.compute_3D_filter(pc, [cam], variance=2.0)
    with torch.no_grad():
        out = normals.render_with_normals(cam, pc, PIPE, bg)
        reset_forward_state()
        want = filter3d.render_with_3d_filter(cam, pc, PIPE, bg)
        assert torch.equal(out["render"], want["render"])
        with pytest.raises(ValueError, match="filter_3D"):
            normals.render_with_normals(cam, pc, PIPE, bg, fused=True)
        pc.filter_3D = None
        reset_forward_state()
        plain = normals.render_with_normals(cam, pc, PIPE, bg)
        assert (out["render"] - plain["render"]).abs().max() > 1e-3 and out["normal"].abs().max() > 0.1


def test_verification_mode_is_refused_before_any_launch(monkeypatch):
    import normals
    pc, cam, bg = _fresh()
    calls = []
    monkeypatch.setattr(dgr, "_normals_probe", calls.append)
    before = dgr.forward_stats["forwards"]
    prev = dgr.set_deterministic(True)
    try:
        for fused in (False, True):
            with pytest.raises(ValueError, match="verification mode"):
                normals.render_with_normals(cam, pc, PIPE, bg, fused=fused)
    finally:
        dgr.set_deterministic(prev)
    assert dgr.forward_stats["forwards"] == before and calls == []
