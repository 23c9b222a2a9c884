"""Gradients of the camera: viewmatrix, projmatrix and campos (include/msgs.h msgs_backward_with_camera).

The truth is the float64 torch oracle with float64 camera leaves (oracle/torch_oracle.py, checked against central differences
in tests/test_camera_grad_cpu.py).  Its depth map is not differentiable, so a depth loss enters the oracle as a second pass
whose colour is [z, 0, 0] with z = (p, 1) V[:, 2] (differentiable in V) on a zero background: the depth map restated as a
colour channel, as tests/test_depth_grad_gpu.py does on the HIP side.  Both sides put no weight on the oracle's borderline
pixels (an alpha decision near a flip), so they blend the same entries.  Identities that need no oracle — moving the camera
is moving the world the other way — run on every backward route."""
import copy
import ctypes as C
import math
import types

import pytest
import torch

import diff_gaussian_rasterization as dgr
import scenes
from oracle import torch_oracle as to
from parity_utils import PIPE, report, small_scene
from route_utils import reset_forward_state
from synthetic_model import SyntheticGaussians
from test_depth_grad_gpu import MS, _env, _scene, _set_route

pytestmark = pytest.mark.gpu

W, H = 160, 96
# max|g - g64| <= CEIL * max|g64| per camera tensor.  Measured on the MI355X over every case of this file: 9.2e-7 .. 7.2e-6 (V),
# 1.1e-6 .. 2.1e-6 (campos), 1.6e-6 .. 5.8e-6 (PM); the verification mode 1.2e-6 .. 6.0e-6 — not tighter: its sums are
# exact either way, and what is left is the float32 arithmetic of the per-Gaussian backward that both modes share.
CEIL = 2e-5
# translation / rotation identities (one backward, no oracle): measured <= 1.4e-8 resp. 4.3e-9 of the summed magnitudes
IDENTITY_CEIL = 1e-7
COV = types.SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=True, debug=False)
COLORS = types.SimpleNamespace(convert_SHs_python=True, compute_cov3D_python=False, debug=False)


@pytest.fixture(autouse=True)
def _restore():
    chain = dgr.chain_reference_getters
    yield
    dgr.chain_reference_getters = chain
    dgr._C.lib.msgs_set_backward_generation(0)
    dgr._C.lib.msgs_set_blend_granularity(0)


def _case(kind):
    """(scene, camera, settings, scaling_modifier, pipe)"""
    if kind == "plain":
        sc, cam = small_scene(2000, W, H, seed=31)
        return sc, cam, {}, 1.0, PIPE
    if kind == "multiscale":
        sc, cam = small_scene(2500, W, H, seed=32, multiscale=True, scale_k=0.004 * 1920.0 / W * 0.25)
        return sc, cam, MS, 1.0, PIPE
    if kind == "scaling_modifier":
        sc, cam = small_scene(2000, W, H, seed=33)
        return sc, cam, {}, 0.7, PIPE
    if kind == "cov3D_precomp":
        sc, cam = small_scene(2000, W, H, seed=34)
        return sc, cam, {}, 1.0, COV
    if kind == "colors_precomp":
        sc, cam = small_scene(2000, W, H, seed=35)
        return sc, cam, {}, 1.0, COLORS
    raise KeyError(kind)


def _seeds(w=W, h=H):
    return scenes.grad_seed(w, h, 81), scenes.grad_seed(w, h, 82)[0] * 0.1


def _leaf_camera(cam, pm_from_v=False):
    """cam on the GPU with leaf tensors: {V, PM, cp} (PM = V @ proj when pm_from_v: then no PM leaf)"""
    from camera_pose import projection_of
    c = copy.copy(cam.to("cuda"))
    V = c.world_view_transform.clone().requires_grad_(True)
    cp = c.camera_center.clone().requires_grad_(True)
    c.world_view_transform, c.camera_center = V, cp
    leaves = {"V": V, "cp": cp}
    if pm_from_v:
        c.full_proj_transform = V @ projection_of(cam).to("cuda", torch.float32)
    else:
        PM = c.full_proj_transform.clone().requires_grad_(True)
        c.full_proj_transform = PM
        leaves["PM"] = PM
    return c, leaves


def _hip(sc, cam, st, smod, pipe, dL, Gd=None, entry="plain", pm_from_v=False, camera_grad=True, bg=None):
    """one forward + backward; returns (out, per-Gaussian grads, camera grads {V, PM, cp})"""
    from gaussian_renderer import render, render_fused
    dgr.chain_reference_getters = entry == "chained"
    pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
    if camera_grad:
        c, leaves = _leaf_camera(cam, pm_from_v)
    else:
        c, leaves = cam.to("cuda"), {}
    bgd = (bg if bg is not None else torch.tensor([0.1, 0.2, 0.3])).cuda()
    if entry == "fused":
        out = render_fused(c, pc, pipe, bgd, scaling_modifier=smod, **st)
    else:
        out = render(c, pc, pipe, bgd, scaling_modifier=smod, **st)
    loss = (out["render"] * dL.cuda()).sum()
    if Gd is not None:
        loss = loss + (out["depth"] * Gd.cuda()).sum()
    loss.backward()
    torch.cuda.synchronize()
    g = {n: getattr(pc, n).grad for n in pc.LEAVES}
    g["viewspace"] = out["viewspace_points"].grad
    g = {k: (v.detach().clone() if v is not None else None) for k, v in g.items()}
    cg = {k: v.grad for k, v in leaves.items()}
    return out, g, cg


def _oracle(sc, cam, st, smod, pipe, dL, Gd=None, pm_from_v=False):
    """float64 camera gradients {V, PM, cp} of the oracle, and the borderline mask [H, W]"""
    from camera_pose import projection_of
    dt = torch.float64
    V = cam.world_view_transform.to(dt).clone().requires_grad_(True)
    cp = cam.camera_center.to(dt).clone().requires_grad_(True)
    leaves = {"V": V, "cp": cp}
    if pm_from_v:
        PM = V @ projection_of(cam)
    else:
        PM = cam.full_proj_transform.to(dt).clone().requires_grad_(True)
        leaves["PM"] = PM
    view = to.view_dict(cam, sh_degree=sc.sh_degree, scale_modifier=smod, **st)
    view["viewmatrix"], view["projmatrix"], view["campos"] = V, PM, cp
    p = sc.means3D.to(dt)
    kw = dict(max_pixel_sizes=sc.max_pixel_sizes, min_pixel_sizes=sc.min_pixel_sizes, base_mask=sc.base_mask)
    if pipe.compute_cov3D_python:
        kw["cov3D_precomp"] = to.cov3d_from_scale_rot(sc.scales.to(dt), sc.rotations.to(dt), smod)
    else:
        kw["scales"], kw["rotations"] = sc.scales.to(dt), sc.rotations.to(dt)
    if pipe.convert_SHs_python:
        d = p - cp[None]
        d = d / d.norm(dim=1, keepdim=True)
        col = torch.clamp_min(to.eval_sh_color(sc.sh_degree, sc.shs.to(dt), d) + 0.5, 0.0)
        color, _, _, _, _, aux = to.rasterize(p, sc.opacities.to(dt), view, torch.tensor([0.1, 0.2, 0.3]), colors_precomp=col, **kw)
    else:
        color, _, _, _, _, aux = to.rasterize(p, sc.opacities.to(dt), view, torch.tensor([0.1, 0.2, 0.3]), shs=sc.shs.to(dt), **kw)
    bl = aux["borderline"]
    if Gd is not None:                # the depth map as colour channel 0 with colour z and no background
        z = torch.cat([p, torch.ones(sc.P, 1, dtype=dt)], 1) @ V[:, 2]
        zc = torch.stack([z, torch.zeros_like(z), torch.zeros_like(z)], 1)
        cz, _, _, _, _, auxz = to.rasterize(p, sc.opacities.to(dt), view, torch.zeros(3), colors_precomp=zc, **kw)
        bl = bl | auxz["borderline"]
    ok = (~bl).to(dt)
    loss = (color * dL.to(dt) * ok).sum()
    if Gd is not None:
        loss = loss + (cz[0] * Gd.to(dt) * ok).sum()
    loss.backward()
    return {k: v.grad for k, v in leaves.items()}, bl


def _masked(dL, Gd, bl):
    keep = (~bl).to(torch.float32)
    return dL * keep, (Gd * keep if Gd is not None else None)


def _compare(name, cg, og, ceil=CEIL):
    errs = {}
    for k, ref in og.items():
        got = cg[k].detach().double().cpu().reshape(-1)
        ref = ref.reshape(-1)
        scale = ref.abs().max().item()
        assert scale > 0, (name, k)
        errs[k] = (got - ref).abs().max().item() / scale
        report(name, f"camera grad {k} max|g - g64| / max|g64|", errs[k])
    if "V" in cg:
        assert torch.all(cg["V"].detach().reshape(4, 4)[:, 3] == 0), name          # V column 3 never enters
    if "PM" in cg:
        assert torch.all(cg["PM"].detach().reshape(4, 4)[:, 2] == 0), name         # PM column 2 never enters
    for k, e in errs.items():
        assert e <= ceil, f"{name}: {k} off by {e:.3e} of its scale (ceiling {ceil:g})"
    return errs


# -------------------------------------------------------------------------------------------------------------------------
# 4. against float64
# -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [False, True], ids=["colour", "colour+depth"])
@pytest.mark.parametrize("kind", ["plain", "multiscale", "scaling_modifier", "cov3D_precomp", "colors_precomp"])
def test_camera_gradients_against_float64(kind, depth):
    sc, cam, st, smod, pipe = _case(kind)
    dL, Gd = _seeds()
    og, bl = _oracle(sc, cam, st, smod, pipe, dL, Gd if depth else None)
    dLm, Gdm = _masked(dL, Gd if depth else None, bl)
    _, _, cg = _hip(sc, cam, st, smod, pipe, dLm, Gdm)
    _compare(f"{kind}/{'depth' if depth else 'colour'}", cg, og)


@pytest.mark.parametrize("depth", [False, True], ids=["colour", "colour+depth"])
@pytest.mark.parametrize("entry", ["fused", "chained"])
def test_camera_gradients_of_the_raw_entries(entry, depth):
    sc, cam, st, smod, pipe = _case("multiscale")
    dL, Gd = _seeds()
    og, bl = _oracle(sc, cam, st, smod, pipe, dL, Gd if depth else None)
    dLm, Gdm = _masked(dL, Gd if depth else None, bl)
    _, _, cg = _hip(sc, cam, st, smod, pipe, dLm, Gdm, entry=entry)
    _compare(f"{entry}/{'depth' if depth else 'colour'}", cg, og)


@pytest.mark.parametrize("entry", ["plain", "chained"])
def test_projection_built_from_the_view_matrix(entry):
    """PM = V @ proj in torch: autograd adds the projection path to V's own"""
    sc, cam, st, smod, pipe = _case("plain")
    dL, Gd = _seeds()
    og, bl = _oracle(sc, cam, st, smod, pipe, dL, Gd, pm_from_v=True)
    dLm, Gdm = _masked(dL, Gd, bl)
    _, _, cg = _hip(sc, cam, st, smod, pipe, dLm, Gdm, entry=entry, pm_from_v=True)
    assert set(cg) == {"V", "cp"}
    _compare(f"V@proj/{entry}", cg, og)


# -------------------------------------------------------------------------------------------------------------------------
# 5. translation identity on every route
# -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,kind", [("default", "plain"), ("gen1", "plain"), ("gen2", "plain"), ("fine", "plain"),
                                        ("default", "multiscale"), ("default", "slab"), ("default", "occlusion")])
@pytest.mark.parametrize("depth", [False, True], ids=["colour", "colour+depth"])
def test_translation_identity(route, kind, depth):
    """-sum_k dL/dV[12+k] V[4j+k] - sum_k dL/dPM[12+k] PM[4j+k] + dL/dcampos_j = -sum_i dL/dmeans3D_ij"""
    sc, cam, st, smod, pipe, env = _scene(kind)
    _set_route(route)
    w, h = cam.image_width, cam.image_height
    dL, Gd = scenes.grad_seed(w, h, 83), scenes.grad_seed(w, h, 84)[0] * 0.1
    with _env(env):
        reset_forward_state()
        dgr.chain_reference_getters = False
        from gaussian_renderer import render
        pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
        c, leaves = _leaf_camera(cam)
        out = render(c, pc, pipe, torch.tensor([0.1, 0.2, 0.3], device="cuda"), scaling_modifier=smod, **st)
        loss = (out["render"] * dL.cuda()).sum() + ((out["depth"] * Gd.cuda()).sum() if depth else 0.0)
        loss.backward()
        torch.cuda.synchronize()
    gV, gPM, gc = (leaves[k].grad.double().cpu().reshape(-1) for k in ("V", "PM", "cp"))
    V, PM = c.world_view_transform.detach().double().cpu().reshape(-1), c.full_proj_transform.detach().double().cpu().reshape(-1)
    gm = pc._xyz.grad.double().cpu()
    lhs = torch.stack([-sum(gV[12 + k] * V[4 * j + k] for k in range(4)) - sum(gPM[12 + k] * PM[4 * j + k] for k in range(4))
                       + gc[j] for j in range(3)])
    rhs = -gm.sum(0)
    scale = gm.abs().sum(0).max().item()
    err = (lhs - rhs).abs().max().item() / scale
    report(f"translation/{route}/{kind}", "|camera side - Gaussian side| / sum|dL/dmeans3D|", err)
    assert (pc._xyz.grad != 0).any()
    assert err <= IDENTITY_CEIL, (lhs, rhs)


# -------------------------------------------------------------------------------------------------------------------------
# 6. rotation identity
# -------------------------------------------------------------------------------------------------------------------------
def test_rotation_identity():
    """rotating the camera about its centre = rotating every mean and covariance the other way about it: the twist's
    directional derivative (camera gradients composed through posed_camera) against the one formed from dL/dmeans3D and
    dL/dcov3D_precomp (constant colours: colour is then not view dependent)"""
    from camera_pose import posed_camera
    from gaussian_renderer import _settings
    sc, cam, _, _, _ = _case("cov3D_precomp")
    dt = torch.float64
    m = sc.means3D.to("cuda", torch.float32).clone().requires_grad_(True)
    cov = to.cov3d_from_scale_rot(sc.scales.to(dt), sc.rotations.to(dt), 1.0).to("cuda", torch.float32).clone().requires_grad_(True)
    col = torch.rand(sc.P, 3, generator=torch.Generator().manual_seed(3)).cuda()
    op = sc.opacities.to("cuda", torch.float32).reshape(-1, 1)
    twist = torch.zeros(6, device="cuda", requires_grad=True)
    camd = cam.to("cuda")
    c = posed_camera(camd, twist)
    bg = torch.tensor([0.1, 0.2, 0.3], device="cuda")
    rs = _settings(c, types.SimpleNamespace(active_sh_degree=0), PIPE, bg, 1.0, False, False, 1.0)
    m2 = torch.zeros_like(m, requires_grad=True)
    img = dgr.GaussianRasterizer(rs)(means3D=m, means2D=m2, opacities=op, colors_precomp=col, cov3D_precomp=cov)[0]
    (img * scenes.grad_seed(W, H, 85).cuda()).sum().backward()
    torch.cuda.synchronize()
    omega = torch.tensor([0.3, -0.5, 0.8], dtype=dt)
    omega = omega / omega.norm()
    d_cam = (twist.grad.double().cpu()[:3] * omega).sum().item()
    Vm = camd.world_view_transform.double().cpu()
    Rw, T = Vm[:3, :3].T, Vm[3, :3]                      # W2C rotation and translation
    ox = torch.tensor([[0.0, -omega[2], omega[1]], [omega[2], 0.0, -omega[0]], [-omega[1], omega[0], 0.0]], dtype=dt)
    p = m.detach().double().cpu()
    t = p @ Rw.T + T
    dp = (t @ ox.T) @ Rw                                 # R^T [w]x t, per row
    Om = Rw.T @ ox @ Rw
    S = cov.detach().double().cpu()
    Sm = torch.stack([S[:, 0], S[:, 1], S[:, 2], S[:, 1], S[:, 3], S[:, 4], S[:, 2], S[:, 4], S[:, 5]], 1).view(-1, 3, 3)
    dS = Om @ Sm + Sm @ Om.T
    dSp = torch.stack([dS[:, 0, 0], dS[:, 0, 1], dS[:, 0, 2], dS[:, 1, 1], dS[:, 1, 2], dS[:, 2, 2]], 1)
    gm, gcov = m.grad.double().cpu(), cov.grad.double().cpu()
    terms = torch.cat([(gm * dp).reshape(-1), (gcov * dSp).reshape(-1)])
    d_world = terms.sum().item()
    err = abs(d_cam - d_world) / terms.abs().sum().item()
    report("rotation", "|camera side - world side| / sum|terms|", err)
    assert abs(d_world) > 1e-3 * terms.abs().sum().item()
    assert err <= IDENTITY_CEIL, (d_cam, d_world)


# -------------------------------------------------------------------------------------------------------------------------
# 7. verification mode
# -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [False, True], ids=["colour", "colour+depth"])
def test_verification_mode_against_float64(depth):
    sc, cam, st, smod, pipe = _case("multiscale")
    dL, Gd = _seeds()
    og, bl = _oracle(sc, cam, st, smod, pipe, dL, Gd if depth else None)
    dLm, Gdm = _masked(dL, Gd if depth else None, bl)
    prev = dgr.set_deterministic(True)
    try:
        _, _, cg = _hip(sc, cam, st, smod, pipe, dLm, Gdm)
        _, _, cg2 = _hip(sc, cam, st, smod, pipe, dLm, Gdm)
    finally:
        dgr.set_deterministic(prev)
    for k in cg:
        assert torch.equal(cg[k], cg2[k]), k
    _compare(f"verification/{'depth' if depth else 'colour'}", cg, og)


# -------------------------------------------------------------------------------------------------------------------------
# 8. no side effects, reproducible, NULL camera pointers = msgs_backward_with_depth
# -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["plain", "fused", "chained"])
def test_no_side_effects_and_bit_reproducible(entry):
    sc, cam, st, smod, pipe = _case("multiscale")
    dL, Gd = _seeds()
    out0, g0, cg0 = _hip(sc, cam, st, smod, pipe, dL, Gd, entry=entry, camera_grad=False)
    assert cg0 == {}
    out1, g1, cg1 = _hip(sc, cam, st, smod, pipe, dL, Gd, entry=entry)
    out2, g2, cg2 = _hip(sc, cam, st, smod, pipe, dL, Gd, entry=entry)
    for k in ("render", "depth", "acc_pixel_size", "radii"):
        assert torch.equal(out0[k], out1[k]), k
    for k in g0:
        assert (g0[k] is None) == (g1[k] is None), k
        if g0[k] is not None:
            assert torch.equal(g0[k], g1[k]), k
    for k in ("V", "PM", "cp"):
        assert cg1[k] is not None and torch.equal(cg1[k], cg2[k]), k
        assert cg1[k].abs().max() > 0, k


def test_null_camera_pointers_are_the_depth_entry(monkeypatch):
    """msgs_backward_with_camera with three NULL camera pointers: the same bits as msgs_backward_with_depth"""
    sc, cam, st, smod, pipe = _case("multiscale")
    dL, Gd = _seeds()
    _, g0, _ = _hip(sc, cam, st, smod, pipe, dL, Gd, entry="fused", camera_grad=False)
    calls = []

    def via_camera_entry(lib, call, ctx, geom, binning, image, D, dLc, dL_ddepth, scratch, grads, stream, camera=None):
        assert camera is None
        calls.append(1)
        dgr._C.check(lib.msgs_backward_with_camera(
            call.view_ref, call.g_ref, dgr._ptr(ctx.radii), dgr._ptr(geom), geom.numel(), D, dgr._ptr(binning), binning.numel(),
            dgr._ptr(image), image.numel(), dgr._ptr(dLc), dgr._ptr(dL_ddepth), dgr._ptr(scratch), scratch.numel(),
            C.byref(grads), None, None, None, None, 0, dgr._C.timer_ptr(), stream), "msgs_backward_with_camera")
    monkeypatch.setattr(dgr, "_call_backward", via_camera_entry)
    _, g1, _ = _hip(sc, cam, st, smod, pipe, dL, Gd, entry="fused", camera_grad=False)
    assert calls
    for k in g0:
        if g0[k] is not None:
            assert torch.equal(g0[k], g1[k]), k


# -------------------------------------------------------------------------------------------------------------------------
# 9. two views in flight
# -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accumulate_in_kernel", [True, False])
def test_two_views_in_flight(accumulate_in_kernel):
    """ViewPipeline.train_views: each view's camera gradients bit-identical to a serial run"""
    from gaussian_renderer import render
    from multi_view import ViewPipeline
    Wv, Hv, nv = 320, 200, 4
    sc = scenes.ball_scene(60000, seed=45, log_s=-3.0)
    dLs = [scenes.grad_seed(Wv, Hv, 95 + v).cuda() for v in range(nv)]
    bg = torch.tensor([0.1, 0.2, 0.3], device="cuda")
    st = dict(filter_small=False, filter_large=False, fade_size=1.0)
    reset_forward_state()
    ref = SyntheticGaussians(sc, "cuda")
    ref_cams = [_leaf_camera(scenes.ring_camera(v, nv, Wv, Hv)) for v in range(nv)]
    for (c, _), dL in zip(ref_cams, dLs):
        (render(c, ref, PIPE, bg, **st)["render"] * dL).sum().backward()
    torch.cuda.synchronize()
    pc = SyntheticGaussians(sc, "cuda")
    cams = [_leaf_camera(scenes.ring_camera(v, nv, Wv, Hv)) for v in range(nv)]

    def bwd(i, pkg):
        (pkg["render"] * dLs[i]).sum().backward()
        return pkg["viewspace_points"]
    ViewPipeline("cuda", n_streams=2).train_views([c for c, _ in cams], pc, PIPE, bg, bwd,
                                                  accumulate_in_kernel=accumulate_in_kernel, **st)
    torch.cuda.synchronize()
    for i in range(nv):
        for k in ("V", "PM", "cp"):
            assert torch.equal(cams[i][1][k].grad, ref_cams[i][1][k].grad), (i, k)
    for n in pc.LEAVES:
        assert torch.equal(getattr(pc, n).grad, getattr(ref, n).grad), n


# -------------------------------------------------------------------------------------------------------------------------
# 10. edge cases and refusals
# -------------------------------------------------------------------------------------------------------------------------
def test_empty_scene_gives_zero_camera_gradients():
    from gaussian_renderer import render
    sc, cam, st, smod, pipe = _case("plain")
    sc0 = sc.subset(torch.zeros(0, dtype=torch.long))
    pc = SyntheticGaussians(sc0, "cuda", requires_grad=True)
    c, leaves = _leaf_camera(cam)
    out = render(c, pc, pipe, torch.tensor([0.1, 0.2, 0.3], device="cuda"))
    ((out["render"] * scenes.grad_seed(W, H, 86).cuda()).sum() + out["depth"].sum()).backward()
    for k, v in leaves.items():
        assert v.grad is not None and v.grad.shape == v.shape and torch.all(v.grad == 0), k


def test_optimizer_in_backward_with_a_camera_leaf_is_refused():
    from gaussian_renderer import render_fused
    sc, cam, st, smod, pipe = _case("plain")
    pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
    c, _ = _leaf_camera(cam)
    prev = dgr.set_optimizer_in_backward(object())
    try:
        with pytest.raises(ValueError, match="set_optimizer_in_backward"):
            render_fused(c, pc, pipe, torch.tensor([0.1, 0.2, 0.3], device="cuda"))
    finally:
        dgr.set_optimizer_in_backward(prev)


def test_camera_without_grad_returns_none_and_keeps_dtype():
    """only the tensors that require grad get one, in their own shape and dtype"""
    from gaussian_renderer import render
    sc, cam, st, smod, pipe = _case("plain")
    pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
    c = copy.copy(cam.to("cuda"))
    cp = c.camera_center.double().requires_grad_(True)
    c.camera_center = cp
    V = c.world_view_transform
    out = render(c, pc, pipe, torch.tensor([0.1, 0.2, 0.3], device="cuda"))
    (out["render"] * scenes.grad_seed(W, H, 87).cuda()).sum().backward()
    assert V.grad is None and cp.grad is not None and cp.grad.dtype == torch.float64 and cp.grad.abs().max() > 0


# -------------------------------------------------------------------------------------------------------------------------
# 11. end to end: pose refinement
# -------------------------------------------------------------------------------------------------------------------------
def test_pose_refinement_recovers_the_pose():
    from camera_pose import posed_camera, projection_of
    from gaussian_renderer import render
    sc, cam = small_scene(6000, W, H, seed=36)
    pc = SyntheticGaussians(sc, "cuda", requires_grad=False)
    camd = cam.to("cuda")
    proj = projection_of(cam)
    bg = torch.tensor([0.1, 0.2, 0.3], device="cuda")
    with torch.no_grad():
        target = render(camd, pc, PIPE, bg)["render"]
    zmed = sc.means3D[:, 2].median().item()                          # front camera at the origin: depth = z
    ax = torch.tensor([0.3, -0.6, 0.2])
    ax = ax / ax.norm()
    dirn = torch.tensor([1.0, 0.5, -0.4])
    dirn = dirn / dirn.norm()
    twist0 = torch.cat([ax * math.radians(1.0), dirn * 0.02 * zmed])
    twist = twist0.clone().cuda().requires_grad_(True)
    opt = torch.optim.Adam([twist], lr=4e-3)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.98)
    for _ in range(200):
        opt.zero_grad()
        img = render(posed_camera(camd, twist, proj), pc, PIPE, bg)["render"]
        (img - target).abs().mean().backward()
        opt.step()
        sched.step()
    tw = twist.detach().cpu()
    rot0, tr0 = twist0[:3].norm().item(), twist0[3:].norm().item()
    rot1, tr1 = tw[:3].norm().item(), tw[3:].norm().item()
    report("pose", "rotation error after / before", rot1 / rot0)
    report("pose", "translation error after / before", tr1 / tr0)
    # measured on the MI355X: rotation 4.9e-4, translation 1.3e-4 of the initial error (the issue's floor was 0.1)
    assert rot1 <= 5e-3 * rot0 and tr1 <= 5e-3 * tr0, (rot0, rot1, tr0, tr1)
