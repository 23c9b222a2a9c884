"""Gradients through the rendered depth map (D_p = sum_i z_i alpha_i T_i, no background term;
include/msgs.h msgs_backward_with_depth).

The depth map is exactly a colour channel whose per-Gaussian colour is the view depth z_i and whose background is 0, so the
reference for every depth gradient is the colour route of the same op: a render with override_color = [z, 0, 0] (z computed
in torch from the means, differentiable) and bg = 0, loss on channel 0.  Both runs go through HIP; they must agree within the
HIP-vs-HIP ceilings of tests/test_fused_gpu.py, on every backward route.  A loss that does not use depth takes the colour-only
path bit for bit."""
import contextlib
import copy
import types

import pytest
import torch

import diff_gaussian_rasterization as dgr
import scenes
from parity_utils import PIPE, check_backward, leaf_space, rel_err, report, small_scene
from route_utils import PLAIN, reset_forward_state, slab_stats
from synthetic_model import SyntheticGaussians

pytestmark = pytest.mark.gpu

W, H = 160, 96
TOL = {"xyz": 5e-6, "opacity": 5e-6, "viewspace": 5e-6, "scaling": 2e-4, "rotation": 2e-4}
# Linearity: one backward of (colour + depth) against the sum of the two separate backwards.  Every tensor is held to 1e-6 except
# dL/dscaling and dL/drotation: the combined run rounds g_i = colour + z dL/dD and each tile's float32 sums once instead of twice,
# an ulp-level difference that the conic -> 2-D covariance -> 3-D covariance chain of the per-Gaussian backward amplifies by the
# squared aspect ratio (100-850x, tests/test_k8_isolation_gpu.py).  Measured on this scene over the four routes, plain and
# fused: scaling 3.7e-6 .. 9.3e-6, rotation 2.4e-6 .. 4.9e-6; every other tensor <= 3.7e-7.
LIN_TOL = {"scaling": 2e-5, "rotation": 1e-5}
ROUTES = {"default": (0, 0), "gen1": (1, 0), "gen2": (2, 0), "fine": (0, 2)}
MS = dict(filter_small=True, filter_large=True, fade_size=0.0)


def _scene(kind):
    """(scene, camera, settings, scaling_modifier, pipe, env): env = wrapper state the view needs (see _env)"""
    if kind == "slab":               # two exact depth slabs forced on (test_slab_gpu.py's dense scene)
        from test_slab_gpu import _dense_scene
        Ws, Hs = 960, 720
        return (_dense_scene(80_000, Ws, Hs, 9, opacity=(0.5, 0.99)), scenes.front_camera(Ws, Hs), PLAIN, 1.0, PIPE,
                {"slab": "0.12"})
    if kind == "occlusion":          # filters off, giants in front: the occlusion cut-off closes blocks (test_occlusion_gpu.py)
        from test_occlusion_gpu import _giants_scene
        Wo, Ho = 420, 300
        return (_giants_scene(2500, Wo, Ho, 5, 60, giant_scale=1.2, giant_opacity=0.9), scenes.front_camera(Wo, Ho), PLAIN, 1.0,
                PIPE, {"occlusion": 1})
    return _scene_small(kind) + ({},)


def _scene_small(kind):
    if kind == "plain":
        sc, cam = small_scene(3000, W, H, seed=11)
        return sc, cam, {}, 1.0, PIPE
    if kind == "multiscale":
        sc, cam = small_scene(4000, W, H, seed=12, multiscale=True, scale_k=0.004 * 1920.0 / W * 0.25)
        return sc, cam, MS, 1.0, PIPE
    if kind == "scaling_modifier":
        sc, cam = small_scene(3000, W, H, seed=13)
        return sc, cam, {}, 0.7, PIPE
    if kind == "cov3D_precomp":
        sc, cam = small_scene(3000, W, H, seed=14)
        return sc, cam, {}, 1.0, types.SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=True, debug=False)
    raise KeyError(kind)


def _set_route(route):
    gen, gran = ROUTES[route]
    dgr._C.lib.msgs_set_backward_generation(gen)
    dgr._C.lib.msgs_set_blend_granularity(gran)


@contextlib.contextmanager
def _env(env):
    """slab policy / occlusion switch a scene needs, restored afterwards"""
    prev_slab = dgr.slab_policy
    prev_occ = dgr._C.lib.msgs_set_occlusion(env["occlusion"]) if "occlusion" in env else None
    dgr.slab_policy = env.get("slab", prev_slab)
    try:
        yield
    finally:
        dgr.slab_policy = prev_slab
        if prev_occ is not None:
            dgr._C.lib.msgs_set_occlusion(prev_occ)


@pytest.fixture(autouse=True)
def _reset_routes():
    yield
    dgr._C.lib.msgs_set_backward_generation(0)
    dgr._C.lib.msgs_set_blend_granularity(0)


def _view_z(pc, cam):
    V = cam.world_view_transform.to(pc._xyz.device)            # row-vector convention: p_view = [p, 1] @ V
    return pc.get_xyz @ V[:3, 2] + V[3, 2]


def _run(sc, cam, st, smod, pipe, bg, dL=None, Gd=None, colour_z=False, fused=False, env=None):
    """one forward + backward on fresh leaves; returns (out, {name: grad})"""
    from gaussian_renderer import render, render_fused
    if env:
        reset_forward_state()          # the forced routes are taken from the first call on
    pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
    camd, bgd = cam.to("cuda"), bg.to("cuda")
    if fused:
        out = render_fused(camd, pc, pipe, bgd, scaling_modifier=smod, **st)
    else:
        oc = None
        if colour_z:
            z = _view_z(pc, cam)
            oc = torch.stack([z, torch.zeros_like(z), torch.zeros_like(z)], 1)
        out = render(camd, pc, pipe, bgd, scaling_modifier=smod, override_color=oc, **st)
    loss = 0.0
    if colour_z:
        loss = (out["render"][0] * Gd).sum()
    else:
        if dL is not None:
            loss = loss + (out["render"] * dL).sum()
        if Gd is not None:
            loss = loss + (out["depth"] * Gd).sum()
    loss.backward()
    torch.cuda.synchronize()
    _run.last_ctx = out["render"].grad_fn
    g = {"xyz": pc._xyz.grad, "opacity": pc._opacity.grad, "scaling": pc._scaling.grad, "rotation": pc._rotation.grad,
         "viewspace": out["viewspace_points"].grad, "dc": pc._features_dc.grad, "rest": pc._features_rest.grad}
    return out, {k: (v.detach().clone() if v is not None else None) for k, v in g.items()}


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-20)).item()


def _seeds(w=W, h=H):
    Gd = (scenes.grad_seed(w, h, 77)[0] * 0.1).cuda()           # per-pixel dL/dD (depths are ~ 1..10)
    dL = scenes.grad_seed(w, h, 78).cuda()
    return dL, Gd


def test_depth_requires_grad_flags():
    from gaussian_renderer import render, render_fused
    sc, cam, st, smod, pipe, _ = _scene("plain")
    bg = torch.zeros(3, device="cuda")
    pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
    camd = cam.to("cuda")
    for fn in (render, render_fused):
        out = fn(camd, pc, pipe, bg, **st)
        assert out["depth"].requires_grad and out["depth"].grad_fn is not None
        assert not out["acc_pixel_size"].requires_grad
        with torch.no_grad():
            assert not fn(camd, pc, pipe, bg, **st)["depth"].requires_grad
    prev = dgr.chain_reference_getters
    try:
        for chained in (True, False):
            dgr.chain_reference_getters = chained
            out = render(camd, pc, pipe, bg, **st)
            assert out["depth"].requires_grad and not out["acc_pixel_size"].requires_grad
    finally:
        dgr.chain_reference_getters = prev


@pytest.mark.parametrize("kind", ["plain", "multiscale", "scaling_modifier", "cov3D_precomp", "slab", "occlusion"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_depth_equals_colour_channel_of_z(kind, route):
    sc, cam, st, smod, pipe, env = _scene(kind)
    _, Gd = _seeds(cam.image_width, cam.image_height)
    bg = torch.zeros(3)
    _set_route(route)
    with _env(env):
        outA, gA = _run(sc, cam, st, smod, pipe, bg, Gd=Gd, env=env)
        ctxA = _run.last_ctx
        outB, gB = _run(sc, cam, st, smod, pipe, bg, Gd=Gd, colour_z=True, env=env)
        if kind == "slab" and route != "fine":       # (the fine-grained forward never runs in slabs: blend.hip)
            assert slab_stats(ctxA)["active"] == 1
        if kind == "occlusion":
            from test_occlusion_gpu import _stats
            assert _stats(ctxA)["closed_blocks"] > 0
    # the depth map itself is the colour channel of z (same forward arithmetic up to the torch z's rounding)
    assert _rel(outA["depth"].detach(), outB["render"][0].detach()) < 1e-5
    for k, tol in TOL.items():
        if k in ("scaling", "rotation") and kind == "cov3D_precomp":
            continue
        assert gA[k] is not None and gA[k].abs().max() > 0, k
        e = _rel(gA[k], gB[k])
        assert e <= tol, f"{kind}/{route}: grad {k} rel err {e:.3e} > {tol}"
    for k in ("dc", "rest"):                                   # depth carries no colour gradient
        assert gA[k] is None or not gA[k].any(), k


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("fused", [False, True])
def test_depth_plus_colour_is_linear(route, fused):
    sc, cam, st, smod, pipe, _ = _scene("multiscale")
    dL, Gd = _seeds()
    bg = torch.tensor([0.1, 0.2, 0.3])
    _set_route(route)
    _, gc = _run(sc, cam, st, smod, pipe, bg, dL=dL, fused=fused)
    _, gd = _run(sc, cam, st, smod, pipe, bg, Gd=Gd, fused=fused)
    _, gs = _run(sc, cam, st, smod, pipe, bg, dL=dL, Gd=Gd, fused=fused)
    for k in ("xyz", "opacity", "scaling", "rotation", "viewspace", "dc", "rest"):
        ref = gc[k] + (gd[k] if gd[k] is not None else 0)
        e = _rel(gs[k], ref)
        report(f"linearity {route} fused={fused}", f"grad {k}", e)
        assert e <= LIN_TOL.get(k, 1e-6), f"{route}: grad {k} rel err {e:.3e}"


def test_colour_only_loss_takes_the_unchanged_path(monkeypatch):
    """grad_depth is None when the loss ignores depth: the backward calls msgs_backward (never msgs_backward_with_depth), and a
    loss that uses depth calls the new entry"""
    sc, cam, st, smod, pipe, _ = _scene("plain")
    dL, Gd = _seeds()
    bg = torch.tensor([0.1, 0.2, 0.3])
    calls = []
    lib = dgr._C.lib
    for name in ("msgs_backward", "msgs_backward_with_depth"):
        fn = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _fn=fn, _n=name: (calls.append(_n), _fn(*a))[1])
    for fused in (False, True):
        calls.clear()
        _, g1 = _run(sc, cam, st, smod, pipe, bg, dL=dL, fused=fused)
        assert calls == ["msgs_backward"], calls
        calls.clear()
        _run(sc, cam, st, smod, pipe, bg, dL=dL, Gd=Gd, fused=fused)
        assert calls == ["msgs_backward_with_depth"], calls
    monkeypatch.undo()
    _, g2 = _run(sc, cam, st, smod, pipe, bg, dL=dL, fused=True)
    for k in g1:
        if g1[k] is not None:
            assert torch.equal(g1[k], g2[k]), k


def test_verification_mode_depth_is_reproducible():
    sc, cam, st, smod, pipe, _ = _scene("multiscale")
    dL, Gd = _seeds()
    bg = torch.tensor([0.1, 0.2, 0.3])
    _, gdef = _run(sc, cam, st, smod, pipe, bg, dL=dL, Gd=Gd)
    prev = dgr.set_deterministic(True)
    try:
        _, g1 = _run(sc, cam, st, smod, pipe, bg, dL=dL, Gd=Gd)
        _, g2 = _run(sc, cam, st, smod, pipe, bg, dL=dL, Gd=Gd)
        _, gc = _run(sc, cam, st, smod, pipe, bg, dL=dL)
    finally:
        dgr.set_deterministic(prev)
    for k in g1:
        if g1[k] is not None:
            assert torch.equal(g1[k], g2[k]), k
    # the literal restatement agrees with the default kernels (different float32 evaluations of the same sums) ...
    for k in ("xyz", "opacity", "viewspace"):
        assert _rel(g1[k], gdef[k]) < 1e-4, k
    # ... and the depth term is really in it
    assert _rel(g1["xyz"], gc["xyz"]) > 1e-3


def _hip_depth(sc, cam, st, Gd, dL=None):
    """render() with a depth loss (plus a colour term when dL is given) on fresh leaves; also the activated float32 inputs the
    op saw (as parity_utils.hip_render)"""
    from gaussian_renderer import render
    pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
    with torch.no_grad():
        seen = copy.copy(sc)
        seen.scales = pc.get_scaling.detach().cpu().contiguous()
        seen.rotations = pc.get_rotation.detach().cpu().contiguous()
        seen.opacities = pc.get_opacity.detach().cpu().contiguous()
        seen.shs = pc.get_features.detach().cpu().contiguous()
        seen.means3D = pc.get_xyz.detach().cpu().contiguous()
    out = render(cam.to("cuda"), pc, PIPE, torch.zeros(3, device="cuda"), **st)
    loss = (out["depth"] * Gd.cuda()).sum()
    if dL is not None:
        loss = loss + (out["render"] * dL.cuda()).sum()
    loss.backward()
    torch.cuda.synchronize()
    return out, pc, seen, out["viewspace_points"].grad


def _z32(means3D, cam):
    """the view depth in float32 the way the forward forms it: ((m2 x + m6 y) + m10 z) + m14, no contraction"""
    V = cam.world_view_transform.to(torch.float32)
    x, y, z = means3D[:, 0], means3D[:, 1], means3D[:, 2]
    return ((V[0, 2] * x + V[1, 2] * y) + V[2, 2] * z) + V[3, 2]


# Depth against the float64 truth: the depth channel's "colour" is z (1 .. 10 here, against <= 1 for a colour), and dL/dalpha_i =
# T_i (z_i - S_i) subtracts two nearly equal depths, so every float32 evaluation loses more of dL/dalpha to cancellation than it
# does for colour.  Measured on this scene (max-norm relative, unflagged Gaussians): the float32 CPU oracle fed [z32, 0, 0] is
# 2.2e-5 (means3D), 9.1e-5 (opacity), 5.7e-5 (scaling), 2.6e-5 (rotation), 6.3e-5 (means2D) from the truth; HIP 5.3e-5, 9.1e-5,
# 1.13e-4, 3.3e-5, 1.15e-4.  The colour ceiling (1e-4) is therefore doubled for depth.
TRUTH_RTOL = 2e-4


def test_depth_gradients_against_the_float64_truth():
    """oracle/torch_oracle.py in float64 with colors_precomp = [z64, 0, 0], z64 a float64 function of the means3D leaf and bg = 0:
    autograd of sum Gd * color[0] is the truth of every depth gradient.  HIP meets TRUTH_RTOL on every tensor off the Gaussians
    either oracle build flags (the float32 oracle's own distance is reported alongside); the depth map matches color[0]."""
    from oracle import oracle_ctypes as oc
    from oracle import torch_oracle as to
    Wt, Ht = 160, 96
    sc, cam = small_scene(4000, Wt, Ht, seed=123, multiscale=True, scale_k=0.004 * 1920.0 / Wt * 0.25)
    st = dict(filter_small=True, filter_large=True, fade_size=0.0)
    _, Gd = _seeds(Wt, Ht)
    Gd = Gd.cpu()
    out, pc, seen, m2 = _hip_depth(sc, cam, st, Gd)
    dt = torch.float64
    leaf = lambda t: t.detach().to(dt).clone().requires_grad_(True)
    means3D, opac, scales, rots = leaf(seen.means3D), leaf(seen.opacities), leaf(seen.scales), leaf(seen.rotations)
    V = cam.world_view_transform.to(dt)
    z64 = means3D @ V[:3, 2] + V[3, 2]
    col = torch.stack([z64, torch.zeros_like(z64), torch.zeros_like(z64)], 1)
    view = to.view_dict(cam, sh_degree=seen.sh_degree, **st)
    color, _, _, _, _, aux = to.rasterize(means3D, opac, view, torch.zeros(3, dtype=dt), scales=scales, rotations=rots,
                                          colors_precomp=col, max_pixel_sizes=seen.max_pixel_sizes,
                                          min_pixel_sizes=seen.min_pixel_sizes, base_mask=seen.base_mask)
    (color[0] * Gd.to(dt)).sum().backward()
    g2 = aux["means2D"].grad if aux["means2D"].grad is not None else torch.zeros(seen.P, 2, dtype=dt)
    m2t = torch.zeros(seen.P, 3, dtype=dt)
    m2t[:, 0], m2t[:, 1] = g2[:, 0] * 0.5 * Wt, g2[:, 1] * 0.5 * Ht
    truth = dict(means3D=means3D.grad, opacities=opac.grad, scales=scales.grad, rotations=rots.grad, means2D=m2t)
    # flags: both float32 / float64 builds of the oracle on the same colours-precomputed inputs
    c32 = torch.stack([_z32(seen.means3D, cam), torch.zeros(seen.P), torch.zeros(seen.P)], 1)
    o32 = oc.rasterize(seen, cam, st, torch.zeros(3), use_colors_precomp=True, colors_precomp=c32)
    o64 = oc.rasterize(seen, cam, st, torch.zeros(3), use_colors_precomp=True, colors_precomp=c32, f64=True)
    flagged = o32.borderline_gaussians | o64.borderline_gaussians | (o32.radii != o64.radii)
    check_backward(pc, m2, truth, "depth vs float64 truth", rtol=TRUTH_RTOL, flagged=flagged)
    og = dict(oc.backward(o32, torch.stack([Gd, torch.zeros_like(Gd), torch.zeros_like(Gd)], 0)))
    og["means3D"] = og["means3D"].double() + og["colors_precomp"][:, :1].double() * V[:3, 2][None]
    truth_leaf, orc_leaf = leaf_space(pc, m2, truth), leaf_space(pc, m2, og)
    d_orc = {k: rel_err(orc_leaf[k][1], truth_leaf[k][1], ~flagged) for k in truth_leaf}
    for k, v in d_orc.items():
        report("depth vs float64 truth", f"float32 oracle grad {k}", v)
    assert max(d_orc.values()) <= TRUTH_RTOL, d_orc              # the bound is one a float32 evaluation can meet
    okpx = ~(o32.borderline.bool() | o64.borderline.bool())
    ref = color[0].detach()
    d = (out["depth"].detach().cpu().double() - ref).abs()[okpx].max().item()
    report("depth vs float64 truth", "depth map max |HIP - truth|", d)
    assert d <= 1e-5 * max(1.0, ref.abs().max().item()), d
    for k in ("_features_dc", "_features_rest"):
        assert not getattr(pc, k).grad.any(), k


def test_verification_mode_depth_against_the_float32_oracle():
    """set_deterministic(True): a depth + colour loss against the float32 oracle (exp in double, as tests/test_literal_gpu.py)
    fed colors_precomp = [z32, 0, 0] for the depth part, z32 formed as the forward forms it; its dL/dcolors_precomp[:, 0] is
    chained to the means through the view matrix.  Held to the verification mode's flat 1e-4 over every Gaussian."""
    from oracle import oracle_ctypes as oc
    Wt, Ht = 200, 136
    sc = scenes.frustum_scene(3000, Wt, Ht, seed=3, multiscale=True, scale_k=0.004 * 1920.0 / Wt * 0.5)
    cam = scenes.front_camera(Wt, Ht)
    st = dict(filter_small=True, filter_large=True, fade_size=0.0)
    _, Gd = _seeds(Wt, Ht)
    Gd = Gd.cpu()
    prev = dgr.set_deterministic(True)
    try:
        out, pc, seen, m2 = _hip_depth(sc, cam, st, Gd)
        grads1 = [p.grad.clone() for p in (pc._xyz, pc._opacity, pc._scaling, pc._rotation)]
        out2, pc2, _, _ = _hip_depth(sc, cam, st, Gd)
        for a, p in zip(grads1, (pc2._xyz, pc2._opacity, pc2._scaling, pc2._rotation)):
            assert torch.equal(a, p.grad)                          # bit-reproducible run to run
    finally:
        dgr.set_deterministic(prev)
    c32 = torch.stack([_z32(seen.means3D, cam), torch.zeros(seen.P), torch.zeros(seen.P)], 1)
    with oc.exp_double():
        orc = oc.rasterize(seen, cam, st, torch.zeros(3), use_colors_precomp=True, colors_precomp=c32)
        og = oc.backward(orc, torch.stack([Gd, torch.zeros_like(Gd), torch.zeros_like(Gd)], 0))
    assert (out["depth"].detach().cpu() - orc.color[0]).abs().max().item() <= 1e-5 * max(1.0, orc.color[0].abs().max().item())
    og = dict(og)
    V = cam.world_view_transform.to(torch.float64)
    og["means3D"] = og["means3D"].double() + og["colors_precomp"][:, :1].double() * V[:3, 2][None]
    worst = {k: rel_err(got, ref) for k, (got, ref) in leaf_space(pc, m2, og).items()}
    report("verification depth", "worst grad rel err vs float32 oracle", max(worst.values()))
    for k, v in worst.items():
        assert v <= 1e-4, f"grad {k} rel err {v:.3e} ({worst})"


def test_optimizer_in_backward_with_a_depth_loss():
    """set_optimizer_in_backward on render_fused with a colour + depth loss: parameters and both moments bit-identical to
    FusedAdam.step() after the plain backward of the same loss (the comparison tests/test_train_step_gpu.py makes for colour)"""
    from gaussian_renderer import render_fused
    from train_epilogue import FusedAdam
    Wt, Ht = 160, 128
    sc, cam = small_scene(6007, Wt, Ht, 23, multiscale=True, scale_k=0.004 * 1920.0 / Wt * 0.2)
    st = dict(filter_small=True, filter_large=True, fade_size=0.0)
    dL, Gd = _seeds(Wt, Ht)
    bg = torch.zeros(3).cuda()
    camd = cam.to("cuda")
    a, b = SyntheticGaussians(sc, "cuda"), SyntheticGaussians(sc, "cuda")
    oa = FusedAdam(a.training_setup(7, sc.target_reso_lvl), lr=0.0, eps=1e-15)
    ob = FusedAdam(b.training_setup(7, sc.target_reso_lvl), lr=0.0, eps=1e-15)
    for it in range(4):
        taken = getattr(oa, "steps_in_backward", 0)
        prev = dgr.set_optimizer_in_backward(oa)
        try:
            pa = render_fused(camd, a, PIPE, bg, **st)
        finally:
            dgr.set_optimizer_in_backward(prev)
        ((pa["render"] * dL).sum() + (pa["depth"] * Gd).sum()).backward()
        assert getattr(oa, "steps_in_backward", 0) == taken + 1
        pb = render_fused(camd, b, PIPE, bg, **st)
        ((pb["render"] * dL).sum() + (pb["depth"] * Gd).sum()).backward()
        ob.step()
        ob.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        assert all(getattr(a, n).grad is None for n in a.LEAVES)
        assert torch.equal(pa["depth"], pb["depth"]), it
    for n in a.LEAVES:
        p, q = getattr(a, n), getattr(b, n)
        assert torch.equal(p, q), n
        sa, sb = oa.state[p], ob.state[q]
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), n
        assert sa["exp_avg"].abs().max().item() > 0, n


@pytest.mark.parametrize("share_getters,accumulate_in_kernel", [(False, False), (True, True)])
def test_two_views_in_flight_with_a_depth_loss(share_getters, accumulate_in_kernel):
    """ViewPipeline.train_views with a backward_fn whose loss includes depth: leaf gradients and per-view means2D gradients
    bit-identical to the serial loop over the same views (the tolerance of tests/test_multi_view_gpu.py)"""
    from gaussian_renderer import render
    from multi_view import ViewPipeline
    Wv, Hv, nv = 320, 200, 4
    sc = scenes.ball_scene(60000, seed=44, log_s=-3.0)
    cams = [scenes.ring_camera(v, nv, Wv, Hv).to("cuda") for v in range(nv)]
    dLs = [scenes.grad_seed(Wv, Hv, 90 + v).cuda() for v in range(nv)]
    Gds = [(scenes.grad_seed(Wv, Hv, 60 + v)[0] * 0.1).cuda() for v in range(nv)]
    bg = torch.tensor([0.1, 0.2, 0.3], device="cuda")
    st = dict(filter_small=False, filter_large=False, fade_size=1.0)
    reset_forward_state()
    ref = SyntheticGaussians(sc, "cuda")
    ref_m2 = []
    for cam, dL, Gd in zip(cams, dLs, Gds):
        o = render(cam, ref, PIPE, bg, **st)
        ((o["render"] * dL).sum() + (o["depth"] * Gd).sum()).backward()
        ref_m2.append(o["viewspace_points"].grad.clone())
    torch.cuda.synchronize()
    pc = SyntheticGaussians(sc, "cuda")

    def bwd(i, pkg):
        ((pkg["render"] * dLs[i]).sum() + (pkg["depth"] * Gds[i]).sum()).backward()
        return pkg["viewspace_points"]
    vs = ViewPipeline("cuda", n_streams=2).train_views(cams, pc, PIPE, bg, bwd, share_getters=share_getters,
                                                        accumulate_in_kernel=accumulate_in_kernel, **st)
    torch.cuda.synchronize()
    for i in range(nv):
        assert torch.equal(vs[i].grad, ref_m2[i]), i
    for n in pc.LEAVES:
        assert torch.equal(getattr(pc, n).grad, getattr(ref, n).grad), n
