"""Absgrad on the GPU (SPEC M10; include/msgs.h msgs_absgrad): after the backward of a render made with
absgrad=True, viewspace_points.absgrad = (sum over pixels of |that pixel's share of dL/dmean2D| in x and y, 0).

Two truths, both independent of the kernel under test:
  A  float64, from oracle/torch_oracle.py alone: tests/golden/absgrad_truth.npz (scene F; generator and the CPU test that pins
     it: tests/golden/make_absgrad_golden.py, tests/test_absgrad_cpu.py).  The pixels the oracle flags as borderline carry
     dL = 0 on both sides.
  B  the op's own decomposition: one backward of a plain (absgrad=False) render per pixel, with dL / dL_ddepth / dL_dalpha zeroed
     outside that pixel; sum_p |viewspace.grad_p| is the truth, sum_p viewspace.grad_p must reproduce the full gradient.
Both are compared with parity_utils.rel_err against BWD_RTOL, the project's gradient tolerance; the measured maxima are printed
(pytest -s) and recorded in profiles/absgrad_notes.md.  Then: a loss on one pixel (absgrad == |grad|), the invariants, the
untouched default path, the entries (two views in flight, depth slabs, occlusion cut-off), the densification statistic and
the guards.
The float64 truth here lives on one 3 x 2-tile picture; for the breadth (lists of several 256-entry batches, early termination,
filters with a fade, rigid poses, focal lengths, the scaling modifier, small models) see the seeded sweep of all opt-in outputs
against the same kind of truth: tests/test_replay_sweep_gpu.py, tests/replay_cases.py, tests/replay_truth.py."""
import contextlib
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import diff_gaussian_rasterization as dgr
import scenes
from parity_utils import BWD_RTOL, PIPE, rel_err, report, small_scene
from route_utils import PLAIN, assert_identical, reset_forward_state, result
from synthetic_model import SyntheticGaussians
from test_depth_grad_gpu import ROUTES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BG = (0.2, 0.4, 0.1)


@pytest.fixture(autouse=True)
def _reset_routes():
    yield
    dgr._C.lib.msgs_set_backward_generation(0)
    dgr._C.lib.msgs_set_blend_granularity(0)


def _set_route(route):
    gen, gran = ROUTES[route]
    dgr._C.lib.msgs_set_backward_generation(gen)
    dgr._C.lib.msgs_set_blend_granularity(gran)


@contextlib.contextmanager
def _env(slab=None, occlusion=None):
    """slab policy / occlusion switch of a view, restored afterwards; the forced routes are taken from the first call on"""
    prev_slab = dgr.slab_policy
    prev_occ = dgr._C.lib.msgs_set_occlusion(occlusion) if occlusion is not None else None
    if slab is not None:
        dgr.slab_policy = slab
    reset_forward_state()
    try:
        yield
    finally:
        dgr.slab_policy = prev_slab
        if prev_occ is not None:
            dgr._C.lib.msgs_set_occlusion(prev_occ)


def _render_absgrad(sc, cam, bg, dL, Gd=None, Ga=None, fused=False, st=PLAIN):
    """forward + backward of render_with_absgrad on fresh leaves -> (out, pc); dL [3,H,W], Gd / Ga [H,W] or None (device)"""
    from gaussian_renderer import render_with_absgrad
    pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
    out = render_with_absgrad(cam.to("cuda"), pc, PIPE, bg.to("cuda"), fused=fused, alpha=Ga is not None, **st)
    loss = (out["render"] * dL).sum()
    if Gd is not None:
        loss = loss + (out["depth"] * Gd).sum()
    if Ga is not None:
        loss = loss + (out["alpha"] * Ga).sum()
    loss.backward()
    torch.cuda.synchronize()
    return out, pc


def _scene_f():
    sc, cam = small_scene(200, 40, 24, seed=1)
    return sc, cam, torch.tensor(BG), scenes.grad_seed(40, 24, 78)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. truth A: float64, independent of the op
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def truth_a():
    t = np.load(os.path.join(ROOT, "tests", "golden", "absgrad_truth.npz"))
    assert t["borderline"].sum() <= 0.02 * t["borderline"].size         # the condition of the masking (scene F: 1 of 960)
    return {k: torch.from_numpy(t[k]) for k in t.files}


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("route", list(ROUTES))
def test_absgrad_against_float64_truth(truth_a, route, fused):
    sc, cam, bg, dL = _scene_f()
    dL = (dL * (~truth_a["borderline"])[None]).cuda()
    _set_route(route)
    out, _ = _render_absgrad(sc, cam, bg, dL, fused=fused)
    a = out["viewspace_points"].absgrad
    assert a.shape == (200, 3) and a.dtype == torch.float32
    assert torch.equal((out["radii"] > 0).cpu(), truth_a["visible"])
    e = rel_err(a[:, :2], truth_a["absgrad"])
    report(f"absgrad truth A [{route}{', fused' if fused else ''}]", "rel err", e)
    assert e <= BWD_RTOL


# ---------------------------------------------------------------------------------------------------------------------------
# 2. truth B: the op's own per-pixel decomposition
# ---------------------------------------------------------------------------------------------------------------------------
def _scene_b(kind):
    """(scene, camera, dL, Gd, Ga): Gd / Ga = seeds of the depth and the alpha map (scene F only)"""
    if kind == "F":                  # colour + depth + alpha seeds together
        sc, cam, _, dL = _scene_f()
        return sc, cam, dL, scenes.grad_seed(40, 24, 77)[0] * 0.1, scenes.grad_seed(40, 24, 79)[1]
    if kind == "deep":               # every tile list spans several 256-entry batches; 24 x 20: partial tiles in x and y
        sc, cam = small_scene(3000, 24, 20, seed=3)
        sc.opacities = 0.02 + 0.04 * torch.rand(sc.opacities.shape, generator=torch.Generator().manual_seed(3))
        return sc, cam, scenes.grad_seed(24, 20, 78), None, None
    if kind == "opaque":             # early termination inside tile lists of hundreds
        sc, cam = small_scene(1500, 40, 24, seed=1, scale_k=0.192)
        return sc, cam, scenes.grad_seed(40, 24, 78), None, None
    if kind == "sparse":             # whole tiles empty; odd sizes
        sc, cam = small_scene(8, 41, 23, seed=5)
        return sc, cam, scenes.grad_seed(41, 23, 78), None, None
    raise KeyError(kind)


def _per_pixel_truth(sc, cam, bg, dL, Gd, Ga):
    """(sum_p |viewspace.grad_p|, sum_p viewspace.grad_p, the full viewspace.grad) in float64, from ONE plain forward"""
    from gaussian_renderer import render, render_with_alpha
    pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
    camd, bgd = cam.to("cuda"), bg.to("cuda")
    out = render_with_alpha(camd, pc, PIPE, bgd, **PLAIN) if Ga is not None else render(camd, pc, PIPE, bgd, **PLAIN)
    assert not hasattr(out["viewspace_points"], "absgrad")
    outs = [out["render"]] + ([out["depth"]] if Gd is not None else []) + ([out["alpha"]] if Ga is not None else [])
    seeds = [dL] + ([Gd] if Gd is not None else []) + ([Ga] if Ga is not None else [])
    vs = out["viewspace_points"]
    full, = torch.autograd.grad(outs, [vs], seeds, retain_graph=True)
    H, W = dL.shape[1:]
    one = [torch.zeros_like(s) for s in seeds]
    tot_abs = torch.zeros(vs.shape, dtype=torch.float64, device="cuda")
    tot = torch.zeros_like(tot_abs)
    for y in range(H):
        for x in range(W):
            for o, s in zip(one, seeds):
                o[..., y, x] = s[..., y, x]
            g, = torch.autograd.grad(outs, [vs], one, retain_graph=True)
            tot_abs += g.abs()
            tot += g
            for o in one:
                o[..., y, x] = 0
    torch.cuda.synchronize()
    return tot_abs, tot, full.double(), out["radii"]


@pytest.mark.parametrize("kind", ["F", "deep", "opaque", "sparse"])
def test_absgrad_against_per_pixel_backwards(kind):
    sc, cam, dL, Gd, Ga = _scene_b(kind)
    bg = torch.tensor(BG)
    dL, Gd, Ga = (None if t is None else t.cuda() for t in (dL, Gd, Ga))
    tot_abs, tot, full, radii = _per_pixel_truth(sc, cam, bg, dL, Gd, Ga)
    e_method = rel_err(tot, full)
    report(f"absgrad truth B [{kind}]", "sum of per-pixel gradients vs full gradient", e_method)
    assert e_method <= BWD_RTOL                       # the method: the per-pixel backwards add up to the gradient
    assert tot_abs.abs().max().item() > 0
    out, _ = _render_absgrad(sc, cam, bg, dL, Gd, Ga)
    assert torch.equal(out["radii"], radii)
    a = out["viewspace_points"].absgrad
    e = rel_err(a[:, :2], tot_abs[:, :2])
    report(f"absgrad truth B [{kind}]", "rel err", e)
    assert e <= BWD_RTOL
    assert torch.equal(a[:, 2], torch.zeros_like(a[:, 2]))


# ---------------------------------------------------------------------------------------------------------------------------
# 3. a loss on ONE pixel: nothing to cancel, absgrad == |grad| (the image is not square: a swapped W / H scale fails)
# ---------------------------------------------------------------------------------------------------------------------------
def test_single_pixel_loss_gives_the_absolute_gradient():
    sc, cam, bg, dL = _scene_f()
    one = torch.zeros_like(dL)
    one[:, 11, 17] = dL[:, 11, 17] * 100.0
    out, _ = _render_absgrad(sc, cam, bg, one.cuda())
    a, g = out["viewspace_points"].absgrad, out["viewspace_points"].grad
    assert g.abs().max().item() > 0
    for c, name in ((0, "x"), (1, "y")):
        e = rel_err(a[:, c], g[:, c].abs())
        report("absgrad single pixel", f"{name}: rel err against |grad|", e)
        assert e <= 1e-6


# ---------------------------------------------------------------------------------------------------------------------------
# 4. invariants, and the default path untouched
# ---------------------------------------------------------------------------------------------------------------------------
def _run_result(sc, cam, bg, dL, absgrad, fused):
    from gaussian_renderer import render, render_fused, render_with_absgrad
    pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
    if absgrad:
        out = render_with_absgrad(cam, pc, PIPE, bg, fused=fused, **PLAIN)
    else:
        out = (render_fused if fused else render)(cam, pc, PIPE, bg, **PLAIN)
    out["render"].backward(dL)
    torch.cuda.synchronize()
    return result(out, pc, out["render"].grad_fn, cam.image_width, cam.image_height)


@pytest.mark.parametrize("fused", [False, True])
def test_invariants_and_untouched_defaults(fused):
    W, H = 150, 90
    sc, cam = small_scene(3000, W, H, seed=11)
    cam, bg, dL = cam.to("cuda"), torch.tensor(BG).cuda(), scenes.grad_seed(W, H, 78).cuda()
    reset_forward_state()
    plain = _run_result(sc, cam, bg, dL, False, fused)
    first = _run_result(sc, cam, bg, dL, True, fused)
    second = _run_result(sc, cam, bg, dL, True, fused)
    assert not hasattr(plain[0]["viewspace_points"], "absgrad")
    assert_identical(plain, first, "absgrad on against off")
    assert_identical(first, second, "absgrad twice")
    a, g = first[0]["viewspace_points"].absgrad, first[0]["viewspace_points"].grad
    radii = first[0]["radii"]
    assert a.shape == g.shape == (3000, 3) and a.dtype == torch.float32
    assert torch.isfinite(a).all()
    assert torch.equal(a, second[0]["viewspace_points"].absgrad)                  # two runs: equal bits
    assert torch.equal(a[:, 2], torch.zeros_like(a[:, 2]))
    assert (radii == 0).any() and torch.equal(a[radii == 0], torch.zeros_like(a[radii == 0]))
    assert (a >= 0).all() and a.max().item() > 0
    slack = (a[:, :2] - g[:, :2].abs() * (1 - 1e-5)).min().item()
    report(f"absgrad invariants [{'fused' if fused else 'plain'}]", "min of absgrad - |grad| (1 - 1e-5)", slack)
    assert slack >= 0
    assert a[:, :2].sum().item() > g[:, :2].abs().sum().item()                    # and it is not |grad|: pixels do cancel here


# ---------------------------------------------------------------------------------------------------------------------------
# 5. entries: two views in flight, depth slabs, occlusion cut-off
# ---------------------------------------------------------------------------------------------------------------------------
def test_two_views_in_flight_equal_the_serial_results():
    from gaussian_renderer import render_with_absgrad
    from multi_view import ViewPipeline
    W, H, V = 200, 128, 3
    sc = scenes.ball_scene(30000, seed=12, log_s=-3.2)
    cams = [scenes.ring_camera(v, 8, W, H).to("cuda") for v in range(V)]
    dLs = [scenes.grad_seed(W, H, 60 + v).cuda() for v in range(V)]
    bg = torch.tensor(BG).cuda()
    pc = SyntheticGaussians(sc, "cuda", requires_grad=True)

    def backward_fn(i, pkg):
        pkg["render"].backward(dLs[i])
        return pkg
    pkgs = ViewPipeline("cuda").train_views(cams, pc, PIPE, bg, backward_fn, render_fn=render_with_absgrad, share_getters=False,
                                            **PLAIN)
    torch.cuda.synchronize()
    for v in range(V):
        ref = SyntheticGaussians(sc, "cuda", requires_grad=True)
        out = render_with_absgrad(cams[v], ref, PIPE, bg, **PLAIN)
        out["render"].backward(dLs[v])
        torch.cuda.synchronize()
        a = pkgs[v]["viewspace_points"].absgrad
        assert a.abs().max().item() > 0
        assert torch.equal(a, out["viewspace_points"].absgrad), v
        assert torch.equal(pkgs[v]["viewspace_points"].grad, out["viewspace_points"].grad), v


def test_absgrad_behind_a_slab_forward():
    from test_slab_gpu import _dense_scene
    W, H = 960, 720
    sc, cam = _dense_scene(80_000, W, H, 9, opacity=(0.5, 0.99)), scenes.front_camera(W, H)
    bg, dL = torch.tensor(BG), scenes.grad_seed(W, H, 78).cuda()
    got = {}
    for policy in ("never", "0.12"):
        with _env(slab=policy):
            out, _ = _render_absgrad(sc, cam, bg, dL)
            got[policy] = out["viewspace_points"].absgrad.clone()
            if policy != "never":
                from route_utils import slab_stats
                assert slab_stats(out["render"].grad_fn)["active"] == 1
    e = rel_err(got["0.12"], got["never"])
    report("absgrad slab 0.12 vs never", "rel err", e)
    assert got["never"].abs().max().item() > 0 and e <= BWD_RTOL


def test_absgrad_behind_the_occlusion_cut_off():
    from test_occlusion_gpu import _giants_scene
    W, H = 420, 300
    sc, cam = _giants_scene(2500, W, H, 5, 60, giant_scale=1.2, giant_opacity=0.9), scenes.front_camera(W, H)
    bg, dL = torch.tensor(BG), scenes.grad_seed(W, H, 78).cuda()
    got = {}
    for occ in (0, 1):
        with _env(occlusion=occ):
            out, _ = _render_absgrad(sc, cam, bg, dL)
            got[occ] = out["viewspace_points"].absgrad.clone()
    e = rel_err(got[1], got[0])
    report("absgrad occlusion cut-off on vs off", "rel err", e)
    assert got[0].abs().max().item() > 0 and e <= BWD_RTOL


@pytest.mark.parametrize("fused", [False, True])
def test_every_trailing_input_at_once_and_retain_graph(fused):
    """camera, background and alpha-map gradients together with absgrad (the four kinds of trailing inputs of the autograd
    Functions): their gradients are those of the call without the flag, bit for bit, and a second backward through the
    retained graph ASSIGNS the attribute again while .grad accumulates"""
    import copy
    from gaussian_renderer import render_with_absgrad, render_with_alpha
    W, H = 150, 90
    sc, cam = small_scene(3000, W, H, seed=11)
    dL, Ga = scenes.grad_seed(W, H, 78).cuda(), scenes.grad_seed(W, H, 79)[1].cuda()
    got = []
    for absgrad in (False, True):
        c = copy.copy(cam.to("cuda"))
        c.world_view_transform = c.world_view_transform.clone().requires_grad_(True)
        c.full_proj_transform = c.full_proj_transform.clone().requires_grad_(True)
        c.camera_center = c.camera_center.clone().requires_grad_(True)
        bg = torch.tensor(BG, device="cuda", requires_grad=True)
        pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
        if absgrad:
            out = render_with_absgrad(c, pc, PIPE, bg, fused=fused, alpha=True, **PLAIN)
        else:
            out = render_with_alpha(c, pc, PIPE, bg, fused=fused, **PLAIN)
        loss = (out["render"] * dL).sum() + (out["alpha"] * Ga).sum()
        loss.backward(retain_graph=absgrad)
        torch.cuda.synchronize()
        got.append((out, pc, c, bg))
    (oa, pa, ca, ba), (ob, pb, cb, bb) = got
    assert not hasattr(oa["viewspace_points"], "absgrad")
    for k in ("render", "alpha", "depth", "radii"):
        assert torch.equal(oa[k], ob[k]), k
    assert torch.equal(oa["viewspace_points"].grad, ob["viewspace_points"].grad)
    for n in pa.LEAVES:
        assert torch.equal(getattr(pa, n).grad, getattr(pb, n).grad), n
    for n in ("world_view_transform", "full_proj_transform", "camera_center"):
        assert getattr(ca, n).grad.abs().max().item() > 0 and torch.equal(getattr(ca, n).grad, getattr(cb, n).grad), n
    assert ba.grad.abs().max().item() > 0 and torch.equal(ba.grad, bb.grad)
    vs = ob["viewspace_points"]
    first, g1 = vs.absgrad, vs.grad.clone()
    assert first.shape == vs.shape and first.abs().max().item() > 0
    ((ob["render"] * dL).sum() + (ob["alpha"] * Ga).sum()).backward()
    torch.cuda.synchronize()
    assert vs.absgrad is not first and torch.equal(vs.absgrad, first)              # assigned, not accumulated
    assert torch.equal(vs.grad, g1 + g1)                                           # (.grad does accumulate)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the densification statistic
# ---------------------------------------------------------------------------------------------------------------------------
def test_training_stats_accumulate_the_absgrad_norm():
    from train_epilogue import update_training_stats
    W, H = 150, 90
    sc, cam = small_scene(3000, W, H, seed=11)
    out, pc = _render_absgrad(sc, cam, torch.tensor(BG), scenes.grad_seed(W, H, 78).cuda())
    vsp, radii, ps = out["viewspace_points"], out["radii"], out["pixel_sizes"]
    pc.training_setup(4)
    gen = torch.Generator().manual_seed(9)
    pc.xyz_gradient_accum = torch.rand(3000, 4, 1, generator=gen).cuda()
    pc.denom = torch.randint(0, 5, (3000, 4, 1), generator=gen).float().cuda()
    acc0, den0 = pc.xyz_gradient_accum.clone(), pc.denom.clone()
    lvl = 2
    with torch.no_grad():
        update_training_stats(pc, vsp, radii, ps, lvl, update_pixel_sizes=False, densify=True, absgrad=True)
    vis = radii > 0
    acc0[:, lvl][vis] += torch.norm(vsp.absgrad[vis, :2], dim=-1, keepdim=True)
    den0[:, lvl][vis] += 1
    assert torch.equal(pc.denom, den0)
    assert torch.allclose(pc.xyz_gradient_accum, acc0, rtol=1e-6, atol=0)
    # the signed statistic of the same view is another number
    signed = torch.norm(vsp.grad[vis, :2], dim=-1).sum().item()
    assert torch.norm(vsp.absgrad[vis, :2], dim=-1).sum().item() > signed
    # a render without absgrad has no attribute to read: a clear error, nothing launched on garbage
    plain = types.SimpleNamespace(grad=vsp.grad)
    with pytest.raises(RuntimeError, match="absgrad"):
        update_training_stats(pc, plain, radii, ps, lvl, update_pixel_sizes=False, densify=True, absgrad=True)


def test_fused_iterations_with_absgrad_with_and_without_the_step_in_backward():
    from train_epilogue import FusedAdam
    from train_step import fused_train_iteration
    W, H = 160, 128
    sc, cam = small_scene(6007, W, H, 23, multiscale=True, scale_k=0.004 * 1920.0 / W * 0.2)
    st = dict(filter_small=True, filter_large=True, fade_size=0.0)
    gt = torch.rand(3, H, W, generator=torch.Generator().manual_seed(2)).cuda()
    bg, camd = torch.zeros(3).cuda(), cam.to("cuda")
    models = [SyntheticGaussians(sc, "cuda") for _ in range(3)]
    opts = [FusedAdam(m.training_setup(7, sc.target_reso_lvl), lr=0.0, eps=1e-15) for m in models]
    kws = [dict(absgrad=True, step_in_backward=True), dict(absgrad=True), dict()]
    for it in range(3):
        pk = [fused_train_iteration(m, o, camd, gt, PIPE, bg, **kw, **st)[2] for m, o, kw in zip(models, opts, kws)]
        assert torch.equal(pk[0]["viewspace_points"].absgrad, pk[1]["viewspace_points"].absgrad), it
        assert not hasattr(pk[2]["viewspace_points"], "absgrad")
    a, b, c = models
    for n in a.LEAVES:                                 # the flag changes the statistic, never the training step
        assert torch.equal(getattr(a, n), getattr(b, n)) and torch.equal(getattr(b, n), getattr(c, n)), n
    for k in ("denom", "max_radii2D", "max_pixel_sizes", "min_pixel_sizes", "xyz_gradient_accum"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert torch.equal(b.denom, c.denom)
    assert (b.xyz_gradient_accum >= c.xyz_gradient_accum * (1 - 1e-5)).all()
    assert b.xyz_gradient_accum.sum().item() > c.xyz_gradient_accum.sum().item()


# ---------------------------------------------------------------------------------------------------------------------------
# 7. guards
# ---------------------------------------------------------------------------------------------------------------------------
def test_verification_mode_refuses_absgrad_before_any_launch():
    from gaussian_renderer import render_with_absgrad
    sc, cam, bg, _ = _scene_f()
    pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
    before = dgr.forward_stats["forwards"]
    prev = dgr.set_deterministic(True)
    try:
        for fused in (False, True):
            with pytest.raises(ValueError, match="verification mode"):
                render_with_absgrad(cam.to("cuda"), pc, PIPE, bg.cuda(), fused=fused, **PLAIN)
    finally:
        dgr.set_deterministic(prev)
    assert dgr.forward_stats["forwards"] == before


def test_no_gaussians_gives_an_empty_absgrad():
    rs = dgr.GaussianRasterizationSettings(24, 40, 0.5, 0.3, torch.tensor(BG).cuda(), 1.0, torch.eye(4).cuda(), torch.eye(4).cuda(),
                                           3, torch.zeros(3).cuda(), False, False)
    z = lambda *s: torch.zeros(*s, device="cuda")
    m3, m2 = z(0, 3).requires_grad_(), z(0, 3).requires_grad_()
    out = dgr.GaussianRasterizer(rs, absgrad=True)(means3D=m3, means2D=m2, opacities=z(0, 1), shs=z(0, 16, 3), scales=z(0, 3),
                                                   rotations=z(0, 4))
    assert not hasattr(m2, "absgrad")
    out[0].sum().backward()
    assert m2.absgrad.shape == (0, 3) and m2.absgrad.dtype == torch.float32 and m2.absgrad.is_cuda


def test_no_grad_forward_leaves_no_attribute():
    from gaussian_renderer import render_with_absgrad
    sc, cam, bg, _ = _scene_f()
    pc = SyntheticGaussians(sc, "cuda", requires_grad=False)
    with torch.no_grad():
        out = render_with_absgrad(cam.to("cuda"), pc, PIPE, bg.cuda(), **PLAIN)
    torch.cuda.synchronize()
    assert not hasattr(out["viewspace_points"], "absgrad")


def test_c_entry_checks_capacity_and_arguments():
    from gaussian_renderer import render
    sc, cam, bg, dL = _scene_f()
    pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
    out = render(cam.to("cuda"), pc, PIPE, bg.cuda(), **PLAIN)
    ctx = out["render"].grad_fn
    geom, binning, image, D = dgr._resolve(ctx.state)
    lib, call, P = dgr._C.lib, ctx.call, ctx.call.P
    need = lib.msgs_absgrad_scratch_bytes(P)
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    res = torch.full((P, 3), 7.0, device="cuda")
    dLc = dL.cuda().contiguous()
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def entry(image_bytes=image.numel(), scratch_bytes=need, dl=p(dLc), n=P):
        return lib.msgs_absgrad(call.view_ref, n, p(geom), geom.numel(), D, p(binning), binning.numel(), p(image), image_bytes,
                                dl, None, None, p(scratch), scratch_bytes, p(res), stream)
    assert entry(scratch_bytes=need - 1) == -2                    # MSGS_ERR_CAPACITY
    assert entry(image_bytes=lib.msgs_image_bytes(40, 24) - 1) == -2
    assert entry(dl=None) == -1                                   # MSGS_ERR_INVALID_ARG
    assert entry(n=-1) == -1
    torch.cuda.synchronize()
    assert torch.equal(res, torch.full_like(res, 7.0))            # refused calls wrote nothing
    assert entry() == 0
    torch.cuda.synchronize()
    # the entry is independent of the backward calls: it serves a forward whose backward has not run
    ref, _ = _render_absgrad(sc, cam, bg, dLc)
    assert torch.equal(res, ref["viewspace_points"].absgrad)
